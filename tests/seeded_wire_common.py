"""Shared by tests/test_seeded_wire_cpu.py and tests/test_gpu_seeded_wire.py: seed-compressed packing keys and ring samples
restated from the definitions in include/tfhe_hip.h -- where the mask polynomial of a key row lies in the stream, what a
row's phase must be, the plain words of a compressed ring sample -- over the stream of tests/compressed_common.py (block
numbers and word positions computed there, the blocks from the library's known-answer hook).  Shares no code with the
generators, the expansions or the kernels."""
import numpy as np

import compressed_common as K
from pack_common import custom_tuple, negacyclic_matrix, to_i32   # noqa: F401

MASK_SEED, NOISE_SEED = K.MASK_SEED, 0x5EEDED
SIGMA = 2.0 ** -25 * 2.0 ** 32                      # bk_stdev of every set here, in Torus32 units
TOL = 6 * SIGMA
# (t, basebit, N, gadget of the custom set): the set's own decomposition, one row of 4-bit digits, the most rows the pack
# kernel takes at either ring size
DECOMPS = [(8, 2, 1024, (3, 7)), (1, 4, 1024, (3, 7)), (18, 1, 1024, (3, 7)), (16, 2, 2048, (2, 8))]
KEY_CASES = [(n, t, bb, N, g) for (t, bb, N, g) in DECOMPS for n in (1, 7, 10)]


def seed_of(r):
    """a mask seed of its own for ring sample r"""
    return ((MASK_SEED.astype(np.uint64) + 0x01000193 * (r + 1)) % 2 ** 32).astype(np.uint32)


def row_mask_ref(L, seed, i, p, t, N):
    """the mask polynomial of key row (i, p): stream words (i t + p) N .. + N - 1 -> uint32 [N]"""
    return K.stream_words(L, seed, (i * t + p) * N, N)


def row_messages(lwe_key, t, bb):
    """mu[i][p] = lwe_key[i] << (32 - (p+1) bb), wrapping -> int32 [n][t]"""
    s = np.asarray(lwe_key, dtype=np.int64)[:, None]
    return to_i32(s << (32 - (np.arange(t, dtype=np.int64)[None, :] + 1) * bb))


def ring_phases(words, tlwe_key):
    """B - A S of TLWE samples words [..., 2, N] under the binary ring key, int32 -- pack_common.ring_phases with the product
    in float64 on the 16-bit halves of the mask words: a sum of N halves stays below 2^27, exact in a double"""
    w = np.asarray(words)
    N = w.shape[-1]
    T = negacyclic_matrix(np.asarray(tlwe_key)[:N]).astype(np.float64)
    a = w[..., 0, :].astype(np.int64) % 2 ** 32
    lo = ((a & 0xFFFF).astype(np.float64) @ T).astype(np.int64)
    hi = ((a >> 16).astype(np.float64) @ T).astype(np.int64)
    return to_i32(w[..., 1, :].astype(np.int64) - (lo + ((hi % 2 ** 16) << 16)))


def ring_expand_ref(L, compressed, N):
    """the plain 2N words of compressed records [nring][10 + N]: stream words 0 .. N-1 of each seed, then its body"""
    c = np.ascontiguousarray(compressed, dtype=np.int32).reshape(-1, 10 + N)
    out = np.zeros((len(c), 2, N), dtype=np.int32)
    for r in range(len(c)):
        out[r, 0] = K.stream_words(L, c[r, :10].view(np.uint32), 0, N).view(np.int32)
        out[r, 1] = c[r, 10:]
    return out


def random_compressed(rng, nring, N):
    """records of random bodies under seeds that differ -> int32 [nring][10 + N]"""
    c = rng.integers(-2 ** 31, 2 ** 31, size=(nring, 10 + N), dtype=np.int64).astype(np.int32)
    for r in range(nring):
        c[r, :10] = seed_of(r).view(np.int32)
    return c


def assert_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got[bad[:3]], want[bad[:3]])
