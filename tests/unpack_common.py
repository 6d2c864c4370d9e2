"""Shared by tests/test_unpack_cpu.py and tests/test_gpu_unpack.py: the sample extract of a ring sample restated in numpy
from the definition in include/tfhe_hip.h, the variance the header states for an unpacked sample, and what both files
reuse by import -- the key switch from its definition (tests/ks_common.py) and the ring phases and custom parameter
tuples of the packing tests (tests/pack_common.py).  Shares no code with the library."""
import numpy as np

from ks_common import keyswitch_ref                         # noqa: F401  (re-exported: the tests name it through here)
from pack_common import STDEVS, custom_tuple, ring_phases, to_i32   # noqa: F401

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def extract_ref(ring_words, index, N):
    """Extract_e of ring samples ring_words [nring][2][N] (int32) for every index[j] = r N + e -> int32 [count][N + 1]:
    b = B[e], a_i = A[e - i] for i <= e, a_i = -A[N + e - i] for i > e, wrapping mod 2^32."""
    w = np.asarray(ring_words).reshape(-1, 2, N).astype(np.int64)
    idx = np.asarray(index, dtype=np.int64).reshape(-1)
    assert idx.min() >= 0 and idx.max() < len(w) * N
    r, e = idx // N, idx % N
    i = np.arange(N)[None, :]
    below = i <= e[:, None]
    src = np.where(below, e[:, None] - i, N + e[:, None] - i)
    A = np.take_along_axis(w[r, 0], src, axis=1)
    out = np.empty((len(idx), N + 1), dtype=np.int64)
    out[:, :N] = np.where(below, A, -A)
    out[:, N] = w[r, 1, e]
    return to_i32(out)


def extracted_phases(u, tlwe_key):
    """b - sum_i a_i S_i of extracted samples u [rows][N + 1] under the extracted key (the ring key's bits), int32"""
    u = np.asarray(u).astype(np.int64)
    N = u.shape[1] - 1
    S = np.asarray(tlwe_key)[:N].astype(np.int64)
    a = u[:, :N] % 2 ** 32
    return to_i32(u[:, N] - ((a & 0xFFFF) @ S + (((a >> 16) @ S) % 2 ** 16 << 16)))


def lwe_phases(words, lwe_key):
    """b - <a, s> of LWE samples words [rows][n + 1] under the binary LWE key, int32"""
    w = np.asarray(words).astype(np.int64)
    n = w.shape[1] - 1
    return to_i32(w[:, n] - (w[:, :n] % 2 ** 32) @ np.asarray(lwe_key)[:n].astype(np.int64))


def keyswitch_rows(ksk, u, n, N, t, bb, workers=8):
    """keyswitch_ref (tests/ks_common.py) of every row of u, the rows dealt to a few threads: the same function, the same
    words -- a row's key switch reads nothing of another row's"""
    from concurrent.futures import ThreadPoolExecutor
    u = np.asarray(u)
    parts = np.array_split(np.arange(len(u)), min(4 * workers, len(u)))
    with ThreadPoolExecutor(workers) as ex:
        return np.concatenate(list(ex.map(lambda rows: keyswitch_ref(ksk, u[rows], n, N, t, bb), parts)))


def unpack_ref(ksk, params, ring_words, index):
    """what an unpack writes: keyswitch_ref(KSK words, extract_ref(ring words, index)) -> int32 [count][n + 1]"""
    pp = params
    return keyswitch_rows(ksk, extract_ref(ring_words, index, pp.N), pp.n, pp.N, pp.ks_t, pp.ks_basebit)


def unpack_variance(N, t, bb, ks_stdev, ring_stdev):
    """the first-order variance the header states for an unpacked sample (torus units): the ring sample's own, the key
    term N t ks_stdev^2 and the rounding of the N / 2 set key bits; no rotation term"""
    prec = 2.0 ** -(1 + bb * t)
    return ring_stdev ** 2 + N * t * ks_stdev ** 2 + (N / 2.0) * prec ** 2 / 3.0


def random_ring(rng, nring, N):
    return rng.integers(I32_MIN, I32_MAX + 1, size=(nring, 2, N), dtype=np.int64).astype(np.int32)
