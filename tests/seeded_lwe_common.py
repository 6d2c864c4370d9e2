"""Shared by tests/test_seeded_lwe_cpu.py and tests/test_gpu_seeded_lwe.py: seed-compressed LWE sample arrays restated from
the definition in include/tfhe_hip.h -- which stream words are the mask of sample j, what its body must be, the plain
words of an expanded sample -- over the stream of tests/compressed_common.py (block numbers and word positions computed
there, the blocks from the library's known-answer hook).  Shares no code with the encryptors, the expansion or the kernel."""
import numpy as np

import compressed_common as K
from compressed_common import centred            # noqa: F401
from pack_common import custom_tuple, to_i32   # noqa: F401
from seeded_wire_common import assert_words    # noqa: F401

MASK_SEED, NOISE_SEED = K.MASK_SEED, 0x5EED1E
KS_STDEV = 2.0 ** -15                              # ks_stdev of every set here and of P128: what bootsSymEncrypt uses
RECORD_MAX = 1 << 20
# every residue of the row start mod 8 and mod 4 (n = 7, 9, 10, 630), rows shorter than a block, one block, the widest row
DIMENSIONS = (1, 7, 8, 9, 10, 630, 1024)


def stride_of(n):
    """the words of a pool slot: n + 1 rounded up to a 16-byte group"""
    return (n + 4) & ~3


def mask_ref(L, seed, n, s):
    """the mask of sample s: stream words s n .. s n + n - 1 -> uint32 [n]"""
    return K.stream_words(L, seed, s * n, n)


def expand_ref(L, record, n, index):
    """the plain words of samples `index` of a record [10 + record_count] -> int32 [len(index)][n + 1]"""
    rec = np.ascontiguousarray(record, dtype=np.int32).reshape(-1)
    seed, masks = rec[:10].view(np.uint32), {}
    out = np.zeros((len(index), n + 1), dtype=np.int32)
    for j, s in enumerate(int(x) for x in index):
        if s not in masks:
            masks[s] = mask_ref(L, seed, n, s).view(np.int32)
        out[j, :n] = masks[s]
        out[j, n] = rec[10 + s]
    return out


def inner_u32(a, key):
    """<a, key> wrapping in uint32, a [..., n]"""
    with np.errstate(over="ignore"):
        return (np.asarray(a).view(np.uint32) * np.asarray(key).astype(np.uint32)).sum(axis=-1, dtype=np.uint32)


def phases(words, key):
    """body - <a, key> of plain samples [count][n + 1] as signed words"""
    w = np.ascontiguousarray(words, dtype=np.int32)
    with np.errstate(over="ignore"):
        return (w[:, -1].view(np.uint32) - inner_u32(w[:, :-1], key)).view(np.int32)


def fixture_noise(oracle, noise_seed, sigma, count):
    """what the _seeded encryptors add: one gaussian per sample in order from xoshiro256** started from noise_seed, as a
    Torus32 (fraction of the double times 2^32, truncated) -> int32 [count]"""
    rng = oracle.Rng(noise_seed)
    out = []
    for _ in range(count):
        d = rng.gauss(sigma)
        out.append(int((d - int(d)) * 4294967296.0))
    return to_i32(out)


def random_record(rng, record_count, seed=MASK_SEED):
    """a record of random bodies under `seed` -> int32 [10 + record_count]"""
    rec = rng.integers(-2 ** 31, 2 ** 31, size=10 + record_count, dtype=np.int64).astype(np.int32)
    rec[:10] = np.asarray(seed, dtype=np.uint32).view(np.int32)
    return rec


def index_cases(rng, record_count, total):
    """sample 0, the record's last sample, a repeat, a descending run, then random samples up to `total` indices"""
    last = record_count - 1
    run = np.arange(min(last, 12), max(min(last, 12) - 8, -1), -1)
    head = np.concatenate([[0, last, last, 0], run]).astype(np.int64)
    assert len(head) <= total
    return np.concatenate([head, rng.integers(0, record_count, total - len(head))]).astype(np.int32)
