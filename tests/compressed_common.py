"""Shared by tests/test_compressed_cpu.py and tests/test_gpu_compressed.py: the mask stream of a seed-compressed cloud key
restated from the definition in include/tfhe_hip.h (block numbers and word positions computed here, the ChaCha20 blocks
themselves from the library's known-answer hook, which tests/test_host_cpu.py pins to RFC 8439), the layouts of an expanded
key, and the custom parameter tuples of the packing tests.  Shares no code with the generator or the expansions."""
import ctypes as C

import numpy as np

from pack_common import STDEVS, custom_tuple, to_i32   # noqa: F401

MASK_SEED = np.array([0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C, 0x13121110, 0x17161514, 0x1B1A1918, 0x1F1E1D1C,
                      0x4A000000, 0x00000009], dtype=np.uint32)
NOISE_SEED = 0xC0DE5EED


def host_block(L, seed, counter):
    """ChaCha20 block `counter` (64-bit) under seed = key[8] + nonce[2] -> uint32 [16]"""
    from peba1_amd import lib
    seed = np.ascontiguousarray(seed, dtype=np.uint32)
    key, nonce, out = seed[:8].copy(), seed[8:].copy(), np.zeros(16, dtype=np.uint32)
    L.tfhe_hip_test_chacha20_block(key.ctypes.data_as(lib.U32P), C.c_uint64(int(counter)), nonce.ctypes.data_as(lib.U32P),
                                   out.ctypes.data_as(lib.U32P))
    return out


def stream_words(L, seed, first, count):
    """mask words first .. first + count - 1: word 2 (m mod 8) + 1 of block floor(m / 8) -> uint32 [count]"""
    first = int(first)
    blocks = {b: host_block(L, seed, b) for b in range(first // 8, (first + count - 1) // 8 + 1)}
    return np.array([blocks[m // 8][2 * (m % 8) + 1] for m in range(first, first + count)], dtype=np.uint32)


class Shape:
    """the sizes of a parameter set's cloud key, plain and compressed, and where mask word m lands"""

    def __init__(self, pp):
        self.n, self.N, self.k, self.l, self.t, self.bb = pp.n, pp.N, pp.k, pp.l, pp.ks_t, pp.ks_basebit
        self.kpl, self.base = (self.k + 1) * self.l, 1 << self.bb
        self.bk_words = self.n * self.kpl * (self.k + 1) * self.N
        self.ksk_words = self.k * self.N * self.t * self.base * (self.n + 1)
        self.bk_body_words = self.n * self.kpl * self.N
        self.ksk_body_words = self.k * self.N * self.t * (self.base - 1)
        self.bk_masks = self.n * self.kpl * self.k * self.N
        self.ksk_masks = self.ksk_body_words * self.n
        self.stride = (self.n + 1 + 3) & ~3

    def bk_mask_index(self, m):
        """BK mask word m -> index into bk [n][kpl][k+1][N]"""
        poly, j = divmod(m, self.N)
        row, u = divmod(poly, self.k)
        return (row * (self.k + 1) + u) * self.N + j

    def ksk_mask_index(self, m):
        """KSK mask word m (0 = the first word behind the BK's) -> index into ksk [kN][t][base][n+1]"""
        crow, q = divmod(m, self.n)
        r, v1 = divmod(crow, self.base - 1)
        return (r * self.base + v1 + 1) * (self.n + 1) + q


def compact_ksk(ksk, sh):
    """the layout the key-switch kernels read, from host words [kN][t][base][n+1]: rows of digits 1 .. base-1 padded with
    zeros to ct_stride, one all-zero row behind them -> int32 [(kN t (base-1) + 1) * stride]"""
    K = np.asarray(ksk).reshape(sh.k * sh.N * sh.t, sh.base, sh.n + 1)
    out = np.zeros((sh.ksk_body_words + 1, sh.stride), dtype=np.int32)
    out[:-1, :sh.n + 1] = K[:, 1:, :].reshape(sh.ksk_body_words, sh.n + 1)
    return out.reshape(-1)


def negacyclic_by_bits(a, bits):
    """a(X) * bits(X) mod (X^N + 1), exact in int64: a [N] with |a| < 2^32, bits binary"""
    N = len(a)
    full = np.convolve(np.asarray(a, dtype=np.int64), np.asarray(bits, dtype=np.int64))
    return full[:N] - np.concatenate([full[N:], [0]])


def centred(x):
    """a Torus32 difference as a signed integer"""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)
