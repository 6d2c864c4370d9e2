"""Shared by tests/test_public_cpu.py and tests/test_gpu_public.py: a ring sample times public polynomials restated from the
integers of include/tfhe_hip.h ("ring sample times public polynomials") -- the negacyclic product in Python integers,
reduced mod 2^32 (term by term from the definition, and the same sums in exact int64 halves for dense operands), the sample
extraction at the entries' first coefficients, the key switch of tests/ks_common.py and the variance the header states.
Shares no code with the library."""
import numpy as np

import unpack_common as U
from pack_common import P0, P1, STDEVS, custom_tuple, forward_bound, ring_phases, to_i32   # noqa: F401

CRT_EXACT_LIMIT = P0 * P1 // 100 * 36            # ntt_field.hpp
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
RINGS = {"P128": 1024, "P2048": 2048}            # name -> N (the gadget does not enter the product)
BK_STDEVS = {"P128": 2.0 ** -25, "l2": 7.18e-9, "P2048": 2.0 ** -25}


def max_coef(N):
    """the largest power of two T with N T 2^31 < CRT_EXACT_LIMIT, in Python integers"""
    T = 1
    while N * (2 * T) * 2 ** 31 < CRT_EXACT_LIMIT:
        T *= 2
    assert N * T * 2 ** 31 < CRT_EXACT_LIMIT
    return T


def negacyclic_python(q, c):
    """q c in Z[X]/(X^N + 1) in Python integers, term by term from the definition (q may be sparse), NOT reduced"""
    N = len(c)
    c = [int(v) for v in c]
    out = [0] * N
    for i in range(N):
        qi = int(q[i])
        if qi:
            for j in range(N):
                if i + j < N:
                    out[i + j] += qi * c[j]
                else:
                    out[i + j - N] -= qi * c[j]
    return out


def negacyclic_matrix(q):
    """M with (q c)[m] = sum_j M[m][j] c[j]: M[m][j] = q[m - j] for j <= m, -q[m - j + N] past it -> int64 [N][N]"""
    q = np.asarray(q, dtype=np.int64)
    N = len(q)
    d = np.arange(N)[:, None] - np.arange(N)[None, :]
    return np.where(d >= 0, q[d % N], -q[d % N])


def product(q, c):
    """q * c for one public polynomial q [N] (|q| <= 2^11) and one ring sample c [2][N] int32 (words signed) -> int32 [2][N].
    The same sums as negacyclic_python, the words split into a signed high and an unsigned low half so that every int64 sum
    is exact (N 2^11 2^16 = 2^38); the low 32 bits are put together mod 2^32."""
    M = negacyclic_matrix(q)
    w = np.asarray(c).astype(np.int64)
    lo, hi = w & 0xFFFF, w >> 16
    return to_i32((M @ lo.T).T + (((M @ hi.T).T % 2 ** 16) << 16))


def products(polys, ring, first=0, npolys=None):
    """the three broadcast forms of tfhe_hip_ring_mul_public -> int32 [max(npolys, count)][2][N]"""
    polys, ring = np.asarray(polys), np.asarray(ring)
    npolys = len(polys) - first if npolys is None else npolys
    count = len(ring)
    assert npolys == 1 or count == 1 or npolys == count
    total = max(npolys, count)
    return np.stack([product(polys[first + (0 if npolys == 1 else g)], ring[0 if count == 1 else g]) for g in range(total)])


def monomial(c, r):
    """X^r c on both polynomials: c[u][j - r] for j >= r, -c[u][j - r + N] below it (the lookup's X^(-r) with the sign of
    the exponent flipped) -> int32 [2][N]"""
    c = np.asarray(c).astype(np.int64)
    N = c.shape[-1]
    j = np.arange(N)
    return to_i32(np.where(j >= r, c[:, (j - r) % N], -c[:, (j - r) % N]))


def inverse_monomial(c, r):
    """the lookup's X^(-r) c of include/tfhe_hip.h: c[u][j + r] for j + r < N, -c[u][j + r - N] otherwise"""
    c = np.asarray(c).astype(np.int64)
    N = c.shape[-1]
    j = np.arange(N)
    return to_i32(np.where(j + r < N, c[:, (j + r) % N], -c[:, (j + r) % N]))


def probe_poly(s, N):
    """sum_i s_i X^(-i): p[0] = s_0, p[N - i] = -s_i for 1 <= i < w, 0 elsewhere -> int64 [N]"""
    s = [int(x) for x in s]
    p = [0] * N
    p[0] = s[0]
    for i in range(1, len(s)):
        p[N - i] = -s[i]
    return np.array(p, dtype=np.int64)


def rows(polys, probe, M, w):
    """row i = Extract_((i mod S) w)(polys[i / S] * probe) for i < M -> int32 [M][N + 1]"""
    N = np.asarray(probe).shape[-1]
    per = N // w
    R = -(-M // per)
    prods = np.stack([product(polys[r], probe) for r in range(R)])
    return U.extract_ref(prods, [(i // per) * N + (i % per) * w for i in range(M)], N)


def keyswitched(ksk, params, u):
    """the key switch of tests/ks_common.py on extracted rows u [M][N + 1] -> int32 [M][n + 1]"""
    return U.keyswitch_rows(ksk, u, params.n, params.N, params.ks_t, params.ks_basebit)


def variance(norm2, ring_variance):
    """the header's variance of a coefficient of q * c before the key switch: |q|_2^2 times the ring sample's, nothing else"""
    return norm2 * ring_variance


def worst_case(N):
    """all q[j] = -T against words 0x80000000 in Python integers: (the unreduced coefficients, their largest magnitude).
    Coefficient m of the product of two constant polynomials a, b is a b ((m + 1) - (N - 1 - m))."""
    T = max_coef(N)
    coef = [(-T) * I32_MIN * ((m + 1) - (N - 1 - m)) for m in range(N)]
    return coef, max(abs(v) for v in coef)


def random_ring(rng, count, N):
    return rng.integers(I32_MIN, I32_MAX + 1, size=(count, 2, N), dtype=np.int64).astype(np.int32)
