"""Shared by tests/test_public_sum_cpu.py and tests/test_gpu_public_sum.py: sums of public-polynomial products over several
ring samples restated from the integers of include/tfhe_hip.h ("public products over several ring samples") -- the
negacyclic products in int64 with the words taken mod 2^32 (every sum is exact: terms N T 2^32 <= 2^57), added over the
terms and wrapped to 2^32 once, and the extraction at the entries' first coefficients as tests/public_common.py states it.
Shares no code with the library, and none with public_common's product (a test compares the two at terms = 1)."""
import numpy as np

import public_common as K
import unpack_common as U

MAX_TERMS = 8                                     # TFHE_HIP_PUBLIC_MAX_TERMS
P1 = K.P1


def mac_terms(N):
    """the most products one accumulator takes: terms f P / 2^32 < 3.5, f the forward bound for inputs below P (float)"""
    f = K.forward_bound(10 if N == 1024 else 11, float(P1))
    k = 0
    while (k + 1) * f * P1 / 2.0 ** 32 < 3.5:
        k += 1
    return k


def wrap32(x):
    """int64 -> the int32 with the same low 32 bits"""
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def negacyclic_int64(q, c):
    """q c in Z[X]/(X^N + 1) for q [N] (|q| <= 2^11) and c [..., N] of 0 <= c < 2^32, exact in int64 (below 2^54)"""
    q = np.asarray(q, dtype=np.int64)
    N = len(q)
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    mat = np.where(i >= j, q[(i - j) % N], -q[(i - j) % N])     # coefficient i takes q[i - j] c[j], negated past the wrap
    return (mat @ np.asarray(c, dtype=np.int64).T).T


def sum_product(polys, ring):
    """sum_t polys[t] * ring[t] for polys [terms][N] and ring samples [terms][2][N] int32 (words signed) -> int32 [2][N]"""
    polys, ring = np.asarray(polys), np.asarray(ring)
    assert len(polys) == len(ring) <= MAX_TERMS
    acc = np.zeros(ring.shape[1:], dtype=np.int64)
    for q, c in zip(polys, ring):
        acc += negacyclic_int64(q, c.astype(np.int64) % 2 ** 32)
    return wrap32(acc)


def sum_products(polys, ring, terms, first=0, ngroups=None):
    """tfhe_hip_ring_mul_public_sum: out[g] = sum_t polys[first + g terms + t] * ring[t] -> int32 [ngroups][2][N]"""
    polys = np.asarray(polys)
    ngroups = (len(polys) - first) // terms if ngroups is None else ngroups
    return np.stack([sum_product(polys[first + g * terms:first + (g + 1) * terms], ring) for g in range(ngroups)])


def sum_rows(polys, probe, terms, M, w):
    """row i = Extract_((i mod S) w)(sum_t polys[(i / S) terms + t] * probe[t]) for i < M -> int32 [M][N + 1]"""
    N = np.asarray(probe).shape[-1]
    per = N // w
    prods = sum_products(polys, probe, terms, 0, -(-M // per))
    return U.extract_ref(prods, [(i // per) * N + (i % per) * w for i in range(M)], N)


def worst_group(N, terms):
    """every coefficient -T / terms: the per-term maxima sum to T exactly, and against words 0x80000000 coefficient N - 1
    of the sum reaches N T 2^31 -> (polys int64 [terms][N], ring int32 [terms][2][N], the unreduced coefficients)"""
    T = K.max_coef(N)
    assert T % terms == 0
    polys = np.full((terms, N), -(T // terms), dtype=np.int64)
    ring = np.full((terms, 2, N), K.I32_MIN, dtype=np.int32)
    coef = [terms * (-(T // terms)) * K.I32_MIN * ((m + 1) - (N - 1 - m)) for m in range(N)]
    return polys, ring, coef


def masked_counts(b, g, m, n):
    """(valid, disagree) over the bits both masks keep, plain integers"""
    b, g, m, n = (np.asarray(x, dtype=np.int64) & 1 for x in (b, g, m, n))
    return int((m & n).sum()), int(((b ^ g) & m & n).sum())
