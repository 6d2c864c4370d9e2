"""Shared by tests/test_inner_sum_cpu.py and tests/test_gpu_inner_sum.py: sums of TGSW products over several ring samples
restated in numpy from the integers of include/tfhe_hip.h ("TGSW products over several ring samples") -- the summed product
built on select_common.extern_product_exact (the unreduced integer sums, added over the terms and reduced mod 2^32 once), the
rows through inner_common.extract, the two bounds restated from their derivation and the variance the header states.
Shares no code with the library.

Exactness: one term's unreduced coefficient stays below (k+1) l N (Bg/2) 2^31, K terms below the CRT bound's 2^52.5, so the
int64 sums never wrap."""
import numpy as np

import inner_common as I
import select_common as S
from pack_common import P0, P1, forward_bound

MAX_TERMS = 8                                    # TFHE_HIP_INNER_MAX_TERMS
NTT_R = (2 ** 32 % P0, 2 ** 32 % P1)             # ntt_field.hpp


def sum_product_exact(G, c, l, Bgbit):
    """G [K][(k+1) l][2][N] int32, c [K][2][N] int32 -> the unreduced integer sum [2][N] int64"""
    G, c = np.asarray(G), np.asarray(c)
    assert len(G) == len(c)
    out = np.zeros(c.shape[1:], dtype=np.int64)
    for t in range(len(c)):
        s, _ = S.extern_product_exact(G[t], c[t], l, Bgbit)
        out += s
    return out


def sum_product(G, c, l, Bgbit):
    """sum_t G_t (.) c_t -> int32 [2][N]"""
    return S.to_i32(sum_product_exact(G, c, l, Bgbit))


def sum_products(sel, first, terms, ring, l, Bgbit):
    """out[g] = sum_t G_(first + t) (.) ring[g terms + t]: sel [d][(k+1) l][2][N], ring [groups terms][2][N] -> int32 [groups][2][N]"""
    sel, ring = np.asarray(sel), np.asarray(ring)
    assert len(ring) % terms == 0 and first + terms <= len(sel)
    return np.stack([sum_product(sel[first:first + terms], ring[g * terms:(g + 1) * terms], l, Bgbit) for g in range(len(ring) // terms)])


def sum_rows(sel, first, terms, ring, M, w, l, Bgbit):
    """row i = Extract_((i mod S) w)(the sum of group i / S) for i < M -> int32 [M][N + 1]"""
    return I.inner_rows(sum_products(sel, first, terms, ring, l, Bgbit), M, w)


# ---- the two bounds of peba1_amd/csrc/ring_inner_sum.hpp, from their derivation ----
def fold_bound():
    """what a fold leaves in the accumulator, in units of P^2: |y| < 4 P times R = 2^32 mod P, the larger R over the smaller P"""
    return 4.0 * max(NTT_R) / min(P0, P1)


def block_ok(N, rows):
    """`rows` products of a transform output of signed digits up to 2^11 with an image word below P on top of a folded
    accumulator, one Montgomery reduction (|T| / 2^32 + P / 2), and the inverse transform takes inputs below 4 P"""
    logn = {1024: 10, 2048: 11}[N]
    return (rows * forward_bound(logn, 2.0 ** 11) + fold_bound()) * P1 * P1 / 2.0 ** 32 + P1 / 2.0 < 4.0 * P1


def block_rows(N):
    B = 0
    while block_ok(N, B + 1):
        B += 1
    return B


def mac_ok(N, l, terms):
    """the block the kernel folds after, or the whole sum where it is shorter (no fold under it then: select_common.mac_ok's
    inequality at that many rows)"""
    rows, B = terms * 2 * l, block_rows(N)
    if rows > B:
        return B >= 1 and block_ok(N, B)
    logn = {1024: 10, 2048: 11}[N]
    return rows * forward_bound(logn, 2.0 ** 11) * P1 * P1 / 2.0 ** 32 + P1 / 2.0 < 4.0 * P1


def crt_ok(N, l, Bgbit, terms):
    """terms (k+1) l N (Bg/2) 2^31 below the exact range of the signed CRT, in Python integers"""
    return terms * 2 * l * N * 2 ** (Bgbit - 1) * 2 ** 31 < S.CRT_EXACT_LIMIT


def max_terms(N, l, Bgbit):
    K = 0
    while K < MAX_TERMS and mac_ok(N, l, K + 1) and crt_ok(N, l, Bgbit, K + 1):
        K += 1
    return K


def variance(N, l, Bgbit, bk_stdev, norm2s, ring_variance, k=1):
    """the header's variance before the key switch: tfhe_hip_ring_inner's three terms, summed over the terms' probe norms"""
    return sum(I.inner_variance(N, l, Bgbit, bk_stdev, n2, ring_variance, k) for n2 in norm2s)


def rounding_weight(values, N, key=None):
    """|p|^2 + |p S|^2 for p = sum_i v_i X^(-i), from the definition: under the ring key `key` (N bits), or -- key None -- its
    expectation over a uniform binary key, E (p S)[j]^2 = (|v|^2 + sigma_j^2) / 4 with sigma_j the signed sum of the v_i
    split at the wrap"""
    v = [int(x) for x in np.asarray(values).reshape(-1)]
    n2 = sum(x * x for x in v)
    if key is not None:
        pS = S.negacyclic(I.probe_poly(v, N), np.asarray(key, dtype=np.int64)[:N])
        return n2 + int((pS.astype(np.int64) ** 2).sum())
    total = 0.0
    for j in range(N):
        sigma = sum(x if j + i < N else -x for i, x in enumerate(v))
        total += (n2 + sigma * sigma) / 4.0
    return n2 + total


def variance_weighted(N, l, Bgbit, bk_stdev, norm2s, weights, ring_variance, k=1):
    """variance() with the rounding term from rounding weights: sum_t [(k+1) l N (Bg/2)^2 bk^2 + W_t eps^2 / 3 + |p_t|^2 v]"""
    eps = 2.0 ** -(l * Bgbit + 1)
    return sum((k + 1) * l * N * (2.0 ** (Bgbit - 1)) ** 2 * bk_stdev ** 2 + w * eps ** 2 / 3.0 + n2 * ring_variance
               for n2, w in zip(norm2s, weights))


# ---- worst-case operands ----
def worst_case(N, l, Bgbit, terms):
    """ring words whose digits are all -Bg/2 against selector words 0x80000000 everywhere: (sel [terms][2 l][2][N], ring
    [terms][2][N], the unreduced coefficients in Python integers).  Coefficient m of a product of two constant polynomials
    a, b is a b ((m + 1) - (N - 1 - m)); there are terms (k+1) l of them."""
    word = S.extreme_difference(l, Bgbit, "min")
    ring = np.full((terms, 2, N), word, dtype=np.int64)
    sel = np.full((terms, 2 * l, 2, N), S.I32_MIN, dtype=np.int64)
    digit = -2 ** (Bgbit - 1)
    coef = [terms * 2 * l * digit * S.I32_MIN * ((m + 1) - (N - 1 - m)) for m in range(N)]
    return S.to_i32(sel), S.to_i32(ring), coef


# ---- the masked identity in plain integers ----
def masked_counts(b, g, m, n):
    b, g, m, n = (np.asarray(x, dtype=np.int64).reshape(-1) & 1 for x in (b, g, m, n))
    both = m & n
    return int(both.sum()), int((both & (b ^ g)).sum())
