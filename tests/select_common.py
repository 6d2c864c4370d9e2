"""Shared by tests/test_select_cpu.py and tests/test_gpu_select.py: the private selection restated in numpy from the integers
of include/tfhe_hip.h -- the offset decomposition (a mirror of the oracle's orc_decompose), the external product of a TGSW
sample with a ring sample, the CMUX and the tree -- the two magnitude bounds of the CMUX kernel restated from their
derivation, and the variance the header states.  Shares no code with the library.

Everything is exact: a negacyclic product is an int64 convolution of digits (at most 2^11 in magnitude) with row words
taken as signed 32-bit integers, folded modulo X^N + 1; one coefficient of the sum over the (k+1) l rows stays below
(k+1) l N (Bg/2) 2^31, which the CRT bound holds under 2^52.5, so int64 never wraps; the sum is then reduced mod 2^32."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from pack_common import P0, P1, STDEVS, custom_tuple, forward_bound, ring_phases, to_i32   # noqa: F401

CRT_EXACT_LIMIT = P0 * P1 // 100 * 36            # ntt_field.hpp
SETS = {"P128": (1024, 3, 7), "P80": (1024, 2, 10), "P2048": (2048, 3, 6)}       # name -> (N, l, Bgbit)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def decomp_offset(l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (32 - j * Bgbit) for j in range(1, l + 1)) & 0xFFFFFFFF


def decompose(poly, l, Bgbit):
    """orc_decompose: ((x + offset) >> (32 - (p+1) Bgbit) & (Bg - 1)) - Bg/2 for p < l -> int64 [l][N]"""
    v = (np.asarray(poly).astype(np.int64) % 2 ** 32 + decomp_offset(l, Bgbit)) % 2 ** 32
    return np.stack([((v >> (32 - (p + 1) * Bgbit)) & (2 ** Bgbit - 1)) - 2 ** (Bgbit - 1) for p in range(l)])


def negacyclic(d, w):
    """d(X) w(X) in Z[X]/(X^N + 1), exact in int64"""
    N = len(d)
    c = np.convolve(np.asarray(d, dtype=np.int64), np.asarray(w).astype(np.int64))
    out = c[:N].copy()
    out[:N - 1] -= c[N:]
    return out


def extern_product_exact(G, c, l, Bgbit):
    """G [(k+1) l][2][N] int32, c [2][N] int32 -> (the unreduced integer sums [2][N] int64, the digits [2 l][N])"""
    G, c = np.asarray(G), np.asarray(c)
    dig = np.concatenate([decompose(c[u], l, Bgbit) for u in range(2)])
    out = np.zeros(c.shape, dtype=np.int64)
    for r in range(2 * l):
        if dig[r].any():
            for w in range(2):
                out[w] += negacyclic(dig[r], G[r, w])
    return out, dig


def cmux(G, d1, d0, l, Bgbit):
    """CMUX(G, d1, d0) = d0 + G (.) (d1 - d0) -> int32 [2][N]"""
    d1, d0 = np.asarray(d1).astype(np.int64), np.asarray(d0).astype(np.int64)
    s, _ = extern_product_exact(G, to_i32(d1 - d0), l, Bgbit)
    return to_i32(d0 + s)


def cmux_many(G, d1, d0, l, Bgbit, workers=16):
    """cmux of every pair d1[c], d0[c] ([count][2][N]) under one G, the pairs dealt to a few threads"""
    with ThreadPoolExecutor(workers) as ex:
        return np.stack(list(ex.map(lambda c: cmux(G, d1[c], d0[c], l, Bgbit), range(len(d1)))))


def tree(selector_words, gallery, l, Bgbit):
    """The tree of the header: selector_words [d][2 l][2][N], gallery [M][2][N], 1 <= M <= 2^d -> int32 [2][N]"""
    sel = np.asarray(selector_words)
    e = [np.asarray(g) for g in np.asarray(gallery)]
    d = len(sel)
    assert 1 <= len(e) <= 2 ** d
    zero = np.zeros_like(e[0])
    for j in range(d):
        e = [cmux(sel[j], e[2 * i + 1] if 2 * i + 1 < len(e) else zero, e[2 * i], l, Bgbit) for i in range((len(e) + 1) // 2)]
    assert len(e) == 1
    return e[0].copy()


# ---- the two bounds of peba1_amd/csrc/cmux.hpp, from their derivation ----
def mac_ok(N, l):
    """(k+1) l products of a transform output of signed digits up to 2^11 with an image word below P, one Montgomery reduction
    (|T| / 2^32 + P / 2), and the inverse transform takes inputs below 4 P"""
    logn = {1024: 10, 2048: 11}[N]
    return 2 * l * forward_bound(logn, 2.0 ** 11) * P1 * P1 / 2.0 ** 32 + P1 / 2.0 < 4.0 * P1


def crt_ok(N, l, Bgbit):
    """(k+1) l N (Bg/2) 2^31 below the exact range of the signed CRT"""
    return 2 * l * N * 2 ** (Bgbit - 1) * 2 ** 31 < CRT_EXACT_LIMIT


def grid(N):
    return [(N, l, B) for B in range(1, 13) for l in range(1, 32 // B + 1)]


def cloud_key_accepted(ok, g):
    """what unsupported_reason (engine.cpp) takes: the CRT range and one admissible blind-rotate form;
    ok = tfhe_hip_test_form_admissible"""
    N, l, B = g
    return crt_ok(N, l, B) and any(ok(f, N, l, B, t) == 1 for f in range(4) for t in range(3))


def cmux_variance(N, l, Bgbit, bk_stdev, k=1):
    """the first-order bound the header states for one CMUX (torus units): key term + rounding term"""
    eps = 2.0 ** -(l * Bgbit + 1)
    return (k + 1) * l * N * (2.0 ** (Bgbit - 1)) ** 2 * bk_stdev ** 2 + (1 + k * N) * eps ** 2 / 3.0


# ---- worst-case operands ----
def extreme_difference(l, Bgbit, which):
    """the word whose l digits are all -Bg/2 ("min") or all Bg/2 - 1 ("max"), bits below the lowest digit field zero"""
    fields = 0 if which == "min" else sum((2 ** Bgbit - 1) << (32 - (p + 1) * Bgbit) for p in range(l))
    return (fields - decomp_offset(l, Bgbit)) % 2 ** 32


def extreme_closed_form(N, l, word, digit, d0):
    """CMUX of rows that hold `word` everywhere against digits that are `digit` everywhere, in Python integers: coefficient
    j of a product of two constant polynomials is digit word ((j + 1) - (N - 1 - j)), and there are (k+1) l rows.
    -> (int32 [2][N], the largest magnitude of an unreduced sum)"""
    sums = [2 * l * digit * word * (2 * j + 2 - N) for j in range(N)]
    out = np.array([[(int(d0[w][j]) + sums[j]) % 2 ** 32 for j in range(N)] for w in range(2)], dtype=np.int64)
    return to_i32(out), max(abs(s) for s in sums)


def random_ring(rng, count, N):
    return rng.integers(I32_MIN, I32_MAX + 1, size=(count, 2, N), dtype=np.int64).astype(np.int32)
