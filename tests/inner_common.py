"""Shared by tests/test_inner_cpu.py and tests/test_gpu_inner.py: the encrypted inner products restated in numpy from the
integers of include/tfhe_hip.h ("encrypted inner products") -- the probe polynomial, the product G (.) c (select_common's
exact external product with nothing added), the sample extraction at the entries' first coefficients and the variance the
header states.  Shares no code with the library."""
import numpy as np

import select_common as S


def probe_poly(s, N):
    """sum_i s_i X^(-i): p[0] = s_0, p[N - i] = -s_i for 1 <= i < w, 0 elsewhere -> int64 [N]"""
    s = [int(x) for x in s]
    p = [0] * N
    p[0] = s[0]
    for i in range(1, len(s)):
        p[N - i] = -s[i]
    return np.array(p, dtype=np.int64)


def negacyclic_python(p, t):
    """p t in Z[X]/(X^N + 1) in Python integers, term by term from the definition (p sparse)"""
    N = len(t)
    out = [0] * N
    for m in range(N):
        if int(p[m]):
            for j in range(N):
                if j + m < N:
                    out[j + m] += int(p[m]) * int(t[j])
                else:
                    out[j + m - N] -= int(p[m]) * int(t[j])
    return out


def product(G, c, l, Bgbit):
    """G (.) c: G [(k+1) l][2][N] int32, c [2][N] int32 -> int32 [2][N]"""
    s, _ = S.extern_product_exact(G, c, l, Bgbit)
    return S.to_i32(s)


def extract(c, e):
    """Extract_e of a ring sample c [2][N]: a_i = A[e - i] for i <= e, -A[N + e - i] past it, b = B[e] -> int32 [N + 1]"""
    A, B = np.asarray(c[0]).astype(np.int64), np.asarray(c[1]).astype(np.int64)
    N = len(A)
    i = np.arange(N)
    a = np.where(i <= e, A[(e - i) % N], -A[(N + e - i) % N])
    return S.to_i32(np.concatenate([a, [B[e]]]))


def inner_rows(products, M, w):
    """row i = Extract_((i mod S) w)(products[i / S]) for i < M -> int32 [M][N + 1]"""
    N = products.shape[-1]
    per = N // w
    return np.stack([extract(products[i // per], (i % per) * w) for i in range(M)])


def row_phases(rows, tlwe_key):
    """b - <a, key> of extracted rows [M][N + 1] under the extracted ring key (the ring key's coefficients), int32"""
    r = np.asarray(rows).astype(np.int64) % 2 ** 32
    key = np.asarray(tlwe_key).astype(np.int64)[:r.shape[1] - 1]
    return S.to_i32(r[:, -1] - (r[:, :-1] * key).sum(axis=1))


def inner_variance(N, l, Bgbit, bk_stdev, norm2, ring_variance, k=1):
    """the header's variance of a coefficient of G (.) c before the key switch, for a probe of squared norm norm2"""
    eps = 2.0 ** -(l * Bgbit + 1)
    return (k + 1) * l * N * (2.0 ** (Bgbit - 1)) ** 2 * bk_stdev ** 2 + (1 + k * N) * norm2 * eps ** 2 / 3.0 + norm2 * ring_variance


def truncation_bias(p, tlwe_key, l, Bgbit):
    """The header's bias of G (.) c on words that were NOT centred, in torus32 units: the decomposition drops the low
    32 - l Bgbit bits of every word, a mean of eps = 2^(31 - l Bgbit) on both polynomials, whose phase is eps (1 - ones * S);
    the product multiplies it by -p -> int64 [N]"""
    N = len(p)
    eps = 1 << (31 - l * Bgbit)
    phase_e = eps * (1 - S.negacyclic(np.ones(N, dtype=np.int64), np.asarray(tlwe_key)[:N]))
    return -S.negacyclic(np.asarray(p, dtype=np.int64), phase_e)
