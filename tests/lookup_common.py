"""Shared by tests/test_lookup_cpu.py and tests/test_gpu_lookup.py: the packed lookup restated in numpy from the integers of
include/tfhe_hip.h ("private lookup in packed galleries") -- the monomial multiple X^(-r) c, the rotation step
ROT(G, r, c) = CMUX(G, X^(-r) c, c) and the lookup: the select's tree over the samples under the high bits, then one
rotation step per low bit.  The CMUX and the tree are those of tests/select_common.py; nothing here shares code with the
library."""
import numpy as np

from select_common import cmux, tree


def rotate_ref(c, r):
    """X^(-r) c for a ring sample c [2][N] (or one polynomial [N]), 0 <= r < N: coefficient j is c[j + r] for j + r < N and
    -c[j + r - N] otherwise, wrapping mod 2^32 -> int32, the shape of c"""
    c = np.asarray(c)
    N = c.shape[-1]
    assert 0 <= r < N
    v = c.astype(np.int64)
    out = np.concatenate([v[..., r:], -v[..., :r]], axis=-1)
    return ((out + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


def rot_step(G, r, c, l, Bgbit):
    """ROT(G, r, c) = CMUX(G, X^(-r) c, c) -> int32 [2][N]"""
    return cmux(G, rotate_ref(c, r), c, l, Bgbit)


def log2_exact(x):
    assert x >= 1 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def lookup_ref(selector_words, gallery, M, width, l, Bgbit):
    """The lookup of the header: selector_words [d][2 l][2][N], gallery [R][2][N] holding M entries of `width` coefficients,
    S = N / width per sample -> int32 [2][N] whose coefficients 0 .. width - 1 carry entry sum_t bit_t 2^t"""
    sel, g = np.asarray(selector_words), np.asarray(gallery)
    N, d = g.shape[-1], len(sel)
    S = N // width
    s = log2_exact(S)
    assert width * S == N and d >= s and 1 <= M <= 2 ** d
    R = -(-M // S)
    assert g.shape == (R, 2, N), (g.shape, R)
    c = tree(sel[s:], g, l, Bgbit)                       # level j under G_(s+j)
    for t in range(s):
        c = rot_step(sel[t], width << t, c, l, Bgbit)
    return c


def sample_with_rotated_difference(N, r, E):
    """One polynomial d0 (Python integers -> int64 [N], words mod 2^32) with (X^(-r) d0 - d0)[j] = E mod 2^32 for EVERY j, 0 < r < N.
    Along the orbit j -> j + r mod N the definition gives d0[j + r] = d0[j] + E without a wrap and d0[j + r - N] =
    -(d0[j] + E) with one; an orbit has N / gcd(r, N) members and wraps r / gcd(r, N) times, an odd number, so it closes on
    a = -a + C, where C sums an even number of +-E: C is even and a = C / 2 solves it."""
    g = np.gcd(r, N)
    d0 = [None] * N
    for start in range(g):
        # value at the orbit's members as sign * a + const, a the unknown at `start`
        j, sign, const, members = start, 1, 0, []
        for _ in range(N // g):
            members.append((j, sign, const))
            const += E
            j += r
            if j >= N:
                j, sign, const = j - N, -sign, -const
        assert j == start and sign == -1 and const % 2 == 0
        a = (const // 2) % 2 ** 32
        for j, sg, cn in members:
            d0[j] = (sg * a + cn) % 2 ** 32
    return np.array(d0, dtype=np.int64)
