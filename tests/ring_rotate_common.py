"""Shared by tests/test_ring_rotate_cpu.py and tests/test_gpu_ring_rotate.py: the ring LUT bootstrap restated in numpy from
the integers of include/tfhe_hip.h ("ring LUT bootstrap") -- the monomial multiple X^(-r) c for every r in [0, 2N), the modulus
switch, ACC_0 = X^(-bbar) c and the n steps ACC <- CMUX(BK_i, X^(abar_i) ACC, ACC), a step with abar_i = 0 skipped as the
kernel skips it.  Nothing here is a second definition: the rotation is tests/lookup_common.py's rotate_ref (negated from N
on), the CMUX is tests/select_common.py's, the modulus switch is tests/lut_common.py's, which tests/test_lut_cpu.py holds
against the oracle's orc_modswitch, the extraction is tests/unpack_common.py's.  Shares no code with the library."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from lookup_common import rotate_ref
from lut_common import modswitch
from pack_common import to_i32
from select_common import cmux
from unpack_common import extract_ref


def rotate_any(c, r):
    """X^(-r) c for a ring sample c [2][N] (or one polynomial [N]) and ANY r in [0, 2N): coefficient j is c[(j + r) mod 2N]
    where that index is below N and -c[index - N] from N on -- rotate_ref below N, its negation (X^N = -1) from N on"""
    c = np.asarray(c)
    N = c.shape[-1]
    assert 0 <= r < 2 * N
    out = rotate_ref(c, r % N)
    return to_i32(-out.astype(np.int64)) if r >= N else out


def switched(lwe, N):
    """(abar_0 .. abar_(n-1), bbar) of an LWE sample's n + 1 words"""
    return [modswitch(int(x), N) for x in np.asarray(lwe).reshape(-1)]


def blind_rotate_ref(bk_rows, c, lwe, l, Bgbit):
    """ACC_n of the header: bk_rows [n][(k+1) l][2][N] (the cloud key's raw bootstrapping rows), c [2][N], lwe [n + 1] ->
    int32 [2][N]"""
    bk_rows, c = np.asarray(bk_rows), np.asarray(c)
    N, n = c.shape[-1], len(bk_rows)
    bar = switched(lwe, N)
    assert len(bar) == n + 1
    acc = rotate_any(c, bar[n])
    for i in range(n):
        if bar[i]:                                     # skipped, as in the kernel (computed it leaves the same words)
            acc = cmux(bk_rows[i], rotate_any(acc, 2 * N - bar[i]), acc, l, Bgbit)
    return acc


def blind_rotate_many(bk_rows, tables, ring_index, lwes, l, Bgbit, workers=16):
    """blind_rotate_ref of tables[ring_index[j]] (None: j) by lwes[j] for every j, dealt to a few threads -> [count][2][N]"""
    idx = range(len(lwes)) if ring_index is None else ring_index
    with ThreadPoolExecutor(workers) as ex:
        return np.stack(list(ex.map(lambda jc: blind_rotate_ref(bk_rows, tables[jc[1]], lwes[jc[0]], l, Bgbit), enumerate(idx))))


def extract0(acc):
    """Extract_0 of accumulators [count][2][N] -> int32 [count][N + 1]"""
    acc = np.asarray(acc)
    N = acc.shape[-1]
    acc = acc.reshape(-1, 2, N)
    return extract_ref(acc, np.arange(len(acc)) * N, N)


def bk_rows_of(bk_words, n, l, N):
    """the key's words as [n][(k+1) l][2][N]"""
    return np.asarray(bk_words).reshape(n, 2 * l, 2, N)


def lwe_with_bars(rng, n, N, bars):
    """random LWE words [n + 1] whose first len(bars) modulus-switched words are forced to `bars` (word = bar 2^32 / 2N)"""
    w = rng.integers(-2 ** 31, 2 ** 31, n + 1, dtype=np.int64)
    shift = 32 - int(N).bit_length()
    for i, b in enumerate(bars):
        w[i] = int(b) << shift
    return to_i32(w)
