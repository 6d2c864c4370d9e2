"""Shared by tests/test_lut_multi_cpu.py, tests/test_gpu_lut_multi.py and tests/golden/make_lut_multi_digests.py: the
multi-output LUT bootstrap (tfhe_hip_lut_bootstrap_multi) restated in numpy from its integers (include/tfhe_hip.h) --
the extract at index e, the weighted combination of taps, the construction from tables -- and the fixed cases of
tests/golden/lut_multi_digests.json.  Written from the definitions; it shares no code with the library.  Expected words
are (oracle key switch)(numpy outputs(oracle accumulator)), the accumulator from lut_common.oracle_lut_bootstrap."""
import json
import os

import numpy as np

import lut_common as T

DIGESTS = os.path.join(T.ROOT, "tests", "golden", "lut_multi_digests.json")
KEY_SEED = T.KEY_SEED
CASES = {"P128": 8, "P80": 6, "P2048": 4}
RING = {"P128": 1024, "P80": 1024, "P2048": 2048}
OP_LUTM = 65
SPEC_WORDS = 73


def load_digests():
    with open(DIGESTS) as f:
        return json.load(f)


# ---- the definitions ------------------------------------------------------------------------------------------------
def extract_at(acc, e):
    """Extract_e(ACC), ACC = (A, B): b = B[e]; a_i = A[e - i] for i <= e, -A[N + e - i] for i > e.  N + 1 words."""
    acc = np.asarray(acc, dtype=np.int64)
    N = len(acc) // 2
    A, B = acc[:N], acc[N:]
    d = e - np.arange(N)
    a = np.where(d >= 0, A[d % N], -A[d % N])
    return T.wrap32(np.concatenate([a, [B[e]]]))


def output(acc, taps, c0):
    """(0, c0) + sum weight * Extract_index(ACC), wrapping mod 2^32 on all N + 1 words."""
    N = len(acc) // 2
    u = np.zeros(N + 1, dtype=np.int64)
    for e, w in taps:
        u += int(w) * extract_at(acc, e).astype(np.int64)
    u[N] += int(c0)
    return T.wrap32(u)


def outputs(acc, spec):
    """Every output of a spec [(taps, c0), ...]."""
    return [output(acc, taps, c0) for taps, c0 in spec]


def negacyclic_read(v, p):
    """The negacyclic table v at p (mod 2N): v[p] below N, -v[p - N] from N on."""
    N = len(v)
    p %= 2 * N
    return int(v[p]) if p < N else -int(v[p - N])


def noiseless_phase(v, p, taps, c0):
    """What output (taps, c0) decrypts to without noise for an input phase p (in 1/2N-ths): coefficient e of X^-p v is the
    table read at p + e.  Mod 2^32, as a signed word."""
    return int(T.wrap32(int(c0) + sum(int(w) * negacyclic_read(v, p + e) for e, w in taps)))


def spec_from_tables(N, step, levels):
    """The construction of tfhe_hip_new_lut_multi_from_tables from its definition: (words of the polynomial, spec)."""
    levels = np.asarray(levels, dtype=np.int64)
    slots = levels.shape[1]
    assert step % 2 == 0 and N % slots == 0
    spec = []
    for L in levels:
        taps = [(j * (N // slots), int(L[slots - 1 - j] - L[slots - j])) for j in range(1, slots)]
        spec.append(([t for t in taps if t[1] != 0], int(T.wrap32((step // 2) * int(L[0] + L[slots - 1])))))
    return np.full(N, step // 2, dtype=np.int32), spec


def check_limits(N, spec):
    assert 1 <= len(spec) <= 4
    for taps, _ in spec:
        assert 1 <= len(taps) <= 8 and len({e for e, _ in taps}) == len(taps)
        assert all(0 <= e < N and w != 0 and abs(w) <= 8 for e, w in taps)


# ---- the fixed cases ----------------------------------------------------------------------------------------------------
IDENTITY = [([(0, 1)], 0)]


def spec_templates(N, seed):
    """Six specs: the one-tap identity; two outputs with the extreme weights; four outputs of which the second is not
    wanted; one output of eight taps; four outputs all wanted; two outputs sharing an index."""
    r = [int(x) for x in np.random.default_rng(seed).choice(np.arange(2, N - 1), 8, replace=False) if x != N // 2][:6]
    return [
        (IDENTITY, [True]),
        ([([(1, 1)], 0), ([(N // 2, -8), (N - 1, 8)], 0x01234567)], [True, True]),
        ([([(0, 1)], 0), ([(N // 2, 2)], 12345), ([(r[0], -3), (1, 1)], -(1 << 30) + 7), ([(N - 1, -1)], 0)],
         [True, False, True, True]),
        ([([(0, 8), (1, -8), (N // 2, 1), (N - 1, -1), (r[1], 2), (r[2], -3), (r[3], 5), (r[4], -7)], -0x0BADCAFE)], [True]),
        ([([(r[0], 1), (r[1], -1)], 1 << 29), ([(N - 1, 3)], 0), ([(0, -2), (N // 2, 2)], -(1 << 29)), ([(r[5], 1)], 99)],
         [True, True, True, True]),
        ([([(N // 2, 1), (0, 1)], 0), ([(N // 2, -1), (1, 4)], 1 << 28)], [True, True]),
    ]


def case_specs(pname):
    N = RING[pname]
    base = {"P128": 1100, "P80": 1200, "P2048": 1300}[pname]
    tpl = spec_templates(N, base)
    order = {"P128": [0, 1, 2, 3, 4, 5, 1, 2], "P80": [0, 1, 2, 3, 4, 5], "P2048": [0, 2, 3, 1]}[pname]
    cases = []
    for i, which in enumerate(order):
        spec, wanted = tpl[which]
        check_limits(N, spec)
        coefs = T.COEFS[(i + 5) % len(T.COEFS)]
        rng = np.random.default_rng(8000 + base + i)
        kind = ("random", "sectors", "constant")[i % 3]
        gen = {"kind": kind, "seed": base + i}
        if kind == "sectors":
            gen["slots"] = (4, 16)[(i // 3) % 2]
        if kind == "constant":
            gen = {"kind": kind, "mu": T.MUS[(i // 3) % len(T.MUS)]}
        cases.append({"index": i, "parameter_set": pname, "coefs": coefs, "lut": gen, "enc_seed": 6000 + base + i,
                      "bits": rng.integers(0, 2, len(coefs)).tolist(), "c0": int(rng.integers(-2 ** 31, 2 ** 31)),
                      "template": which, "spec": [[[list(t) for t in taps], int(c0)] for taps, c0 in spec],
                      "wanted": list(wanted)})
    return cases


def spec_of(case):
    """The case's spec as [(taps, c0)] with tuple taps."""
    return [([tuple(t) for t in taps], c0) for taps, c0 in case["spec"]]


def case_lin(O, oks, case):
    return T.linear(case["coefs"], T.case_inputs(O, oks, case), case["c0"])


def oracle_case(O, oks, case):
    """(key-switched samples (None where not wanted), extracted samples of every output, raw accumulator)."""
    _, _, acc = T.oracle_lut_bootstrap(O, oks, case_lin(O, oks, case), T.lut_words(case["lut"], oks.N))
    us = outputs(acc, spec_of(case))
    cts = [oks.keyswitch(u) if w else None for u, w in zip(us, case["wanted"])]
    return cts, us, acc


def pack_spec(spec):
    """One record of the raw entry / the device table: {nout, ntaps[4], out_c0[4], index[4][8], weight[4][8]}."""
    rec = np.zeros(SPEC_WORDS, dtype=np.int32)
    rec[0] = len(spec)
    for m, (taps, c0) in enumerate(spec):
        rec[1 + m] = len(taps)
        rec[5 + m] = T.wrap32(c0)
        for t, (e, w) in enumerate(taps):
            rec[9 + 8 * m + t] = e
            rec[41 + 8 * m + t] = w
    return rec
