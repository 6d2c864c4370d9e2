"""The serial path of a blind-rotate step.  In the 4-wave form the last radix-4 step of the inverse transform makes the
half of its outputs the CRT partner recombines final first and stores it before the wave's own half; and the step loop's
head -- which steps run (abar_i != 0), which are skipped, where the vector ends (bar[n] holds bbar) -- is what a read of
abar ahead of its step would change (tried and taken out, profiles/step_path_ab.txt; the patterns stay as its guard).
Neither may change a word, so every accumulator word and every extracted word is compared with the oracle, for patterns
of zero and non-zero abar made by choosing the input sample's mask words (a_i = 0 gives abar_i = 0), in every kernel form;
each launch proves by the per-form launch counters (TfheHipStats) which kernel and digit-table mode it ran."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adversarial_common as A

pytestmark = pytest.mark.gpu

TUNING_DEFAULTS = {"br_variant": -1, "br_digit_table": 1, "br8_max_rotations": 1 << 30, "br_tail8": 1}
PATTERNS = ["first_zero", "last_zero", "penultimate_zero", "run_of_5", "alternating", "all_zero", "only_first", "only_last",
            "random"]
# N = 2048 (the oracle takes 1.3 s per full rotation there): two full-length rows that hold the same shapes -- both ends and
# a run of five skipped in one, every other step in the other (abar_0 = abar_{n-2} = 0, abar_{n-1} != 0) -- and the rows of
# at most one step
PATTERNS_2048 = ["ends_and_run", "alternating", "all_zero", "only_first", "only_last"]


def restore():
    from peba1_amd import api
    for k, v in TUNING_DEFAULTS.items():
        api.set_tuning(k, v)


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def counters(api):
    s = api.stats()
    return np.array([s[f] for f in A.FORM_COUNTERS + A.TABLE_COUNTERS], dtype=np.int64)


def expect_counters(forms, tables, l, Bgbit):
    want = np.zeros(7, dtype=np.int64)
    for f in forms:
        want[f] += 1
        want[4 + A.tables_run(f, l, Bgbit, tables)] += 1
    return want


def zero_positions(name, n):
    """The mask words that are 0 in a pattern (abar_i = 0 there and nowhere else)."""
    every = set(range(n))
    return {"first_zero": {0}, "last_zero": {n - 1}, "penultimate_zero": {n - 2},
            "run_of_5": set(range(n // 2, n // 2 + 5)), "ends_and_run": {0, n - 1} | set(range(n // 2, n // 2 + 5)),
            "alternating": set(range(0, n, 2)), "all_zero": every,
            "only_first": every - {0}, "only_last": every - {n - 1}, "random": set()}[name]


def pattern_rows(pp, oks, seed, names):
    """One input sample per pattern: uniformly random words, the pattern's mask words set to 0, and any other mask word
    whose modulus switch happens to be 0 (probability 1 / 2N each) replaced by the word that switches to 1."""
    n, N = pp.n, pp.N
    unit = np.int32(1 << (32 - N.bit_length()))          # switches to abar = 1
    rng = np.random.default_rng(seed)
    lin = rng.integers(-2**31, 2**31, (len(names), pp.words), dtype=np.int64).astype(np.int32)
    for row, name in zip(lin, names):
        zeros = sorted(zero_positions(name, n))
        row[zeros] = 0
        bar = oks.modswitch_ct(row)
        stray = [i for i in np.flatnonzero(np.asarray(bar[:n]) == 0) if i not in set(zeros)]
        row[stray] = unit
        bar = np.asarray(oks.modswitch_ct(row))
        assert set(np.flatnonzero(bar[:n] == 0)) == set(zeros), name
    return lin


class Cases:
    pass


@pytest.fixture(scope="module")
def cases(oracle, p128_keys):
    """pname -> the pattern rows of that set, its keys and the oracle's accumulators and extracted samples, computed once."""
    from peba1_amd import api
    made, own = {}, []

    def get(pname):
        if pname not in made:
            c = Cases()
            if pname == "P128":
                c.pp, c.ks, c.oks = p128_keys
            else:
                c.pp = api.ParameterSet(p2048=True)
                c.ks = api.SecretKeySet(c.pp, 0x2048, device=True)
                own.append(c.ks)
                c.oks = oracle.KeySet(oracle.params("P2048"), 0x2048)
            c.names = PATTERNS if pname == "P128" else PATTERNS_2048
            c.lin = pattern_rows(c.pp, c.oks, 0x57E9 + c.pp.N, c.names)
            def rotate(row):
                bar = c.oks.modswitch_ct(row)
                return c.oks.blind_rotate(bar[:-1], bar[-1])
            # on the host's threads (ctypes releases the GIL; the oracle is re-entrant)
            with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as ex:
                c.acc = np.stack(list(ex.map(rotate, c.lin)))
            c.u = np.stack([c.oks.sample_extract(a) for a in c.acc])
            # no step runs: the test vector comes back (mask polynomial 0, body +-mu)
            k = c.names.index("all_zero")
            assert (c.acc[k][:c.pp.N] == 0).all() and (np.abs(c.acc[k][c.pp.N:].astype(np.int64)) == A.MU).all()
            made[pname] = c
        return made[pname]
    yield get
    for ks in own:
        ks.close()


def assert_rows(got, want, names, what, rows=None):
    rows = range(len(want)) if rows is None else rows
    for r, k in enumerate(rows):
        bad = np.flatnonzero(got[r] != want[k])
        assert bad.size == 0, "%s, pattern %s (row %d): %d words differ, first at %d" % (what, names[k], r, bad.size, bad[0])


# (parameter set, label, tunings, kernel form)
FORMS = [("P128", "4-wave, digit tables", {"br_variant": 0, "br_digit_table": 1, "br8_max_rotations": 0}, A.WIDE4),
         ("P128", "4-wave, no tables", {"br_variant": 0, "br_digit_table": 0, "br8_max_rotations": 0}, A.WIDE4),
         ("P128", "8-wave", {}, A.WAVE8),
         ("P128", "split, N = 1024", {"br_variant": 2}, A.SPLIT),
         ("P2048", "split, N = 2048", {}, A.SPLIT)]


@pytest.mark.parametrize("pname,label,tunings,form", FORMS, ids=[f[1] for f in FORMS])
def test_abar_patterns_in_every_kernel_form(cases, pname, label, tunings, form):
    """Every pattern as one launch of the form: the first step skipped (abar_0 = 0), the last skipped (abar_{n-1} = 0), the
    last taken behind a skipped one, a run of five and every other step skipped, no step at all, one step at either end,
    and the random control."""
    from peba1_amd import api, lib
    c = cases(pname)
    pp = c.pp
    ok = lib.load().tfhe_hip_test_form_admissible
    t = dict(TUNING_DEFAULTS, **tunings)
    assert len(c.names) <= cu_count()
    predicted = A.predicted_form(ok, pp.N, pp.l, pp.Bgbit, len(c.names), cu_count(), t["br_variant"], t["br_digit_table"],
                                 t["br8_max_rotations"])
    assert predicted == (form, t["br_digit_table"]), label
    try:
        for k, v in tunings.items():
            api.set_tuning(k, v)
        before = counters(api)
        u, acc = api.kernel_bootstrap_woks(c.ks, c.lin, want_acc=True)
        assert (counters(api) - before == expect_counters([form], t["br_digit_table"], pp.l, pp.Bgbit)).all(), label
    finally:
        restore()
    assert_rows(acc, c.acc, c.names, label + ", accumulator")
    assert_rows(u, c.u, c.names, label + ", extracted sample")


def test_abar_patterns_in_a_4_wave_launch_with_an_8_wave_tail(cases):
    """Two workgroups per CU on the 4-wave kernel and a remainder of three rotations on the 8-wave kernel (br_tail8).  The pattern rows are tiled over it, so every pattern runs in the full round and
    three of them in the tail; a launch with a tail has no accumulator dump, so the extracted samples are compared."""
    from peba1_amd import api, lib
    c = cases("P128")
    pp = c.pp
    ok = lib.load().tfhe_hip_test_form_admissible
    total = 2 * cu_count() + 3
    rows = np.arange(total) % len(PATTERNS)
    assert ok(A.WAVE8, pp.N, pp.l, pp.Bgbit, 1)
    try:
        before = counters(api)
        u = api.kernel_bootstrap_woks(c.ks, c.lin[rows])
        assert (counters(api) - before == expect_counters([A.WIDE4, A.WAVE8], 1, pp.l, pp.Bgbit)).all()
    finally:
        restore()
    assert_rows(u, c.u, c.names, "%d rotations, 4-wave launch + 8-wave tail" % total, rows)


@pytest.mark.parametrize("br8,form", [(0, A.WIDE4), (1 << 30, A.WAVE8)], ids=["4-wave", "8-wave"])
def test_abar_patterns_in_one_multikey_launch_of_two_keys(cases, oracle, br8, form):
    """The multi-key kernels share the step loop (their own instantiation of it): one flush of two gates under two cloud
    keys, one rotation each.  AND of (the pattern row minus the gate's constant) with a zero sample has the pattern row
    as its prelude; the output equals the oracle's key switch of the oracle's extracted sample, word for word."""
    from peba1_amd import api
    c = cases("P128")
    pp, n = c.pp, c.pp.n
    seed2 = 0x4B1
    ks2 = api.SecretKeySet(pp, seed2, device=True)
    oks2 = oracle.KeySet(oracle.params("P128"), seed2)
    picks = [PATTERNS.index("first_zero"), PATTERNS.index("penultimate_zero")]
    api.set_deferred(True)
    api.set_tuning("batch_keys", 1)
    try:
        api.set_tuning("br8_max_rotations", br8)
        want, held = [], []
        for k, ks, oks in zip(picks, (c.ks, ks2), (c.oks, oks2)):
            bar = oks.modswitch_ct(c.lin[k])
            want.append(oks.keyswitch(oks.sample_extract(oks.blind_rotate(bar[:-1], bar[-1]))))
            a = c.lin[k:k + 1].copy()
            a[:, n] = A.i32(a[:, n].astype(np.int64) + (1 << 29))           # AND adds (0, -1/8)
            held.append((api.CiphertextArray(pp, 1).set_words(a), api.CiphertextArray(pp, 1).set_words(np.zeros_like(a)),
                         api.CiphertextArray(pp, 1)))
        api.flush()
        s0, before = api.stats(), counters(api)
        for (xa, za, ra), ks in zip(held, (c.ks, ks2)):
            api.gate_batch("AND", ra, xa, za, ks)
        assert api.flush() >= 0, api.last_error()
        s1 = api.stats()
        assert s1["flushes"] == s0["flushes"] + 1 and api.last_flush_keys() == 2
        assert s1["blind_rotates"] - s0["blind_rotates"] == 2
        assert (counters(api) - before == expect_counters([form], 1, pp.l, pp.Bgbit)).all()
        for (xa, za, ra), w, k in zip(held, want, picks):
            got = ra.words()[0]
            bad = np.flatnonzero(got != w)
            assert bad.size == 0, "key of pattern %s: %d words differ, first at %d" % (PATTERNS[k], bad.size, bad[:1])
    finally:
        api.set_tuning("batch_keys", 0)
        api.set_deferred(False)
        restore()
        ks2.close()


@pytest.mark.parametrize("table", [1, 0], ids=["digit tables", "no tables"])
def test_wrap_rotations_in_both_halves_of_the_accumulator_update(cases, table):
    """The 4-wave form's accumulator update is split between the two primes' waves, registers [0, 8) and [8, 16) of a lane
    (coefficients below and from N / 2), and each wave stores the half it hands over before it finishes its own.  One
    input whose only steps rotate by 1, N - 1, N, N + 1 and 2N - 1: the wrap positions of X^abar ACC in both halves."""
    from peba1_amd import api
    c = cases("P128")
    pp, n, N = c.pp, c.pp.n, c.pp.N
    unit = 1 << (32 - N.bit_length())
    steps = {0: 1, 7: N - 1, n // 2: N, n - 2: N + 1, n - 1: 2 * N - 1}
    lin = np.zeros((1, pp.words), dtype=np.int32)
    for i, abar in steps.items():
        lin[0, i] = A.i32(abar * unit)
    lin[0, n] = A.i32(1300 * unit)
    bar = np.asarray(c.oks.modswitch_ct(lin[0]))
    assert {i: int(bar[i]) for i in np.flatnonzero(bar[:n])} == steps and bar[n] == 1300
    want = c.oks.blind_rotate(bar[:-1], bar[-1])
    try:
        api.set_tuning("br_variant", 0)
        api.set_tuning("br_digit_table", table)
        api.set_tuning("br8_max_rotations", 0)
        before = counters(api)
        u, acc = api.kernel_bootstrap_woks(c.ks, lin, want_acc=True)
        assert (counters(api) - before == expect_counters([A.WIDE4], table, pp.l, pp.Bgbit)).all()
    finally:
        restore()
    assert (acc[0] == want).all(), "accumulator: %d words differ" % np.count_nonzero(acc[0] != want)
    assert (u[0] == c.oks.sample_extract(want)).all()
