"""Blind rotation at its worst-case magnitudes: crafted cloud keys (tests/adversarial_common.py) drive the production
kernels, untouched, to the corners of the ranges they are admitted for -- the exact range of the signed two-prime CRT
(ntt_field.hpp CRT_EXACT_LIMIT) and the lazy-arithmetic bounds of each kernel form (br_forms.hpp) -- where generated keys
and honest accumulators stay six bits below.  Every word of every accumulator and extracted sample is compared with the
oracle's schoolbook evaluator on the same crafted words; every launch proves by the per-form launch counters which
kernel and which digit-table mode it ran."""
import itertools
import os

import numpy as np
import pytest

import adversarial_common as A

pytestmark = pytest.mark.gpu

TUNING_DEFAULTS = {"br_variant": -1, "br_digit_table": 1, "br8_max_rotations": 1 << 30, "br_tail8": 1,
                   "ks_tile": 16, "ks_index": 1}


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
    """One launch per form, each counted under the table mode it really runs with (A.tables_run): a planned mode the
    gadget's digits cannot index (Bgbit > 7, lowest field below bit 3, the 2-wave form) counts as mode 0."""
    want = np.zeros(7, dtype=np.int64)
    for f in forms:
        want[f] += 1
        want[4 + A.tables_run(f, l, Bgbit, tables)] += 1
    return want


class Crafted:
    pass


@pytest.fixture(scope="module")
def crafted(oracle, tmp_path_factory):
    """name -> the crafted set, its cloud key loaded from the file written here, the oracle twin and the oracle's
    accumulators and extracted samples of every case (checked against the integer reference)."""
    from peba1_amd import api
    made = {}

    def get(name, key_variant=0):
        if (name, key_variant) not in made:
            c = Crafted()
            c.cs = A.build_set(name, key_variant)
            path = tmp_path_factory.mktemp("adv") / ("%s_%d.key" % (name, key_variant))
            A.write_cloud_key(path, c.cs.params_tuple, c.cs.bk, c.cs.ksk)
            c.cloud = api.CloudKeySet.load(path)
            os.remove(path)
            c.oks = A.oracle_twin(oracle, c.cs)
            c.acc = A.oracle_accumulators(c.oks, c.cs)
            assert (c.acc == np.stack([k["expected"].reshape(-1) for k in c.cs.cases])).all()
            c.u = np.stack([c.oks.sample_extract(a) for a in c.acc])
            made[(name, key_variant)] = c
        return made[(name, key_variant)]
    yield get
    for c in made.values():
        c.cloud.close()


def assert_rows(got, want, cs, what, rows=None):
    rows = range(len(want)) if rows is None else rows
    for r, c in enumerate(rows):
        if not (got[r] == want[c]).all():
            k = cs.cases[c]
            bad = np.flatnonzero(got[r] != want[c])
            raise AssertionError("%s: %s, case %d (%s; largest exact coefficient 2^%.2f of the bound 2^%.2f): %d words differ, "
                                 "first at %d" % (cs.name, what, c, k["name"], np.log2(max(k["most"], 1)),
                                                  np.log2(A.crt_bound(cs.N, cs.l, cs.Bgbit)), bad.size, bad[0]))


@pytest.mark.parametrize("name", sorted(A.SETS))
def test_crafted_corners_in_every_kernel_form(crafted, name):
    """Corners of the product range (every digit -Bg/2, every digit Bg/2 - 1, alternating, a random pattern of the two;
    key rows constant -2^31, constant 2^31 - 1, one sign collected in coefficient 0, alternating, random extreme), the
    spectral corners (digits and key rows signed like Re psi^((2m+1) i), m = 0, 1, N/2 - 1, N - 1: all their weight in one
    transform bin) and the decisions of the gadget decomposition (rotated differences at 2^(32 - l Bgbit) m + {-1, 0, 1}
    and on the digit-field boundaries +- 1), under rotations 1, N - 1, N, N + 1, 2N - 1; among them the case whose exact
    coefficient EQUALS (k+1) l N (Bg/2) 2^31.  Each distinct (kernel form, digit-table mode) the tunings br_variant x
    br_digit_table x br8_max_rotations can reach for this gadget runs once, proven by the launch counters, and every
    word of every accumulator and extracted sample equals the oracle's.

    The spectral cases probe the interval bounds of br_forms.hpp far closer than random data does (the forward
    transform's output in one bin is the l1 norm of the digits); they do not prove them: the bounds are worst cases over
    every intermediate value of every stage, which no finite case list attains together."""
    from peba1_amd import api, lib
    c = crafted(name)
    cs, N, l, Bgbit = c.cs, c.cs.N, c.cs.l, c.cs.Bgbit
    ok = lib.load().tfhe_hip_test_form_admissible
    count, cus = len(cs.cases), cu_count()
    assert count <= cus, "the case list must fit the 8-wave form's one workgroup per CU"
    reach = {}
    for v, t, b8 in itertools.product((-1, 0, 2, 4), (0, 1, 2), (0, 1 << 30)):
        reach.setdefault(A.predicted_form(ok, N, l, Bgbit, count, cus, v, t, b8), []).append((v, t, b8))
    assert None not in reach, "a loadable key has an admissible form"
    excluded = [(A.FORM_NAMES[f], t) for f in range(4) for t in range(3) if not ok(f, N, l, Bgbit, t)]
    print("\n%s: forms x table modes the admissibility predicate excludes: %s" % (name, excluded or "none"))
    # every admissible (form, table mode) the engine would pick is reached by some tuning
    for f in range(4):
        if any(ok(f, N, l, Bgbit, t) for t in range(3)) and (N == 1024 or f == A.SPLIT):
            assert any(k[0] == f for k in reach), "%s: no tuning reaches the admissible form %s" % (name, A.FORM_NAMES[f])
    try:
        for (form, tables), tunings in sorted(reach.items()):
            v, t, b8 = tunings[0]
            api.set_tuning("br_variant", v)
            api.set_tuning("br_digit_table", t)
            api.set_tuning("br8_max_rotations", b8)
            before = counters(api)
            u, acc = api.kernel_bootstrap_woks(c.cloud, cs.lin, want_acc=True)
            what = "%s form, table mode %d (br_variant %d, br_digit_table %d, br8_max_rotations %d)" % (A.FORM_NAMES[form], tables, v, t, b8)
            assert (counters(api) - before == expect_counters([form], tables, l, Bgbit)).all(), what
            print("%s: %s: %d cases, %d tunings collapse here" % (name, what, count, len(tunings)))
            assert_rows(acc, c.acc, cs, what + ", accumulator")
            assert_rows(u, c.u, cs, what + ", extracted sample")
    finally:
        restore()


@pytest.mark.parametrize("name", [n for n in sorted(A.SETS) if A.SETS[n][0] == 1024])
def test_crafted_corners_in_the_full_round_and_in_the_8_wave_tail(crafted, name):
    """A launch of two workgroups per CU and a remainder: with br_tail8 the remainder runs as a second launch of the
    8-wave form (where that form admits the gadget), without it as a third, part-filled round of the 4-wave kernel.  The
    crafted rows are tiled over the launch so that every case lands in the full round and in the tail."""
    from peba1_amd import api, lib
    c = crafted(name)
    cs, N, l, Bgbit = c.cs, c.cs.N, c.cs.l, c.cs.Bgbit
    ok = lib.load().tfhe_hip_test_form_admissible
    cus, ncase = cu_count(), len(cs.cases)
    total = 2 * cus + min(ncase, cus)
    rows = np.arange(total) % ncase
    lin = cs.lin[rows]
    try:
        for tail8 in (1, 0):
            api.set_tuning("br_tail8", tail8)
            form, tb = A.predicted_form(ok, N, l, Bgbit, total, cus, -1, 1, 1 << 30)
            forms = [form] + ([A.WAVE8] if tail8 and form == A.WIDE4 and ok(A.WAVE8, N, l, Bgbit, tb) else [])
            before = counters(api)
            u = api.kernel_bootstrap_woks(c.cloud, lin)
            what = "%d rotations, br_tail8 %d, forms %s" % (total, tail8, [A.FORM_NAMES[f] for f in forms])
            assert (counters(api) - before == expect_counters(forms, tb, l, Bgbit)).all(), what
            print("\n%s: %s" % (name, what))
            assert_rows(u, c.u, cs, what, rows)
    finally:
        restore()


@pytest.mark.parametrize("name", ["P128", "P80"])
def test_crafted_corners_through_whole_gates_under_three_keys(crafted, name):
    """The same corners through recorded gates and the multi-key kernels: three crafted cloud keys of one parameter set
    (different fillers, sign patterns and key-switching words), batch_keys on, one flush.  AND of (the wanted word minus
    the gate's constant) with a zero sample, and for every fifth case MAJ3 with two zero samples, give the crafted `lin`
    rows as the prelude; every output word equals the oracle's key switch (crafted ksk: extreme words) of the extracted
    sample.  Wide: every case under every key on the 4-wave multi-key kernel; narrow: a third of them on the 8-wave one."""
    from peba1_amd import api
    sets = [crafted(name, v) for v in range(3)]
    cs0 = sets[0].cs
    n = cs0.n
    want = [np.stack([c.oks.keyswitch(u) for u in c.u]) for c in sets]
    cus = cu_count()
    api.set_deferred(True)
    api.set_tuning("batch_keys", 1)
    try:
        for label, pick, b8, form in (("wide", list(range(len(cs0.cases))), 0, A.WIDE4),
                                      ("narrow", list(range(0, len(cs0.cases), 3)), 1 << 30, A.WAVE8)):
            assert 3 * len(pick) <= (2 * cus if label == "wide" else cus)
            api.set_tuning("br8_max_rotations", b8)
            maj = [i for i in pick if i % 5 == 0]
            andg = [i for i in pick if i % 5]
            held = []
            for c in sets:
                pp = c.cloud.params
                a_and = c.cs.lin[andg].copy()
                a_and[:, n] = A.i32(a_and[:, n].astype(np.int64) + (1 << 29))     # AND adds (0, -1/8)
                xa = api.CiphertextArray(pp, len(andg)).set_words(a_and)
                za = api.CiphertextArray(pp, len(andg)).set_words(np.zeros_like(a_and))
                xm = api.CiphertextArray(pp, len(maj)).set_words(c.cs.lin[maj])
                zm = api.CiphertextArray(pp, len(maj)).set_words(np.zeros((len(maj), n + 1), dtype=np.int32))
                zm2 = api.CiphertextArray(pp, len(maj)).set_words(np.zeros((len(maj), n + 1), dtype=np.int32))
                held.append((xa, za, xm, zm, zm2, api.CiphertextArray(pp, len(andg)), api.CiphertextArray(pp, len(maj))))
            api.flush()
            s0, before = api.stats(), counters(api)
            for c, (xa, za, xm, zm, zm2, ra, rm) in zip(sets, held):
                api.gate_batch("AND", ra, xa, za, c.cloud)
                api.gate3_batch("MAJ3", rm, zm, xm, zm2, c.cloud)       # the crafted word as the second operand
            assert api.flush() >= 0, api.last_error()
            s1 = api.stats()
            what = "%s, %s: %d gates under 3 keys" % (name, label, 3 * len(pick))
            assert s1["flushes"] == s0["flushes"] + 1 and api.last_flush_keys() == 3, what
            assert s1["blind_rotates"] - s0["blind_rotates"] == 3 * len(pick), what
            delta = counters(api) - before
            assert delta[form] >= 1 and delta[:4].sum() == delta[form], (what, delta)
            for c, w, (xa, za, xm, zm, zm2, ra, rm) in zip(sets, want, held):
                assert_rows(ra.words(), w, c.cs, what + ", AND", andg)
                assert_rows(rm.words(), w, c.cs, what + ", MAJ3", maj)
    finally:
        api.set_tuning("batch_keys", 0)
        api.set_deferred(False)
        restore()


def test_modulus_switch_ties_with_a_generated_key(p128_keys, oracle):
    """lin words at (2m+1) 2^(31 - log2(2N)) + {-1, 0, +1}, where the modulus switch rounds up or down, for m at 0, N - 1,
    N and 2N - 1 (the last wraps to abar = 0), in every mask word and the body; a uniform word is there with probability
    2^-21."""
    from peba1_amd import api
    pp, ks, oks = p128_keys
    N, n = pp.N, pp.n
    step = 1 << (31 - N.bit_length())                           # half an interval of the switch to 2N
    ms = np.array([0, N - 1, N, 2 * N - 1], dtype=np.int64)
    lin = np.stack([A.i32((2 * ms[(np.arange(n + 1) + r) % 4] + 1) * step + d) for r in range(2) for d in (-1, 0, 1)])
    bar = np.stack([oks.modswitch_ct(row) for row in lin])
    assert (bar[1] != bar[0]).all() and (bar[1] == bar[2]).all() and (bar == 0).any() and (bar == N).any()
    u = api.kernel_bootstrap_woks(ks, lin)
    for r in range(len(lin)):
        assert (u[r] == oks.bootstrap_woks(lin[r])).all(), ("modulus-switch tie row", r)


def test_key_switch_ties_in_every_key_switch_form(p128_keys, oracle):
    """Extracted samples whose words sit at (2m+1) 2^(31 - t basebit) + {-1, 0, +1}, where the key switch's rounding offset
    carries into the lowest digit or does not, through the per-gate kernel, the tiled index form (tiles of 16, 24, 32)
    and the LDS-strip form; every output word against the oracle."""
    from peba1_amd import api
    pp, ks, oks = p128_keys
    rng = np.random.default_rng(0x715)
    half = 1 << (31 - pp.ks_t * pp.ks_basebit)
    count = 96
    m = rng.integers(0, (1 << 31) // half, (count, pp.N + 1))
    u = A.i32((2 * m + 1) * half + (np.arange(pp.N + 1)[None, :] + np.arange(count)[:, None]) % 3 - 1)
    want = np.stack([oks.keyswitch(row) for row in u])
    try:
        for tile, index in ((0, 1), (16, 1), (24, 1), (32, 1), (16, 0)):
            api.set_tuning("ks_tile", tile)
            api.set_tuning("ks_index", index)
            got = api.kernel_keyswitch(ks, u)
            assert (got == want).all(), ("key-switch ties", tile, index, np.flatnonzero((got != want).any(axis=1))[:5])
    finally:
        restore()
