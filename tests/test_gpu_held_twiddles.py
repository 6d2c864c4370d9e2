"""Held forward twiddles in the 4-wave blind rotation.  A wave of that form keeps the second- and third-pass twiddles of its
forward transforms in registers over the gadget rows of a step (or longer) instead of reading them from LDS for every row.
Nothing of the arithmetic changes, so every accumulator word and every extracted word must be the oracle's -- at the
smallest shapes at which holding them could go wrong: N = 1024 and n = 16 steps; gadgets of l = 2, 3 and 4 rows, i.e. one,
two and three trips of the row loop behind the first row, with and without the digit table of the first radix-4 step; one
and three rotations per launch, on the 4-wave kernel by tuning; an input whose first, a middle and last step are skipped
(abar_i = 0: the loop's `continue` must leave what is held alone); and two cloud keys in one launch of the multi-key twin.
Each launch proves by the per-form launch counters which kernel and table mode it ran."""
import numpy as np
import pytest

import adversarial_common as A

pytestmark = pytest.mark.gpu

N_STEPS, RING = 16, 1024
TUNING_DEFAULTS = {"br_variant": -1, "br_digit_table": 1, "br8_max_rotations": 1 << 30, "br_tail8": 1}
WIDE4_TUNINGS = {"br_variant": 0, "br8_max_rotations": 0}
# (l, Bgbit, digit table asked for): digits of 7 bits or fewer can index the table, wider ones multiply whatever is asked
GADGETS = [(2, 10, 1), (2, 7, 1), (3, 7, 1), (3, 7, 0), (4, 8, 1), (4, 6, 1)]
SKIPPED = (0, N_STEPS // 2, N_STEPS - 1)


def restore():
    from peba1_amd import api
    for k, v in TUNING_DEFAULTS.items():
        api.set_tuning(k, v)


def counters(api):
    s = api.stats()
    return np.array([s[f] for f in A.FORM_COUNTERS + A.TABLE_COUNTERS], dtype=np.int64)


def expect_wide4(l, Bgbit, tables):
    want = np.zeros(7, dtype=np.int64)
    want[A.WIDE4] += 1
    want[4 + A.tables_run(A.WIDE4, l, Bgbit, tables)] += 1
    return want


def input_rows(pp, oks, seed):
    """Three input samples: random, one whose steps SKIPPED have abar_i = 0 (mask word 0) and no other, random."""
    n = pp.n
    unit = np.int32(1 << (32 - RING.bit_length()))       # switches to abar = 1
    rng = np.random.default_rng(seed)
    lin = rng.integers(-2**31, 2**31, (3, pp.words), dtype=np.int64).astype(np.int32)
    lin[1, list(SKIPPED)] = 0
    for r, zeros in ((0, set()), (1, set(SKIPPED)), (2, set())):
        bar = np.asarray(oks.modswitch_ct(lin[r]))
        stray = [i for i in np.flatnonzero(bar[:n] == 0) if i not in zeros]
        lin[r, stray] = unit
        bar = np.asarray(oks.modswitch_ct(lin[r]))
        assert set(np.flatnonzero(bar[:n] == 0)) == zeros
    return lin


class Case:
    pass


@pytest.fixture(scope="module")
def gadget_case(oracle):
    """(l, Bgbit) -> keys of the custom set, the three input rows and the oracle's accumulators and samples, made once."""
    from peba1_amd import api
    made = {}

    def get(l, Bgbit):
        if (l, Bgbit) not in made:
            c = Case()
            c.pp = api.ParameterSet(custom=(N_STEPS, RING, 1, l, Bgbit, 8, 2, 2.0 ** -15, 2.0 ** -25, 0.012467))
            c.seed = 0x7E1D + 16 * l + Bgbit
            c.ks = api.SecretKeySet(c.pp, c.seed, device=True)
            c.oks = oracle.KeySet(oracle.custom_params(n=N_STEPS, N=RING, l=l, Bgbit=Bgbit), c.seed)
            c.lin = input_rows(c.pp, c.oks, 100 * l + Bgbit)
            c.acc = []
            for row in c.lin:
                bar = c.oks.modswitch_ct(row)
                c.acc.append(c.oks.blind_rotate(bar[:-1], bar[-1]))
            c.acc = np.stack(c.acc)
            c.u = np.stack([c.oks.sample_extract(a) for a in c.acc])
            made[(l, Bgbit)] = c
        return made[(l, Bgbit)]
    yield get
    for c in made.values():
        c.ks.close()


@pytest.mark.parametrize("l,Bgbit,table", GADGETS, ids=["l%d_Bg%d_tab%d" % g for g in GADGETS])
def test_rows_of_a_step_share_held_twiddles(gadget_case, l, Bgbit, table):
    """Three rotations in one launch, then the first row and the row with skipped steps each alone, all on the 4-wave
    kernel: accumulators and extracted samples word for word."""
    from peba1_amd import api, lib
    c = gadget_case(l, Bgbit)
    assert lib.load().tfhe_hip_test_form_admissible(A.WIDE4, RING, l, Bgbit, table)
    try:
        for k, v in WIDE4_TUNINGS.items():
            api.set_tuning(k, v)
        api.set_tuning("br_digit_table", table)
        for rows in ([0, 1, 2], [0], [1]):
            before = counters(api)
            u, acc = api.kernel_bootstrap_woks(c.ks, c.lin[rows], want_acc=True)
            assert (counters(api) - before == expect_wide4(l, Bgbit, table)).all(), rows
            for k, r in enumerate(rows):
                bad = np.flatnonzero(acc[k] != c.acc[r])
                assert bad.size == 0, "rows %s, row %d: %d accumulator words differ, first at %d" % (rows, r, bad.size, bad[0])
                assert (u[k] == c.u[r]).all(), "rows %s, row %d: extracted sample" % (rows, r)
    finally:
        restore()


@pytest.mark.parametrize("l,Bgbit", [(3, 7), (2, 10), (4, 6)], ids=["l3_Bg7_table", "l2_Bg10_no_table", "l4_Bg6_table"])
def test_two_keys_in_one_launch_of_the_multikey_twin(gadget_case, oracle, l, Bgbit):
    """One flush of two gates under two cloud keys of one set, one rotation each, on the 4-wave multi-key kernel.  AND of
    (an input row minus the gate's constant) with a zero sample has that row as its prelude; the output is the oracle's
    key switch of the oracle's extracted sample, word for word.  The first key rotates the row with skipped steps."""
    from peba1_amd import api
    c = gadget_case(l, Bgbit)
    pp, n = c.pp, c.pp.n
    seed2 = c.seed + 0x1000
    ks2 = api.SecretKeySet(pp, seed2, device=True)
    oks2 = oracle.KeySet(oracle.custom_params(n=N_STEPS, N=RING, l=l, Bgbit=Bgbit), seed2)
    picks = [1, 2]
    api.set_deferred(True)
    api.set_tuning("batch_keys", 1)
    try:
        for k, v in WIDE4_TUNINGS.items():
            api.set_tuning(k, v)
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
        assert (counters(api) - before == expect_wide4(l, Bgbit, 1)).all()
        for (xa, za, ra), w, k in zip(held, want, picks):
            got = ra.words()[0]
            bad = np.flatnonzero(got != w)
            assert bad.size == 0, "key of row %d: %d words differ, first at %d" % (k, bad.size, bad[:1])
    finally:
        api.set_tuning("batch_keys", 0)
        api.set_deferred(False)
        restore()
        ks2.close()
