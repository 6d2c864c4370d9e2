"""Every gadget the library accepts runs on the production kernels, not a sample of them.

unsupported_reason (engine.cpp) lets a key upload whenever br_form_admissible (br_forms.hpp) admits one kernel form and
the CRT bound is below CRT_EXACT_LIMIT: about 60 gadgets (l, Bgbit) at N = 1024 and 50 at N = 2048, on the word of an
interval-arithmetic model.  Here the accepted set is ENUMERATED from the library (tfhe_hip_test_form_admissible over
the forms and table modes, no list of gadgets in this file), and for each of its members a generated key runs a short
blind rotation in every (kernel form, digit-table mode) the planner can reach for it: every accumulator word and every
extracted word against the oracle, then an AND and a MUX through the public API (which also run the key switch).
Everything is exact integers; nothing is skipped.  The complement of the accepted set inside the grid is refused at
key upload.  tests/test_gpu_adversarial.py drives the frontier gadgets to the model's corner magnitudes with crafted
keys; this file is the breadth: l = 1, Bgbit 1 .. 11, a lowest digit field at bit 0, 1, 2, every table-mode edge."""
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import adversarial_common as A
from test_gpu_adversarial import counters, cu_count, restore

pytestmark = pytest.mark.gpu

RINGS = (1024, 2048)
N_LWE = 10                    # a short rotation: the gadget is what is under test
STDEVS = (2.0 ** -15, 2.0 ** -25, 0.012467)
# the gadgets the suite ran on a GPU before this file: only the coverage line of the summary reads them
OLD_SEVEN = {(1024, 3, 7), (1024, 2, 10), (2048, 3, 6), (1024, 4, 8), (2048, 6, 4), (1024, 8, 4), (2048, 2, 9)}
RAN = {}                      # (N, l, Bgbit) -> [(form, planned tables, tables run)] compared in this session


def grid(N):
    return [(N, l, B) for B in range(1, 13) for l in range(1, 32 // B + 1)]


def admissible():
    from peba1_amd import lib
    fn = lib.load().tfhe_hip_test_form_admissible
    return lambda f, N, l, B, t: fn(f, N, l, B, t) == 1


def accepted(ok, g):
    N, l, B = g
    return A.crt_bound(N, l, B) < A.CRT_EXACT_LIMIT and any(ok(f, N, l, B, t) for f in range(4) for t in range(3))


def reachable(ok, g, count, cus):
    """(form, planned table mode) -> the first tuning that reaches it, over br_variant x br_digit_table x
    br8_max_rotations for a launch of `count` rotations"""
    N, l, B = g
    reach = {}
    for v, t, b8 in itertools.product((-1, 0, 2, 4), (0, 1, 2), (0, 1 << 30)):
        reach.setdefault(A.predicted_form(ok, N, l, B, count, cus, v, t, b8), (v, t, b8))
    assert None not in reach, (g, "an accepted gadget has an admissible form")
    return reach


def inputs(N, seed):
    """Eight uniformly random rows, then the three sign-wrap rows: every abar (and bbar) = 1, = 2N - 1, = N."""
    unit = 1 << (32 - N.bit_length())
    rng = np.random.default_rng(seed)
    rnd = rng.integers(-2 ** 31, 2 ** 31, (8, N_LWE + 1), dtype=np.int64)
    edge = np.stack([np.full(N_LWE + 1, v, dtype=np.int64) for v in (unit, -unit, -2 ** 31)])
    return A.i32(np.concatenate([rnd, edge]))


def test_enumeration_is_the_librarys_and_has_its_known_members():
    """An empty or shrunken enumeration cannot pass for a sweep: members and non-members that are known by hand."""
    ok = admissible()
    acc = {g for N in RINGS for g in grid(N) if accepted(ok, g)}
    for g in ((1024, 1, 1), (1024, 9, 3), (1024, 1, 11), (2048, 7, 4), (2048, 5, 6)):
        assert g in acc, g
    for g in ((1024, 3, 10), (1024, 2, 11), (2048, 8, 4), (2048, 3, 9)):
        assert g not in acc, g
    assert OLD_SEVEN <= acc
    for N in RINGS:
        print("\nN = %d: %d gadgets accepted of %d in the grid" % (N, sum(g[0] == N for g in acc), len(grid(N))))


@pytest.mark.parametrize("N,Bgbit", [(N, B) for N in RINGS for B in range(1, 13)])
def test_every_accepted_gadget_in_every_reachable_form(oracle, N, Bgbit):
    """All accepted l of one (N, Bgbit).  Per gadget: the generated key equals the oracle's word for word; eleven input
    rows through every reachable (form, table mode), the form and the mode that ran proven by the launch counters, every
    accumulator and extracted word the oracle's; one AND and one MUX through the public API."""
    from peba1_amd import api, lib
    L = lib.load()
    ok = admissible()
    gadgets = [g for g in grid(N) if g[2] == Bgbit and accepted(ok, g)]
    if not gadgets:
        # not a skip: no l at all is accepted for these digits, because l = 1 already leaves the CRT range
        assert A.crt_bound(N, 1, Bgbit) >= A.CRT_EXACT_LIMIT
        return
    cus = cu_count()
    lin = inputs(N, 1000 * N + Bgbit)
    assert len(lin) <= cus, "a narrow launch: the 8-wave form runs where admissible"
    for g in gadgets:
        l = g[1]
        seed = 0x5EE9 + 64 * l + Bgbit
        pp = api.ParameterSet(custom=(N_LWE, N, 1, l, Bgbit, A.KS_T, A.KS_BASEBIT) + STDEVS)
        ks = api.SecretKeySet(pp, seed, device=True)
        oks = oracle.KeySet(oracle.custom_params(n=N_LWE, N=N, l=l, Bgbit=Bgbit, ks_t=A.KS_T, ks_basebit=A.KS_BASEBIT), seed)
        try:
            for name in ("lwe_key", "tlwe_key", "bk", "ksk"):
                assert np.array_equal(getattr(ks, name)(), getattr(oks, name)()), (g, name)

            def reference(row):
                bar = oks.modswitch_ct(row)
                acc = oks.blind_rotate(bar[:-1], bar[-1])
                return bar, acc, oks.sample_extract(acc)
            with ThreadPoolExecutor(16) as ex:
                ref = list(ex.map(reference, lin))
            bars = np.stack([r[0] for r in ref])
            assert (bars[8] == 1).all() and (bars[9] == 2 * N - 1).all() and (bars[10] == N).all(), (g, "sign-wrap rows")
            want_acc, want_u = np.stack([r[1] for r in ref]), np.stack([r[2] for r in ref])
            try:
                for (form, tables), (v, t, b8) in sorted(reachable(ok, g, len(lin), cus).items()):
                    api.set_tuning("br_variant", v)
                    api.set_tuning("br_digit_table", t)
                    api.set_tuning("br8_max_rotations", b8)
                    before = counters(api)
                    u, acc = api.kernel_bootstrap_woks(ks, lin, want_acc=True)
                    ran = A.tables_run(form, l, Bgbit, tables)
                    what = "%s: %s form, table mode %d planned, %d run (br_variant %d, br_digit_table %d, br8_max_rotations %d)" % (
                        g, A.FORM_NAMES[form], tables, ran, v, t, b8)
                    want = np.zeros(7, dtype=np.int64)
                    want[form] = want[4 + ran] = 1
                    assert (counters(api) - before == want).all(), what
                    for r in range(len(lin)):
                        assert (acc[r] == want_acc[r]).all(), (what, "accumulator of row", r, np.flatnonzero(acc[r] != want_acc[r])[:4])
                        assert (u[r] == want_u[r]).all(), (what, "extracted sample of row", r)
                    RAN.setdefault(g, []).append((form, tables, ran))
            finally:
                restore()
            cts = oks.encrypt(oracle.Rng(seed), [1, 0, 1])
            x = api.CiphertextArray(pp, 3).set_words(cts)
            res = api.CiphertextArray(pp, 2)
            L.bootsAND(res.at(0), x.at(0), x.at(2), ks.cloud)
            L.bootsMUX(res.at(1), x.at(0), x.at(1), x.at(2), ks.cloud)
            got = res.words()
            assert (got[0] == oks.gate("AND", cts[0], cts[2])).all(), (g, "AND", api.last_error())
            assert (got[1] == oks.mux(cts[0], cts[1], cts[2])).all(), (g, "MUX", api.last_error())
        finally:
            ks.close()
            oks.close()
    print("\nN = %d, Bgbit = %d: l = %s, %d launches compared" % (N, Bgbit, [g[1] for g in gadgets],
                                                                 sum(len(RAN[g]) for g in gadgets)))


def test_every_other_gadget_of_the_grid_is_refused_at_key_upload():
    """The complement: every gadget of the grid that is not accepted gets no key on the device, the reason
    unsupported_reason gives is in the error channel, and no kernel was launched for it."""
    from peba1_amd import api, lib
    L = lib.load()
    ok = admissible()
    refused = [g for N in RINGS for g in grid(N) if not accepted(ok, g)]
    assert (2048, 8, 4) in refused and (1024, 3, 10) in refused
    before = counters(api)
    for N, l, B in refused:
        why = ("exceed the exact range of the two-prime NTT" if A.crt_bound(N, l, B) >= A.CRT_EXACT_LIMIT
               else "every blind-rotate kernel form")
        pp = api.ParameterSet(custom=(2, N, 1, l, B, A.KS_T, A.KS_BASEBIT) + STDEVS)
        L.tfhe_hip_clear_error()
        with pytest.raises(RuntimeError, match=why):
            api.SecretKeySet(pp, 7, device=True)
        assert why in api.last_error(), (N, l, B)
    assert (counters(api) == before).all()
    print("\n%d gadgets refused: %d by the CRT range, %d by the kernel forms" % (
        len(refused), sum(A.crt_bound(*g) >= A.CRT_EXACT_LIMIT for g in refused),
        sum(A.crt_bound(*g) < A.CRT_EXACT_LIMIT for g in refused)))


def test_sweep_plan_covers_every_form_and_table_mode_beyond_the_old_seven():
    """The sweep's plan, from the enumeration and the planner's restatement alone (so it holds whichever of the tests
    above ran): per ring the accepted gadgets and the (gadget, form, table mode) launches, and every one of the four
    forms and of the three table modes really run (A.tables_run) is run by a gadget outside the seven the suite ran
    before.  What this session's tests compared is printed beside it and must be the plan's, gadget by gadget."""
    ok = admissible()
    cus = cu_count()
    forms, modes = set(), set()
    for N in RINGS:
        gadgets = [g for g in grid(N) if accepted(ok, g)]
        plan = {g: sorted((f, t, A.tables_run(f, g[1], g[2], t)) for f, t in reachable(ok, g, 11, cus)) for g in gadgets}
        for g, launches in plan.items():
            if g in RAN:
                assert sorted(RAN[g]) == launches, (g, RAN[g], launches)
            if g not in OLD_SEVEN:
                forms |= {f for f, _, _ in launches}
                modes |= {r for _, _, r in launches}
        print("\nN = %d: %d gadgets accepted, %d (gadget, form, table mode) launches planned; this session compared %d launches "
              "of %d gadgets" % (N, len(gadgets), sum(map(len, plan.values())), sum(len(RAN[g]) for g in plan if g in RAN),
                                 sum(g in RAN for g in plan)))
    print("forms run by gadgets outside the old seven: %s; table modes run: %s" % (
        [A.FORM_NAMES[f] for f in sorted(forms)], sorted(modes)))
    assert forms == {A.WIDE4, A.SPLIT, A.WAVE8, A.WAVE2} and modes == {0, 1, 2}
