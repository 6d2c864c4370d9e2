"""Every key-switch decomposition and every LWE row-width class the library accepts runs on the kernels.

unsupported_reason (engine.cpp) lets a key upload for the 81 pairs (ks_t, ks_basebit) with ks_basebit <= 8 and
ks_t * ks_basebit <= 31 and for every n in [1, 1024]; the rest of the suite runs (8, 2) at n = 500, 630, 1024 and toy
sizes.  Here every accepted pair runs on keyswitch_kernel -- the only kernel that serves 80 of them -- in every launch
shape the planner gives it, and (8, 2) runs at the widths where a workgroup's last wave is full, holds one lane, or the
workgroup has 64 or 256 threads, in every key-switch form.  Every output word is compared with the oracle's and with
ks_common.keyswitch_ref (the key switch from its definition); the launch shape is taken from the planner
(tfhe_hip_test_ks_plan at this card's CU count) and asserted before the run, and the ks_*_launches counters say which
kernel ran.  Nothing is skipped, every comparison is exact."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ks_common as K
from test_gpu_adversarial import cu_count, restore

pytestmark = pytest.mark.gpu

N, NL = K.N_RING, K.N_LWE
ONE_HOT = {K.PERGATE: (1, 0, 0), K.STRIP: (0, 1, 0), K.INDEX: (0, 0, 1)}


def ks_counters(api):
    s = api.stats()
    return np.array([s[f] for f in K.KS_COUNTERS], dtype=np.int64)


def restore_all():
    from peba1_amd import api
    api.set_tuning("ks_max_splits", K.KS_DEFAULTS["ks_max_splits"])
    restore()


def make_keys(oracle, n, t, bb, seed):
    """(parameter set, device keyset, oracle keyset) from one seed, generated side by side, equal word for word"""
    from peba1_amd import api
    l, Bgbit = K.GADGET
    pp = api.ParameterSet(custom=K.custom_tuple(n, t, bb))
    with ThreadPoolExecutor(2) as ex:
        fo = ex.submit(lambda: oracle.KeySet(oracle.custom_params(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb,
                                                                  ks_stdev=K.STDEVS[0], bk_stdev=K.STDEVS[1]), seed))
        ks = api.SecretKeySet(pp, seed, device=True)
        oks = fo.result()
    for name in ("lwe_key", "tlwe_key", "bk", "ksk"):
        assert np.array_equal(getattr(ks, name)(), getattr(oks, name)()), ((n, t, bb), name)
    return pp, ks, oks


def references(oks, u, n, t, bb):
    """the oracle's words of every row, which are the reference's"""
    with ThreadPoolExecutor(16) as ex:
        want = np.stack(list(ex.map(oks.keyswitch, u)))
    assert (want == K.keyswitch_ref(oks.ksk(), u, n, N, t, bb)).all(), ((n, t, bb), "oracle and reference differ")
    return want


def run_shape(L, api, ks, u, want, n, t, bb, tunings, form, what, rows=None, plan_check=None):
    """One raw key-switch launch: the plan of (shape, tunings, count) asserted first, then the run, the counters, the words."""
    rows = np.arange(len(u)) if rows is None else np.asarray(rows)
    plan = K.ks_plan(L, n, t, bb, tunings, cu_count(), len(rows))
    assert plan[6] == form and plan[0] == (form != K.PERGATE), (what, plan)
    if plan_check:
        plan_check(plan)
    for name in ("ks_tile", "ks_index", "ks_max_splits"):
        api.set_tuning(name, dict(K.KS_DEFAULTS, **tunings)[name])
    before = ks_counters(api)
    got = api.kernel_keyswitch(ks, u[rows])
    assert tuple(ks_counters(api) - before) == ONE_HOT[form], (what, "launch counters", tuple(ks_counters(api) - before))
    bad = np.flatnonzero((got != want[rows]).any(axis=1))
    assert bad.size == 0, (what, "rows that differ", bad[:8], "first word", np.flatnonzero(got[bad[0]] != want[rows][bad[0]])[:4])
    return plan


def gates_through_the_api(L, api, oracle, pp, ks, oks, seed, what):
    """An AND, a MUX and a NOT through the public API, every word the oracle's; the key switches ran per gate."""
    cts = oks.encrypt(oracle.Rng(seed), [1, 0, 1])
    x = api.CiphertextArray(pp, 3).set_words(cts)
    res = api.CiphertextArray(pp, 3)
    s0, before = api.stats(), ks_counters(api)
    L.bootsAND(res.at(0), x.at(0), x.at(2), ks.cloud)
    L.bootsMUX(res.at(1), x.at(0), x.at(1), x.at(2), ks.cloud)
    L.bootsNOT(res.at(2), x.at(1), ks.cloud)
    got = res.words()
    assert (got[0] == oks.gate("AND", cts[0], cts[2])).all(), (what, "AND", api.last_error())
    assert (got[1] == oks.mux(cts[0], cts[1], cts[2])).all(), (what, "MUX", api.last_error())
    assert (got[2] == oks.gate_not(cts[1])).all(), (what, "NOT", api.last_error())
    return api.stats()["keyswitches"] - s0["keyswitches"], ks_counters(api) - before


def test_enumeration_has_its_known_members():
    """An empty or shrunken grid cannot pass for a sweep (tests/test_ks_sweep_cpu.py asks the library for the same set)."""
    acc = set(K.accepted_grid())
    assert len(acc) == 81 and {(1, 1), (31, 1), (3, 8), (15, 2)} <= acc and not acc & {(4, 8), (16, 2), (3, 9)}


# ks_basebit -> its accepted ks_t, at most eight to a case (31 decompositions of base 2 in one case took 13 s)
SLICES = [(bb, tuple(range(lo, min(lo + 8, 31 // bb + 1)))) for bb in range(1, 9) for lo in range(1, 31 // bb + 1, 8)]


def test_the_slices_are_the_accepted_grid():
    assert sorted((t, bb) for bb, ts in SLICES for t in ts) == sorted(K.accepted_grid())
    assert sum(len(ts) for _, ts in SLICES) == 81


@pytest.mark.parametrize("bb,ts", SLICES, ids=["bb%d-t%d..%d" % (bb, ts[0], ts[-1]) for bb, ts in SLICES])
def test_every_accepted_decomposition(oracle, bb, ts):
    """The accepted t of one ks_basebit at N = 1024, n = 10, gadget (3, 7).  Per decomposition: the device keyset equals the
    oracle's; the sweep's rows through the per-gate kernel in four launch shapes -- one sample (64 ranges and the
    reduce), a handful under ks_max_splits 8 (8 ranges), 64 rows or more at the default tunings (wide, never tiled),
    ks_max_splits 1 (unsplit, straight to the pool) -- every word the oracle's and the reference's; then an AND, a MUX and
    a NOT, and one recorded level of 40 independent gates, which makes prepare_flush size the partial sums of this shape."""
    from peba1_amd import api, lib
    L = lib.load()
    assert all(K.accepted_by_rule(t, bb) for t in ts)
    stride = (NL + 1 + 3) & ~3
    deferred = api.get_deferred()
    launches = 0
    try:
        for t in ts:
            seed = 0x4B5 + 64 * t + bb
            what = "(ks_t, ks_basebit) = (%d, %d)" % (t, bb)
            pp, ks, oks = make_keys(oracle, NL, t, bb, seed)
            try:
                u, names = K.inputs(N, t, bb, 1000 * t + bb)
                K.check_inputs(u, names, N, t, bb)
                want = references(oks, u, NL, t, bb)
                wide = np.arange(max(64, len(u))) % len(u)

                def ranges(count, first, nbytes):
                    return lambda plan: plan[2:6] == (count, first, first, nbytes) or pytest.fail("%s: plan %s" % (what, plan))
                run_shape(L, api, ks, u, want, NL, t, bb, {}, K.PERGATE, what + ", one sample", rows=[0],
                          plan_check=ranges(1, 64, 64 * stride * 4))
                run_shape(L, api, ks, u, want, NL, t, bb, {"ks_max_splits": 8}, K.PERGATE, what + ", a handful in 8 ranges",
                          rows=[1, len(u) - 1, 6, 7, 8], plan_check=ranges(5, 8, 5 * 8 * stride * 4))
                run_shape(L, api, ks, u, want, NL, t, bb, {}, K.PERGATE, what + ", wide", rows=wide,
                          plan_check=ranges(len(wide), 64, len(wide) * 64 * stride * 4))
                run_shape(L, api, ks, u, want, NL, t, bb, {"ks_max_splits": 1}, K.PERGATE, what + ", unsplit", rows=wide,
                          plan_check=ranges(len(wide), 1, 0))
                launches += 4
                restore_all()
                nks, delta = gates_through_the_api(L, api, oracle, pp, ks, oks, seed, what)
                assert nks == 2 and delta[0] >= 1 and not delta[1:].any(), (what, nks, delta)
                # one recorded level of 40 independent gates
                rng = oracle.Rng(seed + 1)
                ca, cb = oks.encrypt(rng, np.arange(40) % 2), oks.encrypt(rng, (np.arange(40) // 2) % 2)
                a, b = api.CiphertextArray(pp, 40).set_words(ca), api.CiphertextArray(pp, 40).set_words(cb)
                r = api.CiphertextArray(pp, 40)
                api.set_deferred(True)
                api.flush()
                s0, before = api.stats(), ks_counters(api)
                api.gate_batch("NAND", r, a, b, ks)
                assert api.flush() >= 0, (what, api.last_error())
                s1 = api.stats()
                assert s1["flushes"] == s0["flushes"] + 1 and s1["keyswitches"] == s0["keyswitches"] + 40, what
                assert tuple(ks_counters(api) - before) == (1, 0, 0), (what, "the level's key switch", ks_counters(api) - before)
                assert (r.words() == oks.gate_batch("NAND", ca, cb, nthreads=8)).all(), (what, "level of 40 NANDs")
                api.set_deferred(deferred)
            finally:
                ks.close()
                oks.close()
    finally:
        api.set_deferred(deferred)
        restore_all()
    print("\nks_basebit %d: ks_t = %s, %d raw launches compared" % (bb, list(ts), launches))


def test_wider_digits_are_refused_at_key_upload_and_32_bits_at_the_parameter_set():
    """Every (t, bb) with t bb <= 31 and bb = 9 .. 12 gets no key on the device, with the key-switch reason in the error
    channel and no kernel launched; t bb = 32 is no parameter set."""
    from peba1_amd import api, lib
    L = lib.load()
    refused = [(t, bb) for t, bb in K.GRID if bb >= 9]
    assert refused == [(t, bb) for bb in (9, 10, 11, 12) for t in range(1, 31 // bb + 1)] and len(refused) == 10
    before = ks_counters(api)
    for t, bb in refused:
        pp = api.ParameterSet(custom=K.custom_tuple(1, t, bb))
        L.tfhe_hip_clear_error()
        with pytest.raises(RuntimeError, match="key-switch digits"):
            api.SecretKeySet(pp, 7, device=True)
        assert "key-switch digits" in api.last_error(), (t, bb)
    assert (ks_counters(api) == before).all()
    for t, bb in ((32, 1), (16, 2), (8, 4), (4, 8), (2, 16), (1, 32)):
        with pytest.raises(ValueError, match="parameter set rejected"):
            api.ParameterSet(custom=K.custom_tuple(1, t, bb))


@pytest.fixture(scope="module")
def width_keys(oracle):
    """n -> the (8, 2) keyset of that LWE width, one per n for the module: key generation dominates at n >= 767"""
    made = {}

    def get(n):
        if n not in made:
            made[n] = make_keys(oracle, n, 8, 2, 0x7A0 + n)
        return made[n]
    yield get
    for _, ks, oks in made.values():
        ks.close()
        oks.close()


FORMS = (({"ks_tile": 16, "ks_index": 1}, K.INDEX), ({"ks_tile": 24, "ks_index": 1}, K.INDEX),
         ({"ks_tile": 32, "ks_index": 1}, K.INDEX), ({"ks_tile": 16, "ks_index": 0}, K.STRIP),
         ({"ks_tile": 0, "ks_index": 1}, K.PERGATE))


@pytest.mark.parametrize("n", K.ROW_WIDTHS)
def test_every_row_width_class(oracle, width_keys, n):
    """(8, 2), N = 1024: n = 1 .. 4 (one lane and its padding), 255 / 511 / 767 / 1023 (a full last wave, no padding word:
    the body is a lane's last word), 256 / 512 (one lane in the last wave), 768 and 1023 (256 threads).  77 rows -- four
    tiles of 16 and 13 gates, three of 24 and 5, two of 32 and 13 -- through the index form at tiles 16, 24, 32, the strip
    form and the per-gate kernel; the counters show the form the plan names: index / strips at 128 and 192 threads, the
    per-gate kernel at 64 and 256.  Then gates, a 16-term linear combination with extreme coefficients and an export /
    import round trip at the same width."""
    from peba1_amd import api, lib
    L = lib.load()
    pp, ks, oks = width_keys(n)
    what = "n = %d (%d threads)" % (n, K.threads(n))
    u, names = K.inputs(N, 8, 2, 31 * n, rows=77)
    assert len(u) == 77 and {"zero", "ones", "digit 1 at 0", "digit 3 at 7"} <= set(names)
    K.check_inputs(u, names, N, 8, 2)
    want = references(oks, u, n, 8, 2)
    tiled_width = K.threads(n) in (128, 192)
    assert tiled_width == (n in (256, 511, 512, 767)) and K.threads(n) in (64, 128, 192, 256)
    try:
        for tunings, form in FORMS:
            form = form if tiled_width else K.PERGATE
            plan = run_shape(L, api, ks, u, want, n, 8, 2, tunings, form, "%s, %s" % (what, tunings))
            if form != K.PERGATE:
                assert plan[1] == tunings["ks_tile"] and -(-N // plan[3]) <= 64, (what, plan)
    finally:
        restore_all()
    nks, delta = gates_through_the_api(L, api, oracle, pp, ks, oks, 0x11 + n, what)
    assert nks == 2 and delta[0] >= 1 and not delta[1:].any(), (what, nks, delta)
    # a 16-term linear combination, extreme coefficients, against numpy; no bootstrap and no key switch
    rng = np.random.default_rng(n)
    words = rng.integers(-2 ** 31, 2 ** 31, (16, n + 1), dtype=np.int64)
    coefs = [2 ** 31 - 1, -2 ** 31, 1, -1, 0x55555555, -0x55555556, 2, -2, 2 ** 30, -2 ** 30 - 1, 3, 65537, -65537, 0, 2 ** 31 - 2, -2 ** 31 + 1]
    c0 = -2 ** 31
    x = api.CiphertextArray(pp, 16).set_words(words.astype(np.int32))
    y = api.CiphertextArray(pp, 1)
    api.linear(y.at(0), [x.at(i) for i in range(16)], coefs, c0, ks)
    expect = sum((int(c) * words[i]) % 2 ** 32 for i, c in enumerate(coefs)) % 2 ** 32
    expect[n] = (expect[n] + c0) % 2 ** 32
    assert (y.words()[0].astype(np.int64) % 2 ** 32 == expect).all(), (what, "linear combination", api.last_error())
    # export / import round trip
    z = api.CiphertextArray(pp, 16).set_words(x.words())
    assert (z.words() == words.astype(np.int32)).all(), (what, "export / import")


@pytest.mark.parametrize("t,bb,n", [(t, bb, n) for t, bb in ((3, 8), (31, 1)) for n in (255, 768)])
def test_widest_row_tables_at_untested_widths(oracle, t, bb, n):
    """The most rows per coefficient (255 at base 256) and the most digit positions (31 at base 2), at a workgroup of 64
    threads with a full wave and at one of 256: one sample, every row at the default tunings, every row unsplit; an AND, a
    MUX and a NOT.  The (3, 8) key at n = 768 holds 2.4 GB: its generation is most of this case's time."""
    from peba1_amd import api, lib
    L = lib.load()
    what = "(ks_t, ks_basebit) = (%d, %d), n = %d" % (t, bb, n)
    pp, ks, oks = make_keys(oracle, n, t, bb, 0x3B0 + n + t)
    try:
        u, names = K.inputs(N, t, bb, n + t)
        K.check_inputs(u, names, N, t, bb)
        want = references(oks, u, n, t, bb)
        try:
            run_shape(L, api, ks, u, want, n, t, bb, {}, K.PERGATE, what + ", one sample", rows=[len(u) - 1])
            run_shape(L, api, ks, u, want, n, t, bb, {}, K.PERGATE, what + ", every row")
            run_shape(L, api, ks, u, want, n, t, bb, {"ks_max_splits": 1}, K.PERGATE, what + ", unsplit",
                      plan_check=lambda plan: plan[3:6] == (1, 1, 0) or pytest.fail("%s: plan %s" % (what, plan)))
        finally:
            restore_all()
        nks, delta = gates_through_the_api(L, api, oracle, pp, ks, oks, n + t, what)
        assert nks == 2 and delta[0] >= 1 and not delta[1:].any(), (what, nks, delta)
    finally:
        ks.close()
        oks.close()
