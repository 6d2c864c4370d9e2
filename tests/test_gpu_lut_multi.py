"""GPU tests of the multi-output LUT bootstrap (tfhe_hip_lut_bootstrap_multi): word for word against the committed
digests of the restatement (tests/golden/lut_multi_digests.json, tests/lut_multi_common.py) through the recorded path
and, through the raw entry, in every blind-rotate kernel form -- there the returned accumulator is also pushed through
the numpy restatement, and half of every launch are plain extracts; against tfhe_hip_lut_bootstrap with the one-tap
spec; a three-key flush; dead outputs and sharing through the counters; a 2-bit decomposition and a full adder at
decrypt level.  No oracle bootstrap runs here: inputs are oracle ENCRYPTIONS (cheap) from the fixtures' seeds."""
import contextlib

import numpy as np
import pytest

import lut_common as T
import lut_multi_common as M

pytestmark = pytest.mark.gpu
I32 = np.int32
DEFAULTS = {"br_variant": -1, "br8_max_rotations": 1 << 30, "br_tail8": 1, "br_digit_table": 1}


@pytest.fixture(scope="module")
def api():
    from peba1_amd import api
    return api


@pytest.fixture(scope="module")
def sets(api, oracle):
    """pname -> (parameter set, product keyset on the device, oracle keyset), made on demand from the fixture's seed."""
    made = {}

    def get(pname):
        if pname not in made:
            pp = {"P128": lambda: api.ParameterSet(128), "P80": lambda: api.ParameterSet(80),
                  "P2048": lambda: api.ParameterSet(p2048=True)}[pname]()
            made[pname] = (pp, api.SecretKeySet(pp, M.KEY_SEED, device=True), oracle.KeySet(oracle.params(pname), M.KEY_SEED))
        return made[pname]
    yield get
    for _, ks, oks in made.values():
        ks.close()
        oks.close()


@contextlib.contextmanager
def tunings(api, **kw):
    for k, v in kw.items():
        api.set_tuning(k, v)
    try:
        yield
    finally:
        for k in kw:
            api.set_tuning(k, DEFAULTS.get(k, 0))


@contextlib.contextmanager
def deferred(api, on=True):
    was = api.get_deferred()
    api.set_deferred(on)
    try:
        yield
    finally:
        api.set_deferred(was)


def delta(api, before):
    now = api.stats()
    return {k: now[k] - before[k] for k in now}


def _clear_error():
    from peba1_amd import lib
    lib.load().tfhe_hip_clear_error()


def make_multi(api, pp, case):
    lut = api.Lut(pp, T.lut_words(case["lut"], pp.N))
    mo = api.LutMulti(lut, M.spec_of(case))
    lut.close()
    return mo


def record_case(api, pp, ks, O, oks, case, keep, wanted=None):
    """Records one fixture case; returns one single-sample array per output (None where not wanted)."""
    wanted = case["wanted"] if wanted is None else wanted
    inputs = api.CiphertextArray(pp, len(case["coefs"])).set_words(T.case_inputs(O, oks, case))
    mo = make_multi(api, pp, case)
    rs = [api.CiphertextArray(pp, 1) if w else None for w in wanted]
    _clear_error()
    api.lut_bootstrap_multi(mo, [r.at(0) if r is not None else None for r in rs],
                            [inputs.at(i) for i in range(inputs.count)], case["coefs"], case["c0"], ks)
    assert api.last_error() == ""
    keep += [inputs, mo]
    return rs


def check_output(words, case, m):
    assert [int(x) for x in words[:4]] == case["first_words"][m], (case["parameter_set"], case["index"], m)
    assert T.sha256_words(words) == case["sha256"][m], (case["parameter_set"], case["index"], m)


def check_case(rs, case):
    for m, r in enumerate(rs):
        if r is not None:
            check_output(r.words()[0], case, m)


@pytest.mark.parametrize("pname", list(M.CASES))
def test_every_fixture_case_through_the_recorded_path(api, sets, oracle, pname):
    pp, ks, oks = sets(pname)
    cases = M.load_digests()["sets"][pname]["cases"]
    keep = []
    before = api.stats()
    with deferred(api):
        results = [record_case(api, pp, ks, oracle, oks, c, keep) for c in cases]
        assert api.flush() == 1
    d = delta(api, before)
    wanted = sum(sum(c["wanted"]) for c in cases)
    assert d["multi_rotations"] == len(cases) == d["blind_rotates"] == d["lut_rotations"]
    assert d["multi_outputs"] == d["keyswitches"] == wanted
    for rs, c in zip(results, cases):
        check_case(rs, c)
    for x in keep:
        x.close()


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# (parameter set, tunings, rotations or None = two per case, raw accumulators, expected launch counters): the rows of
# tests/test_gpu_lut.py
RAW_ROWS = {
    "wide4 tables": ("P128", dict(br_variant=0, br8_max_rotations=0), None, True, dict(br_wide4_launches=1, br_tables1_launches=1)),
    "wide4 no tables": ("P128", dict(br_variant=0, br8_max_rotations=0, br_digit_table=0), None, True,
                        dict(br_wide4_launches=1, br_tables0_launches=1)),
    "wide4 P80": ("P80", dict(br_variant=0, br8_max_rotations=0), None, True, dict(br_wide4_launches=1)),
    "wave8": ("P128", dict(), None, True, dict(br_wave8_launches=1, br_wide4_launches=0)),
    "wave8 P80": ("P80", dict(), None, True, dict(br_wave8_launches=1, br_wide4_launches=0)),
    "wide4 with wave8 tail": ("P128", dict(), "tail", False, dict(br_wide4_launches=1, br_wave8_launches=1)),
    "split P2048": ("P2048", dict(), None, True, dict(br_split_launches=1)),
    "split P128": ("P128", dict(br_variant=2), None, True, dict(br_split_launches=1, br_wide4_launches=0, br_wave8_launches=0)),
    "wave2": ("P128", dict(br_variant=4), None, True, dict(br_wave2_launches=1, br_wide4_launches=0, br_wave8_launches=0)),
}


@pytest.mark.parametrize("row", list(RAW_ROWS))
def test_fixture_cases_through_the_raw_entry_in_every_form(api, sets, oracle, row):
    """Combination 2i runs case i through its spec, combination 2i + 1 the same input with spec -1 (the plain extract):
    mixed launches, so the samples of a multi-output rotation lie between those of plain ones."""
    pname, tune, count, want_acc, counters = RAW_ROWS[row]
    pp, ks, oks = sets(pname)
    cases = M.load_digests()["sets"][pname]["cases"]
    polys = np.stack([T.lut_words(c["lut"], pp.N) for c in cases])
    lins = np.stack([M.case_lin(oracle, oks, c) for c in cases])
    specs = [M.spec_of(c) for c in cases]
    count = 2 * len(cases) if count is None else 2 * cu_count() + 8      # "tail": two full rounds and 8 rotations more
    which = (np.arange(count) // 2) % len(cases)
    spec_index = np.where(np.arange(count) % 2 == 0, which, -1).astype(I32)
    with tunings(api, **tune):
        before = api.stats()
        out = api.kernel_lut_bootstrap_multi_woks(ks, lins[which], which.astype(I32), polys, spec_index, specs, want_acc=want_acc)
        d = delta(api, before)
        plain = api.kernel_lut_bootstrap_woks(ks, lins, np.arange(len(cases), dtype=I32), polys)
    for k, v in counters.items():
        assert d[k] == v, (row, k, d[k])
    assert d["lut_rotations"] == count == d["blind_rotates"] and d["multi_rotations"] == count // 2
    assert d["multi_outputs"] == sum(len(specs[ci]) for ci in which[0::2])
    u, acc = out if want_acc else (out, None)
    for i, ci in enumerate(which):
        if spec_index[i] < 0:
            assert (u[i, 0] == plain[ci]).all() and not u[i, 1:].any(), (row, i)
            continue
        nout = len(specs[ci])
        assert [T.sha256_words(w) for w in u[i, :nout]] == cases[ci]["sha256_extracted"], (row, i)
        assert not u[i, nout:].any()
        if want_acc:
            assert T.sha256_words(acc[i]) == cases[ci]["sha256_accumulator"], (row, i)
            for m, w in enumerate(M.outputs(acc[i], specs[ci])):          # independently: the restatement of what came back
                assert (w == u[i, m]).all(), (row, i, m)
    # the key switch of the extracted outputs = the recorded words
    first = {ci: i for i, ci in reversed(list(enumerate(which))) if spec_index[i] >= 0}
    todo = [(ci, m) for ci in sorted(first) for m, w in enumerate(cases[ci]["wanted"]) if w]
    ct = api.kernel_keyswitch(ks, np.stack([u[first[ci], m] for ci, m in todo]))
    for w, (ci, m) in zip(ct, todo):
        check_output(w, cases[ci], m)


def test_the_one_tap_spec_gives_the_lut_bootstraps_words(api, sets, oracle):
    pp, ks, oks = sets("P128")
    lcases = T.load_digests()["sets"]["P128"]["cases"][:4]
    keep = []
    with deferred(api):
        for c in lcases:
            inputs = api.CiphertextArray(pp, len(c["coefs"])).set_words(T.case_inputs(oracle, oks, c))
            lut = api.Lut(pp, T.lut_words(c["lut"], pp.N))
            mo = api.LutMulti(lut, M.IDENTITY)
            want, got = api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 1)
            ins = [inputs.at(i) for i in range(inputs.count)]
            api.lut_bootstrap(lut, want.at(0), ins, c["coefs"], c["c0"], ks)
            api.lut_bootstrap_multi(mo, [got.at(0)], ins, c["coefs"], c["c0"], ks)
            keep += [inputs, lut, mo, (want, got, c)]
        assert api.flush() == 1
    for x in keep:
        if isinstance(x, tuple):
            want, got, c = x
            assert (got.words() == want.words()).all()
            assert T.sha256_words(got.words()[0]) == c["sha256"]
        else:
            x.close()
    # immediate mode: complete on return, every result's host mirror refreshed
    c = M.load_digests()["sets"]["P128"]["cases"][1]
    with deferred(api, False):
        rs = record_case(api, pp, ks, oracle, oks, c, keep := [])
        for m, r in enumerate(rs):
            assert [r.ptr.contents.a[i] for i in range(3)] == c["first_words"][m][:3]
        check_case(rs, c)
    for x in keep:
        x.close()


def test_three_key_flush_mixing_multi_output_ops_lut_ops_and_gates(api, sets, oracle):
    """One level under three cloud keys of one set (batch_keys): multi-output and LUT ops against their fixtures' digests
    under the fixtures' key, two-input gates and a MUX under two other keys against the oracle's words."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = sets("P128")
    cases = M.load_digests()["sets"]["P128"]["cases"]
    lcases = T.load_digests()["sets"]["P128"]["cases"][:4]
    others = [(api.SecretKeySet(pp, s, device=True), oracle.KeySet(oracle.params("P128"), s)) for s in (21, 22)]
    keep = []
    was = L.tfhe_hip_set_batch_keys(1)
    try:
        with deferred(api):
            before = api.stats()
            multi_results, lut_results, gate_results = [], [], []
            for i, c in enumerate(cases):
                multi_results.append(record_case(api, pp, ks, oracle, oks, c, keep))
                k2, o2 = others[i % 2]
                w = o2.encrypt(oracle.Rng(700 + i), [i & 1, (i >> 1) & 1, 1])
                ins = api.CiphertextArray(pp, 3).set_words(w)
                r = api.CiphertextArray(pp, 1)
                if i == 3:
                    L.bootsMUX(r.at(0), ins.at(0), ins.at(1), ins.at(2), k2.cloud)
                    want = o2.mux(w[0], w[1], w[2], 2)
                else:
                    name = ("AND", "XOR", "ORYN")[i % 3]
                    L.tfhe_hip_gate_batch(api.GATE_CODES[name], r.ptr, ins.at(0), ins.at(1), 1, k2.cloud)
                    want = o2.gate(name, w[0], w[1], 2)
                keep.append(ins)
                gate_results.append((r, want))
                if i < len(lcases):
                    lc = lcases[i]
                    li = api.CiphertextArray(pp, len(lc["coefs"])).set_words(T.case_inputs(oracle, oks, lc))
                    lut = api.Lut(pp, T.lut_words(lc["lut"], pp.N))
                    lr = api.CiphertextArray(pp, 1)
                    api.lut_bootstrap(lut, lr.at(0), [li.at(j) for j in range(li.count)], lc["coefs"], lc["c0"], ks)
                    keep += [li, lut]
                    lut_results.append((lr, lc))
            assert api.flush() == 1
            d = delta(api, before)
        assert api.last_flush_keys() == 3
        wanted = sum(sum(c["wanted"]) for c in cases)
        assert d["multi_rotations"] == 8 and d["multi_outputs"] == wanted and d["lut_rotations"] == 8 + 4
        assert d["blind_rotates"] == 8 + 4 + 8 + 1 and d["keyswitches"] == wanted + 4 + 8
        for rs, c in zip(multi_results, cases):
            check_case(rs, c)
        for lr, lc in lut_results:
            assert T.sha256_words(lr.words()[0]) == lc["sha256"]
        for i, (r, want) in enumerate(gate_results):
            assert (r.words()[0] == want).all(), i
    finally:
        L.tfhe_hip_set_batch_keys(was)
        for x in keep:
            x.close()
        for k2, o2 in others:
            k2.close()
            o2.close()


def test_dead_outputs_and_sharing_are_seen_in_the_counters(api, sets, oracle):
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = sets("P128")
    c = M.load_digests()["sets"]["P128"]["cases"][4]              # four outputs, all wanted in the fixture
    inputs = api.CiphertextArray(pp, len(c["coefs"])).set_words(T.case_inputs(oracle, oks, c))
    ins = [inputs.at(i) for i in range(inputs.count)]
    mo = make_multi(api, pp, c)

    def record(wanted):
        rs = [api.CiphertextArray(pp, 1) if w else None for w in wanted]
        api.lut_bootstrap_multi(mo, [r.at(0) if r is not None else None for r in rs], ins, c["coefs"], c["c0"], ks)
        assert api.last_error() == ""
        return rs

    with deferred(api):
        # an output overwritten before the flush is dead: it loses its key switch, the rotation stays
        before = api.stats()
        rs = record([True, True, True, True])
        L.bootsCONSTANT(rs[2].at(0), 1, ks.cloud)
        assert api.flush() == 1
        d = delta(api, before)
        assert (d["multi_rotations"], d["multi_outputs"], d["keyswitches"], d["blind_rotates"]) == (1, 3, 3, 1)
        check_case([rs[0], rs[1], None, rs[3]], c)
        assert rs[2].decrypt(ks)[0] == 1
        # every output dead: the op goes, nothing runs
        before = api.stats()
        rs = record([True, False, True, False])
        for r in (rs[0], rs[2]):
            L.bootsCONSTANT(r.at(0), 0, ks.cloud)
        api.flush()
        d = delta(api, before)
        assert (d["multi_rotations"], d["blind_rotates"], d["keyswitches"], d["dead_gates"]) == (0, 0, 0, 1)
        # an equal op shares output by output and widens the pending one by what it lacked: one rotation, three outputs
        before = api.stats()
        first = record([True, False, True, False])
        second = record([True, True, False, False])
        assert api.flush() == 1
        d = delta(api, before)
        assert (d["multi_rotations"], d["multi_outputs"], d["keyswitches"], d["reused_gates"]) == (1, 3, 3, 1)
        check_case(first, c)
        check_case(second, c)
        assert (first[0].words() == second[0].words()).all()
        # with sharing off: two rotations
        api.set_tuning("reuse_gates", 0)
        try:
            before = api.stats()
            both = [record([True, False, False, True]), record([False, True, False, True])]
            api.flush()
            d = delta(api, before)
        finally:
            api.set_tuning("reuse_gates", 1)
        assert (d["multi_rotations"], d["multi_outputs"], d["keyswitches"]) == (2, 4, 4)
        for rs in both:
            check_case(rs, c)
        # deleting the object with an op pending runs the recording first
        pending = record([False, False, True, False])
        before = api.stats()
        mo.close()
        assert delta(api, before)["flushes"] == 1
        check_case(pending, c)
    inputs.close()


def test_spec_table_grows_and_entries_are_reused_between_flushes(api, sets, oracle):
    """The twin of test_gpu_lut.py::test_lut_table_grows_and_entries_are_reused_between_flushes for the table of extract
    specs: 40 one-tap specs that differ in out_c0 alone, so output i is the lut_bootstrap sample with out_c0[i] added to
    its body (the key switch passes the body through) -- an op that read a neighbour's spec shows in that one word."""
    pp, ks, oks = sets("P128")
    cases = M.load_digests()["sets"]["P128"]["cases"]
    case = cases[1]
    c0s = [int(T.wrap32((i * 0x9E3779B1 + 12345) & 0xFFFFFFFF)) for i in range(60)]       # distinct: an odd multiplier
    keep = []

    def check_reads_own_spec(results, want):
        want = want.words()[0].astype(np.int64)
        for r, c0 in results:
            got = r.words()[0].astype(np.int64)
            assert (got[:-1] == want[:-1]).all(), c0
            assert (got[-1] - want[-1] - c0) % (1 << 32) == 0, c0

    with deferred(api):
        first = record_case(api, pp, ks, oracle, oks, case, keep)
        assert api.flush() == 1
        check_case(first, case)
        # 40 specs more, each used once: the device table (16 entries at first) doubles twice within this recording
        lut = api.Lut(pp, T.lut_words(cases[0]["lut"], pp.N))
        a = api.CiphertextArray(pp, 1).encrypt([1], ks)
        want = api.CiphertextArray(pp, 1)

        def record(c0):
            mo, r = api.LutMulti(lut, [([(0, 1)], c0)]), api.CiphertextArray(pp, 1)
            api.lut_bootstrap_multi(mo, [r.at(0)], [a.at(0)], [1], 0, ks)
            assert api.last_error() == ""
            return mo, r

        before = api.stats()
        fill = [record(c0) for c0 in c0s[:40]]
        api.lut_bootstrap(lut, want.at(0), [a.at(0)], [1], 0, ks)
        again = record_case(api, pp, ks, oracle, oks, case, keep)
        assert api.flush() == 1
        d = delta(api, before)
        # (nothing is shared: every object holds its own copy of the polynomial and its own spec)
        assert (d["multi_rotations"], d["multi_outputs"]) == (40 + 1, 40 + sum(case["wanted"]))
        assert d["blind_rotates"] == 40 + 1 + 1
        check_reads_own_spec([(r, c0) for (_, r), c0 in zip(fill, c0s)], want)
        check_case(again, case)
        check_case(first, case)
        # 20 objects go, 20 new ones take their entries; the survivors are recorded again beside them
        for mo, _ in fill[0::2]:
            mo.close()
        before = api.stats()
        fresh = [record(c0) for c0 in c0s[40:]]
        survivors = []
        for (mo, _), c0 in zip(fill[1::2], c0s[1:40:2]):
            r = api.CiphertextArray(pp, 1)
            api.lut_bootstrap_multi(mo, [r.at(0)], [a.at(0)], [1], 0, ks)
            survivors.append((r, c0))
        assert api.flush() == 1
        d = delta(api, before)
        assert (d["multi_rotations"], d["multi_outputs"], d["blind_rotates"]) == (40, 40, 40)
        check_reads_own_spec([(r, c0) for (_, r), c0 in zip(fresh, c0s[40:])] + survivors, want)
    for x in keep + [mo for mo, _ in fill[1::2] + fresh] + [lut, a]:
        x.close()


def fresh_at(O, oks, values, seed):
    """Fresh encryptions at given torus phases: an oracle encryption of bit 1 (phase 1/8 + e) moved there."""
    cts = oks.encrypt(O.Rng(seed), [1] * len(values))
    for ct, v in zip(cts, values):
        ct[-1] = T.wrap32(int(ct[-1]) + int(v) - (1 << 29))
    return cts


def signed(ph):
    return (np.asarray(ph) + 0.5) % 1 - 0.5


def noise_report(name, err, weights, typ):
    w2 = sum(w * w for w in weights)
    print(f"  {name}: weights {weights}  output variance {err.var():.3e}  sum w^2 x predicted typical = {w2} x {typ:.3e} = "
          f"{w2 * typ:.3e}  max |e| {np.abs(err).max():.4f}")


def test_two_bit_message_decomposed_into_gate_bits_by_one_rotation(api, sets, oracle):
    """256 fresh 2-bit messages (phase (2m+1)/16), one rotation each -> both bits in the gates' encoding (+-1/8), which
    then go through bootsAND and bootsXOR: every decrypted bit must be right.  Variances are printed, not asserted."""
    from test_gpu_noise import SETS, predicted_variance
    pp, ks, oks = sets("P128")
    _, typ, _ = predicted_variance(pp, SETS[0][1], SETS[0][2])
    G = 256
    msgs = np.random.default_rng(12).integers(0, 4, G)
    mo = api.LutMulti.from_tables(pp, 1 << 29, [[-1, 1, -1, 1], [-1, -1, 1, 1]])
    before = api.stats()
    with deferred(api):
        a = api.CiphertextArray(pp, G).set_words(T.encode_messages(oracle, oks, msgs, 2024))
        lo, hi, both, either = (api.CiphertextArray(pp, G) for _ in range(4))
        api.lut_bootstrap_multi_batch(mo, [lo, hi], [a], [1], 0, ks)
        api.gate_batch("AND", both, lo, hi, ks)
        api.gate_batch("XOR", either, lo, hi, ks)
        assert api.flush() == 2
    d = delta(api, before)
    assert d["multi_rotations"] == G and d["multi_outputs"] == 2 * G and d["blind_rotates"] == 3 * G
    key = ks.lwe_key()
    print("\n2-bit decomposition, 256 messages, one rotation each:")
    smallest = 1.0
    for name, arr, bit, taps in (("low bit", lo, msgs & 1, mo.outputs()[0][0]), ("high bit", hi, msgs >> 1, mo.outputs()[1][0])):
        ph = signed(T.phases(arr.words(), key))
        assert ((ph > 0).astype(int) == bit).all(), name
        smallest = min(smallest, float(np.minimum(np.abs(ph), 0.5 - np.abs(ph)).min()))
        noise_report(name, ph - (2 * bit - 1) / 8, [w for _, w in taps], typ)
    print(f"  smallest distance from a decision boundary (0 and 1/2; ideal 1/8): {smallest:.4f}")
    assert (both.decrypt(ks) == ((msgs & 1) & (msgs >> 1))).all()
    assert (either.decrypt(ks) == ((msgs & 1) ^ (msgs >> 1))).all()
    for x in (a, lo, hi, both, either, mo):
        x.close()


def test_full_adder_on_half_torus_operands_from_one_rotation(api, sets, oracle):
    """256 cases of fresh operands at {0, 1/8}: t = a + b + c + 1/16 lies at the centre of sector a + b + c of four; sum
    and carry at {0, 1/8} come from one rotation.  One layer on fresh inputs: every case must decode right."""
    from test_gpu_noise import SETS, predicted_variance
    pp, ks, oks = sets("P128")
    _, typ, _ = predicted_variance(pp, SETS[0][1], SETS[0][2])
    G = 256
    bits = np.random.default_rng(13).integers(0, 2, (3, G))
    bits[:, :8] = [[0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 0, 0, 1, 1], [0, 1, 0, 1, 0, 1, 0, 1]]     # every row of the truth table
    mo = api.LutMulti.from_tables(pp, 1 << 29, [[0, 1, 0, 1], [0, 0, 1, 1]])
    before = api.stats()
    with deferred(api):
        ops = [api.CiphertextArray(pp, G).set_words(fresh_at(oracle, oks, bits[i].astype(np.int64) << 29, 3000 + i)) for i in range(3)]
        s, cy = api.CiphertextArray(pp, G), api.CiphertextArray(pp, G)
        api.lut_bootstrap_multi_batch(mo, [s, cy], ops, [1, 1, 1], 1 << 28, ks)
        assert api.flush() == 1
    d = delta(api, before)
    assert d["multi_rotations"] == G == d["blind_rotates"] and d["keyswitches"] == 2 * G
    total = bits.sum(axis=0)
    key = ks.lwe_key()
    print("\nfull adder on half-torus operands, 256 cases, one rotation each:")
    smallest = 1.0
    for name, arr, bit, taps in (("sum", s, total & 1, mo.outputs()[0][0]), ("carry", cy, total >> 1, mo.outputs()[1][0])):
        ph = signed(T.phases(arr.words(), key))
        assert (np.round(ph * 8).astype(int) == bit).all(), name
        err = ph - bit / 8
        smallest = min(smallest, float((1 / 16 - np.abs(err)).min()))
        noise_report(name, err, [w for _, w in taps], typ)
    print(f"  smallest distance from a decision boundary (1/16 either side of 0 and 1/8): {smallest:.4f}")
    for x in ops + [s, cy, mo]:
        x.close()
