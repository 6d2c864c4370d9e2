"""GPU tests of the programmable bootstrap (tfhe_hip_lut_bootstrap): word for word against the committed digests of the
oracle restatement (tests/golden/lut_bootstrap_digests.json, tests/lut_common.py) through the recorded path and, through
the raw entry, in every blind-rotate kernel form; against the gates with the gate polynomial; multi-key flushes; the LUT
table's growth and reuse; a chain of 2-bit re-encodings; output noise.  No oracle bootstrap runs here: inputs are
oracle ENCRYPTIONS (cheap) from the fixture's seeds."""
import contextlib

import numpy as np
import pytest

import lut_common as T

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
            made[pname] = (pp, api.SecretKeySet(pp, T.KEY_SEED, device=True), oracle.KeySet(oracle.params(pname), T.KEY_SEED))
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


def record_case(api, pp, ks, O, oks, case, keep):
    """Records one fixture case; returns the result array (inputs and LUT are kept alive in `keep`)."""
    inputs = api.CiphertextArray(pp, len(case["coefs"])).set_words(T.case_inputs(O, oks, case))
    lut = api.Lut(pp, T.lut_words(case["lut"], pp.N))
    r = api.CiphertextArray(pp, 1)
    _clear_error()
    api.lut_bootstrap(lut, r.at(0), [inputs.at(i) for i in range(inputs.count)], case["coefs"], case["c0"], ks)
    assert api.last_error() == ""
    keep += [inputs, lut]
    return r


def check_case(words, case):
    assert [int(x) for x in words[:4]] == case["first_words"], (case["parameter_set"], case["index"])
    assert T.sha256_words(words) == case["sha256"], (case["parameter_set"], case["index"])


def test_constant_lut_at_one_eighth_reproduces_the_gates(api, sets):
    pp, ks, _ = sets("P128")
    mu = 1 << 29
    from peba1_amd import lib
    lib.load().tfhe_hip_set_encrypt_seed(77)
    bits = np.array([[0, 0, 1, 1, 0, 1, 0, 1], [0, 1, 0, 1, 1, 1, 0, 0], [1, 0, 0, 1, 1, 0, 1, 0]])
    a, b, c = (api.CiphertextArray(pp, 8).encrypt(bits[i], ks) for i in range(3))
    lut = api.Lut.constant(pp, mu)
    with deferred(api):
        for name, coefs, c0 in (("AND", [1, 1], -mu), ("XOR", [2, 2], 2 * mu), ("NAND", [-1, -1], mu)):
            want, got = api.CiphertextArray(pp, 8), api.CiphertextArray(pp, 8)
            api.gate_batch(name, want, a, b, ks)
            api.lut_bootstrap_batch(lut, got, [a, b], coefs, c0, ks)
            assert (got.words() == want.words()).all(), name
        for name, s in (("MAJ3", 1), ("XOR3", -2)):
            want, got = api.CiphertextArray(pp, 8), api.CiphertextArray(pp, 8)
            api.gate3_batch(name, want, a, b, c, ks)
            api.lut_bootstrap_batch(lut, got, [a, b, c], [s, s, s], 0, ks)
            assert (got.words() == want.words()).all(), name
    # immediate mode: complete on return, host mirror refreshed
    with deferred(api, False):
        want, got = api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 1)
        lib.load().bootsAND(want.at(0), a.at(3), b.at(3), ks.cloud)
        api.lut_bootstrap(lut, got.at(0), [a.at(3), b.at(3)], [1, 1], -mu, ks)
        n = pp.n
        assert got.ptr.contents.b == want.ptr.contents.b and got.ptr.contents.a[0] == want.ptr.contents.a[0]
        assert got.ptr.contents.a[n - 1] == want.ptr.contents.a[n - 1]
    lut.close()


@pytest.mark.parametrize("pname", list(T.CASES))
def test_every_fixture_case_through_the_recorded_path(api, sets, oracle, pname):
    pp, ks, oks = sets(pname)
    cases = T.load_digests()["sets"][pname]["cases"]
    keep = []
    before = api.stats()
    with deferred(api):
        results = [record_case(api, pp, ks, oracle, oks, c, keep) for c in cases]
        assert api.flush() == 1
    d = delta(api, before)
    assert d["lut_rotations"] == len(cases) == d["blind_rotates"] == d["keyswitches"]
    for r, c in zip(results, cases):
        check_case(r.words()[0], c)
    for x in keep:
        x.close()


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# (parameter set, tunings, rotations or None = one per case, raw accumulators, expected launch counters)
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
    pname, tune, count, want_acc, counters = RAW_ROWS[row]
    pp, ks, oks = sets(pname)
    cases = T.load_digests()["sets"][pname]["cases"]
    polys = np.stack([T.lut_words(c["lut"], pp.N) for c in cases])
    lins = np.stack([T.linear(c["coefs"], T.case_inputs(oracle, oks, c), c["c0"]) for c in cases])
    count = len(cases) if count is None else 2 * cu_count() + 8       # "tail": two full rounds and 8 rotations more
    which = np.arange(count) % len(cases)
    with tunings(api, **tune):
        before = api.stats()
        out = api.kernel_lut_bootstrap_woks(ks, lins[which], which.astype(I32), polys, want_acc=want_acc)
        d = delta(api, before)
    for k, v in counters.items():
        assert d[k] == v, (row, k, d[k])
    assert d["lut_rotations"] == count
    u, acc = out if want_acc else (out, None)
    for i, ci in enumerate(which):
        assert T.sha256_words(u[i]) == cases[ci]["sha256_extracted"], (row, i)
        if want_acc:
            assert T.sha256_words(acc[i]) == cases[ci]["sha256_accumulator"], (row, i)
    # an index below zero is the constant test vector of every gate; key switch of the extracted samples = the recorded words
    mixed = np.where(np.arange(len(cases)) % 2 == 0, -1, np.arange(len(cases))).astype(I32)
    with tunings(api, **tune):
        u2 = api.kernel_lut_bootstrap_woks(ks, lins, mixed, polys)
        plain = api.kernel_bootstrap_woks(ks, lins)
    assert (u2[0::2] == plain[0::2]).all()
    ct = api.kernel_keyswitch(ks, u2[1::2])
    for w, c in zip(ct, cases[1::2]):
        check_case(w, c)


def test_three_key_flush_mixing_lut_ops_gates_and_a_mux(api, sets, oracle):
    """One level under three cloud keys of one set (batch_keys): LUT ops against their fixture digests under the
    fixture's key, two-input gates and a MUX under two other keys against the oracle's words."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = sets("P128")
    cases = T.load_digests()["sets"]["P128"]["cases"][:8]
    others = [(api.SecretKeySet(pp, s, device=True), oracle.KeySet(oracle.params("P128"), s)) for s in (21, 22)]
    keep = []
    was = L.tfhe_hip_set_batch_keys(1)
    try:
        with deferred(api):
            before = api.stats()
            lut_results, gate_results = [], []
            for i, c in enumerate(cases):
                lut_results.append(record_case(api, pp, ks, oracle, oks, c, keep))
                k2, o2 = others[i % 2]
                w = o2.encrypt(oracle.Rng(600 + i), [i & 1, (i >> 1) & 1, 1])
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
            assert api.flush() == 1
            d = delta(api, before)
        assert api.last_flush_keys() == 3
        assert d["lut_rotations"] == 8 and d["blind_rotates"] == 8 + 8 + 1 and d["keyswitches"] == 16
        for r, c in zip(lut_results, cases):
            check_case(r.words()[0], c)
        for i, (r, want) in enumerate(gate_results):
            assert (r.words()[0] == want).all(), i
    finally:
        L.tfhe_hip_set_batch_keys(was)
        for x in keep:
            x.close()
        for k2, o2 in others:
            k2.close()
            o2.close()


def test_lut_table_grows_and_entries_are_reused_between_flushes(api, sets, oracle):
    pp, ks, oks = sets("P128")
    cases = T.load_digests()["sets"]["P128"]["cases"]
    c0, c1 = cases[6], cases[9]
    keep = []
    with deferred(api):
        first = record_case(api, pp, ks, oracle, oks, c0, keep)
        api.flush()
        check_case(first.words()[0], c0)
        # 40 more LUTs, each used once: the device table (16 entries at first) doubles twice between the flushes
        fill = [api.Lut.constant(pp, ((i % 4) << 30) + (1 << 29)) for i in range(40)]
        a = api.CiphertextArray(pp, 1).encrypt([1], ks)
        outs = api.CiphertextArray(pp, 40)
        for i, lut in enumerate(fill):
            api.lut_bootstrap(lut, outs.at(i), [a.at(0)], [1], 0, ks)
        again = record_case(api, pp, ks, oracle, oks, c0, keep)
        api.flush()
        check_case(again.words()[0], c0)
        ph = T.phases(outs.words(), ks.lwe_key())
        want = (np.arange(40) % 4) / 4 + 1 / 8
        assert np.abs((ph - want + 0.5) % 1 - 0.5).max() < 0.03          # each op read its own polynomial (a neighbour's: 1/4 off)
        # a LUT deleted with an op pending: the recording runs first; its entry then serves the next LUT
        pending = record_case(api, pp, ks, oracle, oks, c1, keep)
        before = api.stats()
        keep.pop().close()
        assert delta(api, before)["flushes"] == 1
        check_case(pending.words()[0], c1)
        for lut in fill[:20]:
            lut.close()
        later = record_case(api, pp, ks, oracle, oks, c1, keep)
        api.flush()
        check_case(later.words()[0], c1)
        check_case(first.words()[0], c0)
    for x in keep + fill[20:]:
        x.close()


def test_two_bit_chain_word_for_word_and_at_decrypt_level(api, sets, oracle):
    pp, ks, oks = sets("P128")
    ch = T.load_digests()["chain"]
    perms = ch["perms"]
    assert perms == T.chain_perms(ch["hops"])
    luts = [api.Lut(pp, T.chain_lut(p, pp.N)) for p in perms]
    msgs = [i % 4 for i in range(ch["messages"])]
    with deferred(api):
        cur = api.CiphertextArray(pp, len(msgs)).set_words(T.encode_messages(oracle, oks, msgs, ch["enc_seed"]))
        for h, lut in enumerate(luts):
            nxt = api.CiphertextArray(pp, len(msgs))
            api.lut_bootstrap_batch(lut, nxt, [cur], [1], 0, ks)
            assert [T.sha256_words(w) for w in nxt.words()] == ch["hops_out"][h]["sha256"], h
            cur = nxt
        # 256 messages x 8 hops, recorded as one flush of depth 8: no wrong result allowed
        rng = np.random.default_rng(5)
        perms8 = [rng.permutation(4).tolist() for _ in range(8)]
        luts8 = [api.Lut.from_table(pp, np.array([T.centre(m) for m in p], dtype=np.int64).astype(I32)) for p in perms8]
        msgs = rng.integers(0, 4, 256)
        cur = api.CiphertextArray(pp, 256).set_words(T.encode_messages(oracle, oks, msgs, 31337))
        stages = []
        for lut in luts8:
            nxt = api.CiphertextArray(pp, 256)
            api.lut_bootstrap_batch(lut, nxt, [cur], [1], 0, ks)
            stages.append(nxt)
            cur = nxt
        assert api.flush() == 8
        key = ks.lwe_key()
        smallest = 1.0
        for p, arr in zip(perms8, stages):
            msgs = np.array(p)[msgs]
            ph = T.phases(arr.words(), key)
            assert (T.decode(ph) == msgs).all()
            smallest = min(smallest, float(T.edge_distance(ph).min()))
        print(f"\n2-bit chain: 256 messages x 8 hops, smallest distance from a sector edge {smallest:.4f}")
    for lut in luts + luts8:
        lut.close()


def test_identity_table_output_noise_is_the_gates(api, sets, oracle):
    """1,024 bootstraps of the 4-sector identity table on fresh 2-bit messages: the output phase error is judged by the
    band tests/test_gpu_noise.py uses for gates (the external product's noise does not depend on the test polynomial)."""
    from test_gpu_noise import SETS, ksk_mean_shift, predicted_variance
    pp, ks, oks = sets("P128")
    _, ks_stdev, bk_stdev = SETS[0]
    worst, typ, kb = predicted_variance(pp, ks_stdev, bk_stdev)
    shift = ksk_mean_shift(ks, pp)
    G = 1024
    msgs = np.random.default_rng(8).integers(0, 4, G)
    lut = api.Lut.from_table(pp, np.array([T.centre(m) for m in range(4)], dtype=np.int64).astype(I32))
    with deferred(api):
        a = api.CiphertextArray(pp, G).set_words(T.encode_messages(oracle, oks, msgs, 4711))
        r = api.CiphertextArray(pp, G)
        api.lut_bootstrap_batch(lut, r, [a], [1], 0, ks)
        api.flush()
    ideal = np.array([T.centre(m) for m in msgs]) / 2.0 ** 32
    e = (T.phases(r.words(), ks.lwe_key()) - ideal + 0.5) % 1 - 0.5
    sem = np.sqrt(e.var() / e.size)
    print(f"\nidentity LUT: {G} bootstraps  mean {e.mean():+.3e} (KSK constant {shift:+.3e}, sem {sem:.1e})  var {e.var():.3e}  "
          f"predicted typical {typ:.3e}  worst-case bound {worst:.3e}  max |e| {np.abs(e).max():.4f}")
    assert np.abs(e).max() < 6.5 * np.sqrt(typ)
    assert abs(e.mean() - shift) < 6 * sem + 4 * kb
    assert e.var() < worst and 0.7 * typ < e.var() < 1.4 * typ
    lut.close()
