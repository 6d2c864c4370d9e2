"""Multi-key flushes (tuning "batch_keys"): gates recorded under different cloud keys of one parameter set run as ONE
level sequence, each blind rotation and key switch under its own gate's key.  Every result is compared word for word with
the oracle or with the same circuit run alone under its key (batch_keys 0)."""
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = ["NAND", "OR", "AND", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
SEEDS = (0x5EBA2, 0x4B1, 0x4B2)          # the session key (conftest.py) and two more clients


def golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def three_keys(p128_keys, oracle):
    """Three P128 clients: (device keyset, oracle keyset) each; client 0 is the session keyset."""
    from peba1_amd import api
    pp, ks, oks = p128_keys
    own = [api.SecretKeySet(pp, s, device=True) for s in SEEDS[1:]]
    yield pp, [ks] + own, [oks] + [oracle.KeySet(oracle.params("P128"), s) for s in SEEDS[1:]]
    for k in own:
        k.close()


@pytest.fixture
def batching():
    from peba1_amd import api
    api.set_deferred(True)
    assert api.set_tuning("batch_keys", 1) is None
    yield
    api.set_tuning("batch_keys", 0)
    api.set_tuning("fold_constants", 0)
    api.set_tuning("reuse_gates", 1)
    api.set_deferred(False)


def test_three_keys_record_into_one_flush(three_keys, batching):
    from peba1_amd import api, lib
    pp, keys, _ = three_keys
    lib.load().tfhe_hip_set_encrypt_seed(31)
    xs = [api.CiphertextArray(pp, 2).encrypt([1, 0], k) for k in keys]
    rs = [api.CiphertextArray(pp, 1) for _ in keys]
    api.flush()
    before = api.stats()["flushes"]
    for x, r, k in zip(xs, rs, keys):
        lib.load().bootsOR(r.at(0), x.at(0), x.at(1), k.cloud)
    api.flush()
    assert api.stats()["flushes"] == before + 1
    assert api.last_flush_keys() == 3
    assert [int(r.decrypt(k)[0]) for r, k in zip(rs, keys)] == [1, 1, 1]


def _function_f_inputs(pp, g, key, circuits):
    if isinstance(g["template"], str):                   # (37 i + 11) % 255, probe = template + 1
        template = [(37 * i + 11) % 255 for i in range(g["nslots"])]
        probe = [t + 1 for t in template]
    else:
        template, probe = g["template"], g["probe"]
    T, S = [], []
    for t, s in zip(template, probe):                    # encryption order is part of the fixture
        T.append(circuits.encrypt_number(pp, t, g["bits"], key))
        S.append(circuits.encrypt_number(pp, s, g["bits"], key))
    bound = g["bounds"][0] if "bounds" in g else g["bound"]
    return SimpleNamespace(slots=S), SimpleNamespace(slots=T), circuits.encrypt_number(pp, bound, 3 * g["bits"], key)


@pytest.mark.parametrize("fixture", ["function_f_digest.json", "hamming16_digest.json", "function_f_2_folded_digest.json"])
def test_clients_in_one_flush_reproduce_their_solo_words(three_keys, batching, fixture):
    """Three clients recorded back to back under three keys: one flush of the levels of one client alone; client 0
    (the fixture's key and encryption seed) reproduces the oracle's digest, clients 1 and 2 their own solo words."""
    from peba1_amd import api, circuits, lib
    pp, keys, _ = three_keys
    g = golden(fixture)
    assert g["key_seed"] == SEEDS[0]
    L = lib.load()
    hamming = "nbits" in g
    folded = g.get("constant_folding", False)
    if folded:
        api.set_tuning("fold_constants", 1)
        api.set_tuning("reuse_gates", 0)                 # as the folded fixture was made
    L.tfhe_hip_set_encrypt_seed(g["encrypt_seed"])
    if hamming:
        width = g["count_bits"]
        ins = []
        for k in keys:
            a = circuits.encrypt_number(pp, g["a"], g["nbits"], k)
            b = circuits.encrypt_number(pp, g["b"], g["nbits"], k)
            ins.append((a, b, circuits.encrypt_number(pp, g["runs"][0]["bound"], width, k)))
        want = g["runs"][0]["result_b_sha256"], None
    else:
        width = 3 * g["bits"]
        ins = [_function_f_inputs(pp, g, k, circuits) for k in keys]
        run = g["runs"][0] if "runs" in g else g
        want = run["result_b_sha256"], run["result_b0_sha256"]

    def record(c, rb):
        if hamming:
            circuits.hamming_match(rb, ins[c][0], ins[c][1], g["nbits"], ins[c][2], keys[c])
        else:
            circuits.function_f(rb, ins[c][0], ins[c][1], ins[c][2], g["bits"], keys[c])

    api.flush()
    rbs = [api.CiphertextArray(pp, width) for _ in keys]
    s0 = api.stats()
    for c in range(3):
        record(c, rbs[c])
    api.flush()
    s1 = api.stats()
    assert s1["flushes"] == s0["flushes"] + 1 and api.last_flush_keys() == 3
    batched = [rb.words() for rb in rbs]
    assert hashlib.sha256(batched[0].tobytes()).hexdigest() == want[0]
    if want[1]:
        assert hashlib.sha256(batched[0][0].tobytes()).hexdigest() == want[1]
    api.set_tuning("batch_keys", 0)
    solo_levels = []
    for c in range(3):
        rb = api.CiphertextArray(pp, width)
        before = api.stats()["levels"]
        record(c, rb)
        api.flush()
        solo_levels.append(api.stats()["levels"] - before)
        assert api.last_flush_keys() == 1
        assert np.array_equal(rb.words(), batched[c]), c
    assert s1["levels"] - s0["levels"] == max(solo_levels)


def test_every_gate_interleaved_over_three_keys(three_keys, batching):
    from peba1_amd import api, lib
    pp, keys, okeys = three_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(4242)
    rng = np.random.default_rng(7)
    n = 2
    ops = [(g, c) for g in GATES + ["MUX", "NOT"] for c in range(3)]
    ins = {}
    for c, k in enumerate(keys):
        ins[c] = [api.CiphertextArray(pp, n).encrypt(list(rng.integers(0, 2, n)), k) for _ in range(3)]
    words = {c: [a.words() for a in ins[c]] for c in range(3)}
    api.flush()
    res = {}
    for i in range(n):                                   # gate by gate, the key changing at every call
        for g, c in ops:
            r = res.setdefault((g, c), api.CiphertextArray(pp, n))
            a, b, d = (x.at(i) for x in ins[c])
            if g == "MUX":
                L.bootsMUX(r.at(i), a, b, d, keys[c].cloud)
            elif g == "NOT":
                L.bootsNOT(r.at(i), a, keys[c].cloud)
            else:
                getattr(L, "boots" + g)(r.at(i), a, b, keys[c].cloud)
    before = api.stats()["flushes"]
    api.flush()
    assert api.stats()["flushes"] == before + 1 and api.last_flush_keys() == 3
    for (g, c), r in res.items():
        got, (wa, wb, wd), ok = r.words(), words[c], okeys[c]
        for i in range(n):
            want = ok.mux(wa[i], wb[i], wd[i]) if g == "MUX" else ok.gate_not(wa[i]) if g == "NOT" else ok.gate(g, wa[i], wb[i])
            assert (got[i] == want).all(), (g, c, i)


def test_reuse_index_keeps_keys_apart(three_keys, batching):
    """The same gate on the same operand slots under two keys is two gates: a shared input sample and a shared
    bootsCONSTANT, with reuse_gates on."""
    from peba1_amd import api, lib
    pp, keys, okeys = three_keys
    L = lib.load()
    api.set_tuning("reuse_gates", 1)
    L.tfhe_hip_set_encrypt_seed(99)
    x = api.CiphertextArray(pp, 1).encrypt([1], keys[0])
    one = api.CiphertextArray(pp, 1)
    L.bootsCONSTANT(one.at(0), 1, keys[0].cloud)
    r = [api.CiphertextArray(pp, 2) for _ in range(2)]
    for c in range(2):
        L.bootsAND(r[c].at(0), x.at(0), one.at(0), keys[c].cloud)
        L.bootsXOR(r[c].at(1), x.at(0), x.at(0), keys[c].cloud)
    api.flush()
    wx, w1 = x.words()[0], okeys[0].constant(1)
    got = [q.words() for q in r]
    assert not np.array_equal(got[0][0], got[1][0]) and not np.array_equal(got[0][1], got[1][1])
    for c in range(2):
        assert (got[c][0] == okeys[c].gate("AND", wx, w1)).all(), c
        assert (got[c][1] == okeys[c].gate("XOR", wx, wx)).all(), c


def test_other_parameter_set_flushes_and_deleted_key_runs_first(three_keys, batching, oracle):
    from peba1_amd import api, lib
    pp, keys, okeys = three_keys
    L = lib.load()
    p80 = api.ParameterSet(80)
    k80 = api.SecretKeySet(p80, 0x80, device=True)
    o80 = oracle.KeySet(oracle.params("P80"), 0x80)
    try:
        L.tfhe_hip_set_encrypt_seed(5)
        a128 = api.CiphertextArray(pp, 2).encrypt([1, 0], keys[0])
        a80 = api.CiphertextArray(p80, 2).encrypt([1, 1], k80)
        r128, r80 = api.CiphertextArray(pp, 1), api.CiphertextArray(p80, 1)
        api.flush()
        before = api.stats()["flushes"]
        L.bootsXOR(r128.at(0), a128.at(0), a128.at(1), keys[0].cloud)
        L.bootsAND(r80.at(0), a80.at(0), a80.at(1), k80.cloud)
        api.flush()
        assert api.stats()["flushes"] == before + 2
        w128, w80 = a128.words(), a80.words()
        assert (r128.words()[0] == okeys[0].gate("XOR", w128[0], w128[1])).all()
        assert (r80.words()[0] == o80.gate("AND", w80[0], w80[1])).all()
    finally:
        k80.close()
    # a key deleted while its gates are pending: the whole recording runs first, the other key's results are exact
    tmp = api.SecretKeySet(pp, 0x4B3, device=True)
    L.tfhe_hip_set_encrypt_seed(6)
    b0 = api.CiphertextArray(pp, 2).encrypt([0, 1], keys[0])
    bt = api.CiphertextArray(pp, 2).encrypt([1, 1], tmp)
    r0, rt = api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 1)
    api.flush()
    L.bootsOR(r0.at(0), b0.at(0), b0.at(1), keys[0].cloud)
    L.bootsNAND(rt.at(0), bt.at(0), bt.at(1), tmp.cloud)
    tmp.close()
    wb = b0.words()
    assert (r0.words()[0] == okeys[0].gate("OR", wb[0], wb[1])).all()


def test_multikey_levels_use_both_wide_and_narrow_forms(three_keys, batching):
    """A level wider than two rounds of the chip (the 4-wave form and its 8-wave tail) and narrow levels (the 8-wave
    form), each rotation under its own key."""
    from peba1_amd import api, lib
    pp, keys, okeys = three_keys
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(77)
    width = 185                                          # 3 x 185 = 555 rotations: one round of 2 x 256 CUs + a tail
    ins = [(api.CiphertextArray(pp, width).encrypt([i & 1 for i in range(width)], k),
            api.CiphertextArray(pp, width).encrypt([(i >> 1) & 1 for i in range(width)], k)) for k in keys]
    api.flush()
    api.reset_stats()
    outs = []
    for (a, b), k in zip(ins, keys):
        r = api.CiphertextArray(pp, width)
        for i in range(width):
            L.bootsXOR(r.at(i), a.at(i), b.at(i), k.cloud)
        s = api.CiphertextArray(pp, 1)
        L.bootsAND(s.at(0), r.at(0), r.at(1), k.cloud)   # a narrow second level
        outs.append((r, s))
    api.flush()
    st = api.stats()
    assert st["flushes"] == 1 and api.last_flush_keys() == 3
    assert st["br8_launches"] > 0 and st["br_launches"] > st["br8_launches"]
    for c, ((a, b), (r, s)) in enumerate(zip(ins, outs)):
        wa, wb, wr = a.words(), b.words(), r.words()
        for i in (0, 1, width // 2, width - 1):
            assert (wr[i] == okeys[c].gate("XOR", wa[i], wb[i])).all(), (c, i)
        assert (s.words()[0] == okeys[c].gate("AND", wr[0], wr[1])).all(), c
