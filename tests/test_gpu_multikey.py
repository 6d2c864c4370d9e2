"""Multi-key flushes (tuning "batch_keys"): gates recorded under different cloud keys of one parameter set run as ONE
level sequence, each blind rotation and key switch under its own gate's key.  Every result is compared word for word with
the oracle or with the same circuit run alone under its key (batch_keys 0)."""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = ["NAND", "OR", "AND", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
SEEDS = (0x5EBA2, 0x4B1, 0x4B2)          # the session key (conftest.py) and two more clients


def _oracle_map(fn, items):
    """fn over the items on at most 16 host threads (ctypes releases the GIL; the oracle is re-entrant)"""
    with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as ex:
        return list(ex.map(fn, items))


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
        want = _oracle_map(lambda i: okeys[c].gate("XOR", wa[i], wb[i]), range(width))     # every row
        bad = [i for i in range(width) if not (wr[i] == want[i]).all()]
        assert not bad, (c, bad[:8])
        assert (s.words()[0] == okeys[c].gate("AND", wr[0], wr[1])).all(), c


# ---------------------------------------------------------------- every launch form of a multi-key flush, every word
#
# A circuit here is a list of gates (client, kind, operand references); a reference is ("x", j) = bit j of the client's
# encrypted inputs or ("g", i) = the result of gate i.  Gate i's result is sample i of one result array.  The reference is
# the oracle's gate / mux under the gate's own client key (exact product over one 64-bit prime), level by level; a gate of
# level 2 or 3 takes the oracle's words of the level before as inputs, which ARE the GPU's words of that level once that
# level has been compared (the comparison runs in level order and stops at the first level that differs).

TUNING_DEFAULTS = {"br_tail8": 1, "br_variant": -1, "br_digit_table": 1, "br8_max_rotations": 1 << 30, "balance_levels": 1}
KINDS = ["XOR", "NAND", "ANDNY", "ORYN", "AND", "NOR"]


def restore_tunings():
    from peba1_amd import api
    for name, value in TUNING_DEFAULTS.items():
        api.set_tuning(name, value)


def gate_levels(gates):
    lv = []
    for c, kind, refs in gates:
        lv.append(1 + max([lv[r[1]] for r in refs if r[0] == "g"], default=0))
    return lv


def record_and_flush(pp, keys, ins, gates):
    """Records the gates one call at a time under each gate's client key, flushes, returns the result array."""
    from peba1_amd import api, lib
    L = lib.load()
    res = api.CiphertextArray(pp, len(gates))
    for g, (c, kind, refs) in enumerate(gates):
        ops = [ins[c].at(r[1]) if r[0] == "x" else res.at(r[1]) for r in refs]
        if kind == "MUX":
            L.bootsMUX(res.at(g), ops[0], ops[1], ops[2], keys[c].cloud)
        else:
            getattr(L, "boots" + kind)(res.at(g), ops[0], ops[1], keys[c].cloud)
    assert api.flush() >= 0, api.last_error()
    return res


def oracle_words(okeys, in_words, gates):
    """The oracle's words of every gate, level by level."""
    lv = gate_levels(gates)
    want = [None] * len(gates)

    def one(g):
        c, kind, refs = gates[g]
        ops = [in_words[c][r[1]] if r[0] == "x" else want[r[1]] for r in refs]
        return okeys[c].mux(*ops) if kind == "MUX" else okeys[c].gate(kind, ops[0], ops[1])

    for level in range(1, max(lv) + 1):
        idx = [g for g in range(len(gates)) if lv[g] == level]
        for g, w in zip(idx, _oracle_map(one, idx)):
            want[g] = w
    return np.stack(want)


def assert_words(got, want, gates, label):
    lv = gate_levels(gates)
    for level in range(1, max(lv) + 1):                    # in level order: see the note above
        bad = [(g, gates[g][0], gates[g][1]) for g in range(len(gates)) if lv[g] == level and not (got[g] == want[g]).all()]
        assert not bad, f"{label}: {len(bad)} gates of level {level} differ from the oracle; first (gate, client, kind): {bad[:8]}"


def three_level_circuit(widths):
    """Level 1: widths[c] gates of client c (six two-input kinds in turn, the last gate of every client a MUX), recorded
    interleaved so that the key changes from call to call; level 2: 5, 0 and 2 gates on level-1 results; level 3: one gate
    of client 0.  Client c has 2 widths[c] + 1 input bits."""
    gates, first = [], {}
    order = sorted((i / w, c, i) for c, w in enumerate(widths) for i in range(w))
    for _, c, i in order:
        w = widths[c]
        first[(c, i)] = len(gates)
        if i == w - 1:
            gates.append((c, "MUX", (("x", i), ("x", w + i), ("x", 2 * w))))
        else:
            gates.append((c, KINDS[(i + c) % len(KINDS)], (("x", i), ("x", w + i))))
    level2 = {}
    for c, j in ((0, 0), (2, 0), (0, 1), (2, 1), (0, 2), (0, 3), (0, 4)):
        level2[(c, j)] = len(gates)
        gates.append((c, KINDS[(j + 2 * c + 1) % len(KINDS)], (("g", first[(c, j)]), ("g", first[(c, j + 1)]))))
    gates.append((0, "XOR", (("g", level2[(0, 0)]), ("g", level2[(0, 1)]))))
    lv = gate_levels(gates)
    assert [lv.count(x) for x in (1, 2, 3)] == [sum(widths), 7, 1] and max(lv) == 3
    assert sum(1 for g in gates if g[1] == "MUX") == 3 and len({g[1] for g in gates}) >= 5
    return gates


WIDTHS = {"P128": (230, 185, 140), "P80": (230, 185, 140), "P2048": (64, 40, 24)}
SET_SEEDS = {"P80": (0x80, 0x81, 0x82), "P2048": (0x2048, 0x2049, 0x204A)}


@pytest.fixture(scope="module")
def wide_cases(three_keys, oracle):
    """Per parameter set, made on first use and kept for the module: three client keys, their encrypted inputs (the same
    words in every tuning row), the circuit, the oracle's words of every gate (computed once) and the words of the first
    row that ran (every other row must reproduce them)."""
    from peba1_amd import api, lib
    made, own = {}, []

    def get(pname):
        if pname in made:
            return made[pname]
        if pname == "P128":
            pp, keys, okeys = three_keys
        else:
            pp = api.ParameterSet(80) if pname == "P80" else api.ParameterSet(p2048=True)
            keys = [api.SecretKeySet(pp, s, device=True) for s in SET_SEEDS[pname]]
            own.extend(keys)
            okeys = [oracle.KeySet(oracle.params(pname), s) for s in SET_SEEDS[pname]]
        widths = WIDTHS[pname]
        rng = np.random.default_rng(pp.n + 3)
        lib.load().tfhe_hip_set_encrypt_seed(0x3A + pp.n)
        ins = [api.CiphertextArray(pp, 2 * w + 1).encrypt(list(rng.integers(0, 2, 2 * w + 1)), k) for w, k in zip(widths, keys)]
        gates = three_level_circuit(widths)
        case = SimpleNamespace(pp=pp, keys=keys, okeys=okeys, ins=ins, gates=gates, widths=widths, first=None,
                               in_words=[a.words() for a in ins], want=None)
        made[pname] = case
        return case
    yield get
    for k in own:
        k.close()


def run_wide_row(case, tunings, label):
    """One flush of the three-level circuit under `tunings`; returns (result words, counter deltas).  Asserts one flush
    of three keys with the level widths of three_level_circuit, every word equal to the oracle's and to the first row's."""
    from peba1_amd import api
    if case.want is None:
        case.want = oracle_words(case.okeys, case.in_words, case.gates)
    api.flush()
    try:
        api.set_tuning("balance_levels", 0)              # ASAP levels: the widths are the circuit's
        for name, value in tunings.items():
            api.set_tuning(name, value)
        s0 = api.stats()
        res = record_and_flush(case.pp, case.keys, case.ins, case.gates)
        s1 = api.stats()
    finally:
        restore_tunings()
    d = {k: s1[k] - s0[k] for k in s0}
    assert d["flushes"] == 1 and api.last_flush_keys() == 3, label
    w = sum(case.widths)
    # three levels of w + 3 (one MUX per key), 7 and 1 rotations; w, 7 and 1 key switches
    assert (d["levels"], d["blind_rotates"], d["keyswitches"]) == (3, w + 3 + 7 + 1, w + 7 + 1), label
    got = res.words()
    assert_words(got, case.want, case.gates, label)
    if case.first is None:
        case.first = got
    assert np.array_equal(got, case.first), label
    return got, d


# (set, tunings, expected rise of br8_launches, br_launches, br8_rotations) with 256 CUs (the same rows as plans of
# launch_plan.hpp, without a GPU: tests/test_launch_plan_cpu.py):
#   4- / 8-wave multi-key kernels (N = 1024): level 1 = 558 rotations = one round of 512 on the 4-wave kernel + a tail of
#   46 on the 8-wave kernel (two launches, one of them 8-wave), levels 2 and 3 (7 and 1 rotations) one 8-wave launch each;
#   per-key fallback (split and 2-wave forms, all of N = 2048): one single-key launch per key with a share of the level:
#   3 + 2 + 1 launches, none of them 8-wave.
WIDE_ROWS = [
    ("P128", {}, 3, 4, 54), ("P80", {}, 3, 4, 54),
    ("P128", {"br_tail8": 0}, 2, 3, 8), ("P80", {"br_tail8": 0}, 2, 3, 8),          # level 1 as one 4-wave launch
    ("P128", {"br_digit_table": 0}, 3, 4, 54),                                        # both kernels without digit tables
    ("P128", {"br8_max_rotations": 0}, 0, 3, 0), ("P80", {"br8_max_rotations": 0}, 0, 3, 0),   # narrow levels on the 4-wave kernel
    ("P128", {"br_variant": 2}, 0, 6, 0), ("P80", {"br_variant": 2}, 0, 6, 0),       # per-key split launches
    ("P128", {"br_variant": 4}, 0, 6, 0), ("P80", {"br_variant": 4}, 0, 6, 0),       # per-key 2-wave launches
    ("P2048", {}, 0, 6, 0), ("P2048", {"br_digit_table": 0}, 0, 6, 0), ("P2048", {"br_digit_table": 2}, 0, 6, 0),
]


@pytest.mark.parametrize("pname,tunings,br8,br,rot8", WIDE_ROWS,
                         ids=[p + "-" + ("-".join(f"{k}={v}" for k, v in t.items()) or "defaults") for p, t, *_ in WIDE_ROWS])
def test_multikey_flush_every_word_in_every_launch_form(wide_cases, batching, pname, tunings, br8, br, rot8):
    """One flush of three keys with unequal shares (230 / 185 / 140 gates and a MUX each on level 1: both key boundaries
    inside the first round of 512 workgroups, the tail of 46 wholly under the last key; then 5 / 0 / 2 gates; then one
    gate of the first key alone), EVERY result word against the oracle, in every launch form a multi-key level can take.
    The counters the engine keeps show that the row reached its path (WIDE_ROWS)."""
    case = wide_cases(pname)
    label = f"{pname} {tunings or 'defaults'}"
    _, d = run_wide_row(case, tunings, label)
    assert (d["br8_launches"], d["br_launches"], d["br8_rotations"]) == (br8, br, rot8), (label, d)


def test_multikey_flush_with_kernel_timing_on(wide_cases, batching):
    """The default row at P128 with kernel timing on: the multi-key kernels add to the device clock sums and the tail launch
    records an event between the two launches of level 1.  Same words; the times only have to have been taken."""
    from peba1_amd import lib
    case = wide_cases("P128")
    L = lib.load()
    L.tfhe_hip_set_kernel_timing(1)
    try:
        _, d = run_wide_row(case, {}, "P128 defaults, kernel timing on")
    finally:
        L.tfhe_hip_set_kernel_timing(0)
    assert (d["br8_launches"], d["br_launches"], d["br8_rotations"]) == (3, 4, 54), d
    assert d["ms_blind_rotate"] > 0 and d["ms_keyswitch"] > 0 and d["ms_blind_rotate8"] > 0, d
    assert d["ms_blind_rotate8"] <= d["ms_blind_rotate"], d
    assert d["clk_shader_cycles"] > 0, d


def custom_set(oracle, N, l, Bgbit, ks_t=8, n=24):
    """(product parameter set, oracle parameter set) of a small custom shape: a short blind rotation, the full ring"""
    from peba1_amd import api
    return (api.ParameterSet(custom=(n, N, 1, l, Bgbit, ks_t, 2, 2.0 ** -15, 2.0 ** -25, 0.012467)),
            oracle.custom_params(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=ks_t, ks_basebit=2))


def sixteen_client_circuit(clients):
    """Client c (its position in `clients` decides the recording order and so its place in the key table): c + 1 gates on
    level 1, interleaved over the clients; even clients one more gate on level 2."""
    gates, first = [], {}
    for i in range(16):
        for c in clients:
            if i <= c:
                first[(c, i)] = len(gates)
                gates.append((c, KINDS[(i + c) % len(KINDS)], (("x", i), ("x", 16 + i))))
    for c in clients:
        if c % 2 == 0:
            gates.append((c, "NAND" if c % 4 else "XOR", (("g", first[(c, 0)]), ("g", first[(c, c)]))))
    return gates


@pytest.mark.parametrize("l,Bgbit", [(2, 10), (3, 6)], ids=["l2-Bg10-no-table", "l3-Bg6-table"])
def test_sixteen_keys_in_one_flush_and_key_table_rewritten(oracle, batching, l, Bgbit):
    """Sixteen clients' keys in one flush, every word; then three keys, then the sixteen in reverse order: the device key
    table is rewritten for every flush and no entry of an earlier one survives; then the sixteen on the 4-wave kernel.
    (2, 10): digits too wide for the digit table; (3, 6): with it."""
    from peba1_amd import api, lib
    L = lib.load()
    assert L.tfhe_hip_test_form_admissible(0, 1024, l, Bgbit, 1 if Bgbit <= 7 else 0) == 1     # the 4-wave form runs this gadget
    assert L.tfhe_hip_test_form_admissible(2, 1024, l, Bgbit, 1 if Bgbit <= 7 else 0) == 1     # and the 8-wave form
    pp, op = custom_set(oracle, 1024, l, Bgbit)
    seeds = [0x1600 + 16 * l + c for c in range(16)]
    keys = [api.SecretKeySet(pp, s, device=True) for s in seeds]
    okeys = [oracle.KeySet(op, s) for s in seeds]
    try:
        rng = np.random.default_rng(l)
        L.tfhe_hip_set_encrypt_seed(160 + l)
        ins = [api.CiphertextArray(pp, 32).encrypt(list(rng.integers(0, 2, 32)), k) for k in keys]
        in_words = [a.words() for a in ins]
        api.flush()
        want_of = {}
        # (136 and 8 rotations: the 8-wave kernel by default; the last run keeps both levels on the 4-wave kernel)
        for label, clients, nkeys, br8_max in (("sixteen", list(range(16)), 16, 1 << 30), ("three", [5, 9, 2], 3, 1 << 30),
                                               ("sixteen reversed", list(range(15, -1, -1)), 16, 1 << 30),
                                               ("sixteen, 4-wave kernel", list(range(16)), 16, 0)):
            gates = sixteen_client_circuit(clients)
            before = api.stats()
            try:
                api.set_tuning("balance_levels", 0)
                api.set_tuning("br8_max_rotations", br8_max)
                res = record_and_flush(pp, keys, ins, gates)
            finally:
                restore_tunings()
            after = api.stats()
            assert after["flushes"] == before["flushes"] + 1 and api.last_flush_keys() == nkeys, label
            assert after["br8_launches"] - before["br8_launches"] == (2 if br8_max else 0), label
            assert after["levels"] == before["levels"] + 2 and after["keyswitches"] == before["keyswitches"] + len(gates), label
            # a gate's words depend on its client, kind and operands only: computed once, looked up by that
            ident = [(c, kind, refs if refs[0][0] == "x" else tuple(("g",) + gates[r[1]][:3] for r in refs)) for c, kind, refs in gates]
            todo = [g for g, k in enumerate(ident) if k not in want_of]
            if todo:
                full = oracle_words(okeys, in_words, gates)
                for g in todo:
                    want_of[ident[g]] = full[g]
            want = np.stack([want_of[k] for k in ident])
            assert_words(res.words(), want, gates, f"l={l} Bgbit={Bgbit}, {label}")
    finally:
        for k in keys:
            k.close()


def _one_gate_each(pps, keys, okeys, order, seed):
    """One gate under each of the two keys, recorded back to back in `order`; returns (flushes after the second record,
    keys of that flush, flushes after the explicit flush, keys of that one, words equal to the oracle's per key)."""
    from peba1_amd import api, lib
    L = lib.load()
    L.tfhe_hip_set_encrypt_seed(seed)
    ins = [api.CiphertextArray(pps[c], 2).encrypt([1, c], keys[c]) for c in range(2)]
    res = [api.CiphertextArray(pps[c], 1) for c in range(2)]
    words = [a.words() for a in ins]
    api.flush()
    before = api.stats()["flushes"]
    for c in order:
        getattr(L, "boots" + ("XOR", "NAND")[c])(res[c].at(0), ins[c].at(0), ins[c].at(1), keys[c].cloud)
    mid, mid_keys = api.stats()["flushes"] - before, api.last_flush_keys()
    assert api.flush() >= 0, api.last_error()
    end, end_keys = api.stats()["flushes"] - before, api.last_flush_keys()
    exact = [bool((res[c].words()[0] == okeys[c].gate(("XOR", "NAND")[c], words[c][0], words[c][1])).all()) for c in range(2)]
    return mid, mid_keys, end, end_keys, exact


# pairs of sets with equal n = 24 (one slot pool) that differ in what evaluation reads: ring and gadget, gadget alone, the
# key-switch gadget alone -- (N, l, Bgbit, ks_t) each
MIXED_PAIRS = [((1024, 4, 8, 8), (2048, 6, 4, 8)), ((1024, 4, 8, 8), (1024, 8, 4, 8)), ((1024, 4, 8, 8), (1024, 4, 8, 4))]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["first-then-second", "second-then-first"])
@pytest.mark.parametrize("pair", MIXED_PAIRS, ids=["ring-and-gadget", "gadget", "ks_t"])
def test_keys_of_different_sets_with_equal_n_do_not_batch(oracle, batching, pair, order):
    """Two keys whose ciphertexts have the same size (n = 24: one slot pool) but whose parameter sets differ: a flush runs
    every rotation with the parameters of its first key, so such keys never share one -- the second gate's key flushes the
    first gate (one key), the explicit flush runs the second (one key), both results are the oracle's words."""
    from peba1_amd import api
    sets = [custom_set(oracle, *shape) for shape in pair]
    keys = [api.SecretKeySet(pp, 0xD0 + c, device=True) for c, (pp, _) in enumerate(sets)]
    okeys = [oracle.KeySet(op, 0xD0 + c) for c, (_, op) in enumerate(sets)]
    try:
        mid, mid_keys, end, end_keys, exact = _one_gate_each([s[0] for s in sets], keys, okeys, order, 0xD5)
        assert (mid, mid_keys) == (1, 1), "the second key did not flush the first key's gate"
        assert (end, end_keys) == (2, 1)
        assert exact == [True, True]
    finally:
        for k in keys:
            k.close()


def test_equal_sets_allocated_separately_still_batch(oracle, batching):
    """The positive control: two ParameterSet objects with equal numbers are one parameter set -- their keys share a flush."""
    from peba1_amd import api
    sets = [custom_set(oracle, 1024, 4, 8) for _ in range(2)]
    assert sets[0][0].ptr != sets[1][0].ptr
    keys = [api.SecretKeySet(pp, 0xE0 + c, device=True) for c, (pp, _) in enumerate(sets)]
    okeys = [oracle.KeySet(op, 0xE0 + c) for c, (_, op) in enumerate(sets)]
    try:
        mid, _, end, end_keys, exact = _one_gate_each([s[0] for s in sets], keys, okeys, (0, 1), 0xE5)
        assert mid == 0 and (end, end_keys) == (1, 2)
        assert exact == [True, True]
    finally:
        for k in keys:
            k.close()
