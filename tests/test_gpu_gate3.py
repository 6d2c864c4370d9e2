"""The three-input bootstrapped gates on the GPU (tfhe_hip_gate3: MAJ3, XOR3, XNOR3 under every negation mask -- not
in upstream TFHE's API).  Every word of every gate against the oracle's bootstrap and key switch of the stated linear
combination t = s (+-A +- B +- C) (tests/gate3_common.py), in every blind-rotate launch form, each proven by the launch
counters; truth tables by decryption; the carry-save circuits against the digests the CPU test computes; multi-key
flushes; constant folding; aliasing, reuse, dead gates and refusals; the noise of the gates."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gate3_common as G

pytestmark = pytest.mark.gpu

NAMES = ("MAJ3", "XOR3", "XNOR3")
CONFIGS = [(name, mask) for name in NAMES for mask in range(8)]
TUNING_DEFAULTS = {"br_tail8": 1, "br_variant": -1, "br_digit_table": 1, "br8_max_rotations": 1 << 30, "reuse_gates": 1,
                   "fold_constants": 0, "batch_keys": 0, "eliminate_dead": 1}
POOL_BITS = [0, 1, 0, 1, 1, 0]


def _oracle_map(fn, items):
    with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as ex:
        return list(ex.map(fn, items))


@pytest.fixture
def tunings():
    from peba1_amd import api
    api.set_deferred(True)
    yield api
    for k, v in TUNING_DEFAULTS.items():
        api.set_tuning(k, v)
    api.set_deferred(False)


def _keys(oracle, pname):
    from peba1_amd import api
    pp = {"P80": lambda: api.ParameterSet(80), "P2048": lambda: api.ParameterSet(p2048=True)}[pname]()
    seed = {"P80": 0x80, "P2048": 0x2048}[pname]
    return pp, api.SecretKeySet(pp, seed, device=True), oracle.KeySet(oracle.params(pname), seed)


def _triple(i):
    return i % 6, (i + 2) % 6, (i + 5) % 6


def _pools(api, pp, ks):
    """Six fresh samples and six once-bootstrapped ones (AND of a fresh sample with itself), materialised."""
    from peba1_amd import lib
    lib.load().tfhe_hip_set_encrypt_seed(0x63)
    fresh = api.CiphertextArray(pp, 6).encrypt(POOL_BITS, ks)
    boot = api.CiphertextArray(pp, 6)
    api.gate_batch("AND", boot, fresh, fresh, ks)
    api.flush()
    return fresh, boot


def _operand_arrays(api, L, pp, ks, pool, count):
    """a, b, c arrays whose element j is a copy (a handle of the same slot) of the pool sample of case j's triple."""
    arrs = [api.CiphertextArray(pp, count) for _ in range(3)]
    for j in range(count):
        for arr, src in zip(arrs, _triple(j)):
            L.bootsCOPY(arr.at(j), pool.at(src), ks.cloud)
    return arrs


# (set, tunings, replicas of the 48 distinct cases in the level, expected rise of br_launches, br8_launches,
# br8_rotations) with 256 CUs: 528 rotations = one full round of the 4-wave kernel and a tail of 16 (the same rows as plans
# of launch_plan.hpp, without a GPU: tests/test_launch_plan_cpu.py)
FORM_ROWS = [
    ("P128", {}, 11, 2, 1, 16),                              # 4-wave launch with its 8-wave tail
    ("P128", {"br_tail8": 0}, 11, 1, 0, 0),                  # one 4-wave launch
    ("P128", {"br_digit_table": 0}, 11, 2, 1, 16),           # both without digit tables
    ("P128", {}, 1, 1, 1, 48),                               # the narrow 8-wave form
    ("P128", {"br8_max_rotations": 0}, 1, 1, 0, 0),          # the same width on the 4-wave kernel
    ("P128", {"br_variant": 2}, 1, 1, 0, 0),                 # the split form
    ("P128", {"br_variant": 4}, 1, 1, 0, 0),                 # the 2-wave form
    ("P80", {}, 11, 2, 1, 16), ("P80", {"br_variant": 2}, 1, 1, 0, 0),
    ("P2048", {}, 1, 1, 0, 0),                               # N = 2048: the split form
]


@pytest.fixture(scope="module")
def set_keys(p128_keys, oracle):
    made = {"P128": p128_keys}
    def get(pname):
        if pname not in made:
            made[pname] = _keys(oracle, pname)
        return made[pname]
    yield get
    for name, (pp, ks, oks) in made.items():
        if name != "P128":
            ks.close()


@pytest.fixture(scope="module")
def oracle_words(set_keys):
    """Per set: the pools' words and the oracle's result of the 48 distinct cases (24 gates x fresh / bootstrapped)."""
    cache = {}
    def get(pname, api):
        if pname in cache:
            return cache[pname]
        pp, ks, oks = set_keys(pname)
        fresh, boot = _pools(api, pp, ks)
        fw = fresh.words()
        bw = boot.words()
        want_boot = _oracle_map(lambda i: oks.gate("AND", fw[i], fw[i], use_ntt=2), range(6))
        assert np.array_equal(bw, np.stack(want_boot))
        def one(case):
            (name, mask), pool_words, j = case
            a, b, c = _triple(j)
            return G.oracle_gate3(oks, name, mask, pool_words[a], pool_words[b], pool_words[c])
        cases = [(cfg, w, j) for w in (fw, bw) for j, cfg in enumerate(CONFIGS)]
        want = _oracle_map(one, cases)
        cache[pname] = (fresh, boot, np.stack(want[:24]), np.stack(want[24:]))
        return cache[pname]
    return get


@pytest.mark.parametrize("pname,tune,replicas,br,br8,rot8", FORM_ROWS)
def test_every_word_in_every_launch_form(set_keys, oracle_words, tunings, pname, tune, replicas, br, br8, rot8):
    api = tunings
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = set_keys(pname)
    fresh, boot, want_fresh, want_boot = oracle_words(pname, api)
    for k, v in tune.items():
        api.set_tuning(k, v)
    api.set_tuning("reuse_gates", 0)                         # replicas are evaluated, not shared
    results = []
    operands = [[_operand_arrays(api, L, pp, ks, pool, 24) for pool in (fresh, boot)] for _ in range(replicas)]
    api.flush()
    s0 = api.stats()
    for r in range(replicas):
        for pool_i in range(2):
            a, b, c = operands[r][pool_i]
            res = api.CiphertextArray(pp, 24)
            if r % 2 == 0:                                   # the batch entry, one gate and mask per call: 1-element arrays
                for j, (name, mask) in enumerate(CONFIGS):
                    rc = L.tfhe_hip_gate3_batch(G.GATE3[name][0], mask, res.at(j), a.at(j), b.at(j), c.at(j), 1, ks.cloud)
                    assert rc == 0, api.last_error()
            else:                                            # recorded call by call
                for j, (name, mask) in enumerate(CONFIGS):
                    api.gate3(name, res.at(j), a.at(j), b.at(j), c.at(j), ks, negate_mask=mask)
            results.append((pool_i, res))
    assert api.flush() == 1
    d = {k: api.stats()[k] - s0[k] for k in ("br_launches", "br8_launches", "br8_rotations", "blind_rotates", "keyswitches")}
    assert d["blind_rotates"] == d["keyswitches"] == 48 * replicas
    assert (d["br_launches"], d["br8_launches"], d["br8_rotations"]) == (br, br8, rot8), d
    for pool_i, res in results:
        assert np.array_equal(res.words(), want_boot if pool_i else want_fresh), (pname, tune, pool_i)


def test_immediate_mode_and_whole_array_batch(set_keys, oracle_words, tunings):
    api = tunings
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = set_keys("P128")
    fresh, boot, want_fresh, want_boot = oracle_words("P128", api)
    a, b, c = _operand_arrays(api, L, pp, ks, boot, 24)
    api.flush()
    api.set_deferred(False)                                  # every call complete on return, host mirror refreshed
    res = api.CiphertextArray(pp, 24)
    for j, (name, mask) in enumerate(CONFIGS):
        before = api.stats()["flushes"]
        api.gate3(name, res.at(j), a.at(j), b.at(j), c.at(j), ks, negate_mask=mask)
        assert api.stats()["flushes"] == before + 1
        mirror = np.ctypeslib.as_array(res.at(j).contents.a, shape=(pp.n,))
        assert np.array_equal(mirror, want_boot[j][:-1]) and res.at(j).contents.b == want_boot[j][-1]
    # a whole array under one gate and mask, immediate mode: one flush inside the call
    n = 16
    arrs = [api.CiphertextArray(pp, n) for _ in range(3)]
    idx = [(j % 6, (j // 2) % 6, (j * 5 + 1) % 6) for j in range(n)]
    for j in range(n):
        for arr, src in zip(arrs, idx[j]):
            L.bootsCOPY(arr.at(j), boot.at(src), ks.cloud)
    out = api.CiphertextArray(pp, n)
    before = api.stats()["flushes"]
    api.gate3_batch("XOR3", out, arrs[0], arrs[1], arrs[2], ks, negate_mask=5)
    assert api.stats()["flushes"] == before + 1
    bw = boot.words()
    want = _oracle_map(lambda t: G.oracle_gate3(oks, "XOR3", 5, bw[t[0]], bw[t[1]], bw[t[2]]), idx)
    assert np.array_equal(out.words(), np.stack(want))


def test_truth_tables_by_decryption(p128_keys, tunings):
    """All 8 input combinations x 3 gates x 8 masks, on fresh and on bootstrapped inputs."""
    api = tunings
    from peba1_amd import lib
    L = lib.load()
    pp, ks, _ = p128_keys
    L.tfhe_hip_set_encrypt_seed(0x77)
    combos = [(v & 1, (v >> 1) & 1, (v >> 2) & 1) for v in range(8)]
    fresh = [api.CiphertextArray(pp, 8).encrypt([cmb[i] for cmb in combos], ks) for i in range(3)]
    boot = [api.CiphertextArray(pp, 8) for _ in range(3)]
    for i in range(3):
        api.gate_batch("OR", boot[i], fresh[i], fresh[i], ks)
    outs = []
    for ins in (fresh, boot):
        for name, mask in CONFIGS:
            r = api.CiphertextArray(pp, 8)
            api.gate3_batch(name, r, ins[0], ins[1], ins[2], ks, negate_mask=mask)
            outs.append((name, mask, r))
    api.flush()
    for name, mask, r in outs:
        assert r.decrypt(ks).tolist() == [G.gate3_truth(name, mask, *cmb) for cmb in combos], (name, mask)


def _circuit_inputs(api, pp, oks, oracle, values_and_bits):
    arrs = []
    for words in G.input_words(oks, oracle.Rng(G.ENC_SEED), values_and_bits):
        arrs.append(api.CiphertextArray(pp, len(words)).set_words(words))
    return arrs


def test_circuit_digests_and_full_size_matches(p128_keys, oracle, tunings):
    api = tunings
    from types import SimpleNamespace
    from peba1_amd import circuits, lib
    pp, ks, oks = p128_keys
    digests = G.load_digests()
    h = G.HAMMING16
    a, b, bound = _circuit_inputs(api, pp, oks, oracle, [(h["a"], 16), (h["b"], 16), (h["bound"], 5)])
    rb = api.CiphertextArray(pp, 5)
    s0 = api.stats()
    circuits.hamming_match_csa(rb, a, b, 16, bound, ks)
    api.flush()
    d = {k: api.stats()[k] - s0[k] for k in ("blind_rotates", "reused_gates", "dead_gates")}
    assert sum(d.values()) == digests["hamming_match_csa_16"]["bootstraps"], d      # one rotation per gate of the netlist
    assert G.sha256_words(rb.words()) == digests["hamming_match_csa_16"]["sha256"]
    assert rb.decrypt(ks).tolist() == [1, 0, 0, 0, 0]
    f = G.FF3_2
    # the netlist worker encrypts the probe's slots, then the template's, then the bound
    ins = _circuit_inputs(api, pp, oks, oracle, [(v, 8) for v in f["probe"] + f["template"]] + [(f["bound"], 24)])
    rb = api.CiphertextArray(pp, 24)
    circuits.function_f_fast3(rb, SimpleNamespace(slots=ins[:2]), SimpleNamespace(slots=ins[2:4]), ins[4], 8, ks)
    api.flush()
    assert G.sha256_words(rb.words()) == digests["function_f_fast3_2"]["sha256"]
    # full size, both sides of the bound, by decryption
    lib.load().tfhe_hip_set_encrypt_seed(0x128)
    rng = np.random.default_rng(128)
    av = int.from_bytes(rng.bytes(16), "little")
    bv = av ^ sum(1 << int(i) for i in rng.choice(128, 41, replace=False))
    a, b = circuits.encrypt_number(pp, av, 128, ks), circuits.encrypt_number(pp, bv, 128, ks)
    cnt = api.CiphertextArray(pp, 8)
    circuits.hamming_distance_csa(cnt, a, b, 128, ks)
    assert circuits.decrypt_number(cnt, ks) == 41
    for bd, want in ((40, 1), (41, 0), (42, 0)):
        rb = api.CiphertextArray(pp, 8)
        circuits.hamming_match_csa(rb, a, b, 128, circuits.encrypt_number(pp, bd, 8, ks), ks)
        assert rb.decrypt(ks).tolist() == [want] + [0] * 7, bd
    template = [(37 * i + 11) % 255 for i in range(128)]
    probe = [t + 1 for t in template]                        # distance 128
    S = circuits.EncryptedVector(pp, probe, 8, ks)
    T = circuits.EncryptedVector(pp, template, 8, ks)
    s0 = api.stats()
    for bd, want in ((127, 1), (128, 0)):
        rb = api.CiphertextArray(pp, 24)
        circuits.function_f_fast3(rb, S, T, circuits.encrypt_number(pp, bd, 24, ks), 8, ks)
        assert rb.decrypt(ks).tolist() == [want] + [0] * 23, bd
    print("function_f_fast3, 128 slots, two bounds: blind rotations", api.stats()["blind_rotates"] - s0["blind_rotates"])


def test_three_keys_one_flush(p128_keys, oracle, tunings):
    """Unequal shares under three keys in one flush: every client's words equal its single-key run; the batch entry too."""
    api = tunings
    from peba1_amd import circuits, lib
    L = lib.load()
    pp, ks0, _ = p128_keys
    own = [api.SecretKeySet(pp, s, device=True) for s in (0x4B1, 0x4B2)]
    keys = [ks0] + own
    try:
        L.tfhe_hip_set_encrypt_seed(0x3C)
        shares = (40, 7, 1)
        ins = []
        for k, n in zip(keys, shares):
            bits = np.random.default_rng(n).integers(0, 2, (3, n))
            ins.append([api.CiphertextArray(pp, n).encrypt(bits[i], k) for i in range(3)])
        for x in ins:
            for arr in x:
                arr.set_words(arr.words())                   # on the device before anything is recorded

        def record(c):
            out = []
            for name, mask in (("MAJ3", 0), ("XOR3", 3), ("XNOR3", 4), ("MAJ3", 6)):
                r = api.CiphertextArray(pp, shares[c])
                api.gate3_batch(name, r, ins[c][0], ins[c][1], ins[c][2], keys[c], negate_mask=mask)
                out.append(r)
            return out
        api.set_tuning("batch_keys", 1)
        api.flush()
        before = api.stats()["flushes"]
        batched = [record(c) for c in range(3)]
        api.flush()
        assert api.stats()["flushes"] == before + 1 and api.last_flush_keys() == 3
        batched = [[r.words() for r in rs] for rs in batched]
        api.set_tuning("batch_keys", 0)
        for c in range(3):
            solo = record(c)
            api.flush()
            assert api.last_flush_keys() == 1
            for r, w in zip(solo, batched[c]):
                assert np.array_equal(r.words(), w), c
        # the batch entry with the carry-save match: three clients, one flush, each client's own solo words
        A = [circuits.encrypt_number(pp, 0xB3C5, 16, k) for k in keys]
        B = [circuits.encrypt_number(pp, 0xA98E, 16, k) for k in keys]
        bounds = [circuits.encrypt_number(pp, 6, 5, k) for k in keys]
        for arr in A + B + bounds:
            arr.set_words(arr.words())
        rbs = [api.CiphertextArray(pp, 5) for _ in keys]
        before = api.stats()["flushes"]
        assert circuits.hamming_match_batch(rbs, A, B, 16, bounds, keys, csa=True) > 0
        assert api.stats()["flushes"] == before + 1 and api.last_flush_keys() == 3
        for c in range(3):
            rb = api.CiphertextArray(pp, 5)
            circuits.hamming_match_csa(rb, A[c], B[c], 16, bounds[c], keys[c])
            api.flush()
            assert np.array_equal(rb.words(), rbs[c].words()), c
            assert rb.decrypt(keys[c]).tolist() == [1, 0, 0, 0, 0]
    finally:
        api.set_tuning("batch_keys", 0)
        for k in own:
            k.close()


def test_constant_folding(p128_keys, tunings):
    """One constant operand: exactly the words of the two-input gate with the same truth table; two: no bootstrap."""
    api = tunings
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = p128_keys
    L.tfhe_hip_set_encrypt_seed(0xF0)
    x = api.CiphertextArray(pp, 2).encrypt([1, 0], ks)
    xw = x.words()
    x.set_words(xw)
    const = api.CiphertextArray(pp, 2)
    L.bootsCONSTANT(const.at(0), 0, ks.cloud)
    L.bootsCONSTANT(const.at(1), 1, ks.cloud)
    api.set_tuning("fold_constants", 1)
    AND_V = ["AND", "ANDNY", "ANDYN", "NOR"]
    OR_V = ["OR", "ORNY", "ORYN", "NAND"]
    cases = []
    for name in NAMES:
        for mask in range(8):
            for pos in range(3):                             # where the constant stands
                for v in (0, 1):
                    cases.append((name, mask, pos, v))
    api.flush()
    s0 = api.stats()
    outs = []
    for name, mask, pos, v in cases:
        ops = [x.at(0), x.at(1)]
        ops.insert(pos, const.at(v))
        r = api.CiphertextArray(pp, 1)
        api.gate3(name, r.at(0), ops[0], ops[1], ops[2], ks, negate_mask=mask)
        outs.append(r)
    api.flush()
    s1 = api.stats()
    assert s1["folded_gates"] - s0["folded_gates"] == len(cases)
    want_cache = {}
    for (name, mask, pos, v), r in zip(cases, outs):
        negs = [(mask >> i) & 1 for i in range(3)]
        veff = v ^ negs.pop(pos)
        nx, ny = negs
        if name == "MAJ3":
            g2 = (OR_V if veff else AND_V)[nx + 2 * ny]
        else:
            g2 = "XNOR" if veff ^ nx ^ ny ^ (name == "XNOR3") else "XOR"
        if g2 not in want_cache:
            want_cache[g2] = oks.gate(g2, xw[0], xw[1], use_ntt=2)
        assert np.array_equal(r.words()[0], want_cache[g2]), (name, mask, pos, v, g2)
        bits = [1, 0]
        bits.insert(pos, v)
        assert r.decrypt(ks)[0] == G.gate3_truth(name, mask, *bits)
    # (identical two-input gates were shared: at most the ten distinct gates ran)
    assert s1["blind_rotates"] - s0["blind_rotates"] <= 10
    # two and three constants: the remaining operand, its negation or a constant -- no bootstrap at all
    s0 = api.stats()
    outs = []
    for name in NAMES:
        for mask in range(8):
            for v0 in (0, 1):
                for v1 in (0, 1):
                    r = api.CiphertextArray(pp, 1)
                    api.gate3(name, r.at(0), const.at(v0), x.at(0), const.at(v1), ks, negate_mask=mask)
                    outs.append((G.gate3_truth(name, mask, v0, 1, v1), r))
                    r = api.CiphertextArray(pp, 1)
                    api.gate3(name, r.at(0), const.at(v0), const.at(v1), const.at(v0), ks, negate_mask=mask)
                    outs.append((G.gate3_truth(name, mask, v0, v1, v0), r))
    api.flush()
    s1 = api.stats()
    assert s1["blind_rotates"] == s0["blind_rotates"] and s1["keyswitches"] == s0["keyswitches"]
    assert s1["folded_gates"] - s0["folded_gates"] == len(outs)
    for want, r in outs:
        assert r.decrypt(ks)[0] == want


def test_aliasing_reuse_dead_gates_and_refusals(p128_keys, tunings):
    api = tunings
    from peba1_amd import lib
    L = lib.load()
    pp, ks, oks = p128_keys
    L.tfhe_hip_set_encrypt_seed(0xA1)
    x = api.CiphertextArray(pp, 3).encrypt([1, 0, 1], ks)
    xw = x.words()
    x.set_words(xw)
    # a result that is also an input, twice in a row: SSA renaming keeps the operands' values
    acc = api.CiphertextArray(pp, 1)
    L.bootsCOPY(acc.at(0), x.at(0), ks.cloud)
    api.gate3("MAJ3", acc.at(0), acc.at(0), x.at(1), x.at(2), ks)                  # maj(1,0,1) = 1
    api.gate3("XOR3", acc.at(0), x.at(1), acc.at(0), acc.at(0), ks, negate_mask=2)  # 0 ^ !1 ^ 1 = 1
    api.flush()
    w1 = G.oracle_gate3(oks, "MAJ3", 0, xw[0], xw[1], xw[2])
    assert np.array_equal(acc.words()[0], G.oracle_gate3(oks, "XOR3", 2, xw[1], w1, w1))
    assert acc.decrypt(ks)[0] == 1
    # the same gate recorded twice -- the second time with its operands in another order -- is evaluated once
    r = api.CiphertextArray(pp, 2)
    s0 = api.stats()
    api.gate3("MAJ3", r.at(0), x.at(0), x.at(1), x.at(2), ks, negate_mask=1)
    api.gate3("MAJ3", r.at(1), x.at(2), x.at(0), x.at(1), ks, negate_mask=2)
    api.flush()
    s1 = api.stats()
    assert s1["reused_gates"] - s0["reused_gates"] == 1 and s1["blind_rotates"] - s0["blind_rotates"] == 1
    assert np.array_equal(r.words()[0], r.words()[1])
    assert np.array_equal(r.words()[0], G.oracle_gate3(oks, "MAJ3", 1, xw[0], xw[1], xw[2]))
    # another mask is another gate
    api.gate3("MAJ3", r.at(0), x.at(0), x.at(1), x.at(2), ks, negate_mask=1)
    api.gate3("MAJ3", r.at(1), x.at(0), x.at(1), x.at(2), ks, negate_mask=4)
    api.flush()
    s2 = api.stats()
    assert s2["reused_gates"] == s1["reused_gates"] and s2["blind_rotates"] - s1["blind_rotates"] == 2
    # a three-input gate nobody can observe is not evaluated
    t = api.CiphertextArray(pp, 1)
    api.gate3("XNOR3", t.at(0), x.at(0), x.at(1), x.at(2), ks)
    L.bootsCOPY(t.at(0), x.at(0), ks.cloud)                  # the only handle of the result is re-pointed
    api.flush()
    s3 = api.stats()
    assert s3["dead_gates"] - s2["dead_gates"] == 1 and s3["blind_rotates"] == s2["blind_rotates"]
    # refusals: message set, result untouched, nothing recorded
    keep = r.words()
    foreign = (lib.LweSample * 1)()
    for bad in (lambda: L.tfhe_hip_gate3(0, 0, r.at(0), x.at(0), x.at(1), foreign, ks.cloud),
                lambda: L.tfhe_hip_gate3(0, 0, foreign, x.at(0), x.at(1), x.at(2), ks.cloud),
                lambda: L.tfhe_hip_gate3(0, 0, r.at(0), x.at(0), x.at(1), x.at(2), None),
                lambda: L.tfhe_hip_gate3(3, 0, r.at(0), x.at(0), x.at(1), x.at(2), ks.cloud),
                lambda: L.tfhe_hip_gate3(0, 8, r.at(0), x.at(0), x.at(1), x.at(2), ks.cloud)):
        L.tfhe_hip_clear_error()
        bad()
        assert api.last_error() != ""
    p80 = api.ParameterSet(80)
    other = api.CiphertextArray(p80, 1)
    k80 = api.SecretKeySet(p80, 0x80, device=True)
    try:
        api.gate_batch("AND", other, other, other, k80)      # binds the array to the other dimension's pool
        L.tfhe_hip_clear_error()
        L.tfhe_hip_gate3(0, 0, r.at(0), x.at(0), x.at(1), other.at(0), ks.cloud)
        assert "dimension" in api.last_error()
        L.tfhe_hip_clear_error()
        assert L.tfhe_hip_gate3_batch(0, 0, r.ptr, x.ptr, x.ptr, other.ptr, 1, ks.cloud) == -1
    finally:
        api.flush()
        k80.close()
    L.tfhe_hip_clear_error()
    s4 = api.stats()
    assert api.flush() == 0 and s4["blind_rotates"] == api.stats()["blind_rotates"]
    assert np.array_equal(r.words(), keep)


NOISE_SETS = [("P128", 2.0 ** -15, 2.0 ** -25), ("P80", 2.44e-5, 7.18e-9)]


@pytest.mark.parametrize("pname,ks_stdev,bk_stdev", NOISE_SETS)
def test_noise_of_three_input_gates(pname, ks_stdev, bk_stdev, tunings):
    """The method of tests/test_gpu_noise.py on bootstrapped inputs: the output of a bootstrap does not depend on its
    input's noise, so MAJ3 / XOR3 outputs carry the per-gate variance predicted there; the INPUT phase s (+-a +- b +- c)
    stays inside its decision region -- 1/8 from the boundaries for MAJ3, 1/4 for XOR3 -- by the margin that three
    terms of the per-gate deviation sigma leave at 6.5 sigma (the largest deviation that file tolerates):
    1/8 - 6.5 sqrt(3) sigma and 1/4 - 6.5 * 2 sqrt(3) sigma."""
    api = tunings
    from peba1_amd import lib
    from test_gpu_noise import ksk_mean_shift, phase_errors, predicted_variance
    L = lib.load()
    pp = api.ParameterSet(128) if pname == "P128" else api.ParameterSet(80)
    ks = api.SecretKeySet(pp, 0xA015E + len(pname), device=True)
    try:
        L.tfhe_hip_set_encrypt_seed(0xB0 + pp.n)
        rng = np.random.default_rng(pp.n + 3)
        n = 1024
        s = ks.lwe_key().copy()
        worst, typ, kb = predicted_variance(pp, ks_stdev, bk_stdev)
        shift = ksk_mean_shift(ks, pp)
        bits = rng.integers(0, 2, (3, n))
        boot = []
        for i in range(3):
            f = api.CiphertextArray(pp, n).encrypt(bits[i], ks)
            b = api.CiphertextArray(pp, n)
            api.gate_batch("AND", b, f, f, ks)
            boot.append(b)
        api.flush()
        bw = [b.words() for b in boot]
        sigma = np.sqrt(typ)
        errs = []
        for name, mask, coef, region in (("MAJ3", 0, 1, 0.125), ("MAJ3", 5, 1, 0.125), ("XOR3", 0, 2, 0.25),
                                         ("XOR3", 2, 2, 0.25)):
            r = api.CiphertextArray(pp, n)
            api.gate3_batch(name, r, boot[0], boot[1], boot[2], ks, negate_mask=mask)
            api.flush()
            want = np.array([G.gate3_truth(name, mask, *bits[:, j]) for j in range(n)])
            e = phase_errors(r.words(), s, want)
            assert np.abs(e).max() < 6.5 * sigma, (pname, name, mask, np.abs(e).max())
            errs.append(e)
            # the input phase of the gate: distance from the nearest decision boundary (0 or 1/2)
            lin = np.stack([G.gate3_lin(name, mask, bw[0][j], bw[1][j], bw[2][j]) for j in range(n)])
            a = lin[:, :-1].astype(np.int64)
            ph = (lin[:, -1].astype(np.int64) - a @ s.astype(np.int64)) & 0xFFFFFFFF
            ph = ph.astype(np.float64) / 2.0 ** 32           # in [0, 1): boundaries at 0, 1/2 and 1
            margin = np.minimum(np.minimum(ph, np.abs(ph - 0.5)), 1.0 - ph).min()
            bound = region - 6.5 * coef * np.sqrt(3.0) * sigma
            print(f"\n{pname} {name} mask {mask}: smallest input margin {margin:.4f} (nominal {region}, bound {bound:.4f}); "
                  f"output var {e.var():.3e} (predicted {typ:.3e})")
            assert margin >= bound, (pname, name, mask, margin, bound)
        e = np.concatenate(errs)
        sem = np.sqrt(e.var() / e.size)
        assert abs(e.mean() - shift) < 6 * sem + 4 * kb
        assert e.var() < worst and 0.7 * typ < e.var() < 1.4 * typ, (pname, e.var(), typ)
    finally:
        ks.close()
