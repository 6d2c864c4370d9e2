"""GPU tests of the recorded linear combinations (tfhe_hip_linear): every exported word against numpy's wrapping uint32
arithmetic on exported words (exact: no tolerance anywhere), through the recorder in deferred and immediate mode; ranks of
dependent combinations of one level and the interplay with bootsNOT; linear results feeding gates and LUT bootstraps
against the oracle on the numpy-combined words; a two-key flush; parities of 4 and 5 bits in one bootstrap and a 2-bit
message recombined, at decrypt level; the counters; pool exhaustion."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lut_common as T

pytestmark = pytest.mark.gpu
I32 = np.int32
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from peba1_amd import api
    return api


@pytest.fixture(scope="module")
def sets(api):
    """pname -> (parameter set, keyset on the device), made on demand from the LUT fixtures' seed."""
    made = {}

    def get(pname):
        if pname not in made:
            pp = {"P128": lambda: api.ParameterSet(128), "P80": lambda: api.ParameterSet(80),
                  "P2048": lambda: api.ParameterSet(p2048=True)}[pname]()
            made[pname] = (pp, api.SecretKeySet(pp, T.KEY_SEED, device=True))
        return made[pname]
    yield get
    for _, ks in made.values():
        ks.close()


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


def clear_error():
    from peba1_amd import lib
    lib.load().tfhe_hip_clear_error()


def combine(coefs, words, c0):
    """(0, c0) + sum coefs[i] words[i] on uint32, wrapping: words[i] is [..., n + 1]."""
    acc = np.zeros_like(np.asarray(words[0]), dtype=np.uint32)
    for c, w in zip(coefs, words):
        acc += np.uint32(int(c) & 0xFFFFFFFF) * np.ascontiguousarray(w, dtype=I32).view(np.uint32)
    acc[..., -1] += np.uint32(int(c0) & 0xFFFFFFFF)
    return acc.view(I32)


def random_words(rng, count, words):
    return rng.integers(-2 ** 31, 2 ** 31, (count, words), dtype=np.int64).astype(I32)


# (operand indices, coefficients, c0): nin 1, 2, 3 and 16; 0, 1, -1, INT32_MIN, INT32_MAX and random coefficients; c0 in
# {0, 2^31, -1}; a repeated operand.  RANDOM is replaced by a draw.
RANDOM = None
WORD_CASES = [
    ([0], [1], 0), ([1], [0], 1 << 31), ([2], [-1], -1), ([3], [INT32_MIN], 0), ([4], [INT32_MAX], 1 << 31), ([5], [RANDOM], -1),
    ([0, 1], [1, -1], 0), ([2, 3], [INT32_MIN, INT32_MAX], -1), ([4, 5], [RANDOM, RANDOM], 1 << 31), ([6, 6], [RANDOM, 1], 0),
    ([0, 1, 2], [RANDOM, 0, -1], 1 << 31), ([7, 3, 7], [RANDOM, RANDOM, RANDOM], -1), ([8, 8, 8], [1, 1, INT32_MAX], 0),
    (list(range(16)), [0, 1, -1, INT32_MIN, INT32_MAX] + [RANDOM] * 11, -1),
    ([15 - i for i in range(16)], [RANDOM] * 16, 1 << 31),
    ([3] * 16, [RANDOM] * 16, 0),
]


@pytest.mark.parametrize("count", [1, 257])
@pytest.mark.parametrize("pname", ["P128", "P80", "P2048"])
def test_every_word_is_numpys_through_the_recorder(api, sets, pname, count):
    pp, ks = sets(pname)
    rng = np.random.default_rng(1000 * count + pp.n)
    ins_w = [random_words(rng, count, pp.words) for _ in range(16)]
    guard_w = random_words(rng, count + 3, pp.words)
    cases = [(ops, [int(rng.integers(-2 ** 31, 2 ** 31)) if c is RANDOM else c for c in coefs], c0) for ops, coefs, c0 in WORD_CASES]
    before = api.stats()
    with deferred(api):
        ins = [api.CiphertextArray(pp, count).set_words(w) for w in ins_w]
        guard = api.CiphertextArray(pp, count + 3).set_words(guard_w)        # written before: must be as it was after
        results = [api.CiphertextArray(pp, count) for _ in cases]
        clear_error()
        for r, (ops, coefs, c0) in zip(results, cases):
            if count == 1:
                api.linear(r.at(0), [ins[k].at(0) for k in ops], coefs, c0, ks)
            else:
                api.linear_batch(r, [ins[k] for k in ops], coefs, c0, ks)
        # a result that is also an operand (SSA: the operand is read as it was), after the cases that read it
        own = api.CiphertextArray(pp, count).set_words(ins_w[9])
        if count == 1:
            api.linear(own.at(0), [own.at(0), ins[10].at(0), own.at(0)], [3, -7, INT32_MIN], 1 << 31, ks)
        else:
            api.linear_batch(own, [own, ins[10], own], [3, -7, INT32_MIN], 1 << 31, ks)
        assert api.last_error() == ""
        assert api.flush() == 0                                               # level 0 only: no bootstrap anywhere
    d = delta(api, before)
    assert d["lincomb_ops"] == (len(cases) + 1) * count == d["linear_ops"] and d["lincomb_launches"] == 1
    assert d["blind_rotates"] == 0 == d["keyswitches"] and d["flushes"] == 1
    for r, (ops, coefs, c0) in zip(results, cases):
        got, want = r.words(), combine(coefs, [ins_w[k] for k in ops], c0)
        assert (got == want).all(), (pname, count, ops, coefs, c0)
    assert (own.words() == combine([3, -7, INT32_MIN], [ins_w[9], ins_w[10], ins_w[9]], 1 << 31)).all()
    assert (guard.words() == guard_w).all()
    for a, w in zip(ins, ins_w):
        assert (a.words() == w).all()
    for x in ins + results + [guard, own]:
        x.close()


def test_ranks_and_the_interplay_with_not_word_for_word(api, sets):
    """The three-deep chain and the NOT rewrites of tests/test_linear_cpu.py, on level 0 and riding on a level of bootsAND
    results, in one flush; a 128-term sum as a tree of 16-ary combinations in another."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks = sets("P128")
    rng = np.random.default_rng(77)
    L.tfhe_hip_set_encrypt_seed(55)
    src_w = random_words(rng, 3, pp.words)
    before = api.stats()
    with deferred(api):
        bits = api.CiphertextArray(pp, 4).encrypt([1, 1, 0, 1], ks)
        src = api.CiphertextArray(pp, 3).set_words(src_w)
        gate = api.CiphertextArray(pp, 2)
        L.bootsAND(gate.at(0), bits.at(0), bits.at(1), ks.cloud)
        L.bootsAND(gate.at(1), bits.at(2), bits.at(3), ks.cloud)
        out = {}
        for name, x, y in (("inputs", src.at(0), src.at(1)), ("gates", gate.at(0), gate.at(1))):
            r = api.CiphertextArray(pp, 6)
            L.bootsNOT(r.at(0), x, ks.cloud)                                   # pending NOT (level of x)
            api.linear(r.at(1), [r.at(0), y, src.at(2)], [3, INT32_MIN, -5], 7, ks)       # reads the NOT: rank 0
            api.linear(r.at(2), [r.at(1), x], [2, 1], 1 << 31, ks)            # rank 1
            api.linear(r.at(3), [r.at(2), r.at(1), r.at(2)], [-1, INT32_MAX, 9], -1, ks)  # rank 2
            L.bootsNOT(r.at(4), r.at(3), ks.cloud)                             # NOT of a pending linear result: rank 3
            L.bootsNOT(r.at(5), r.at(0), ks.cloud)                             # NOT of a pending NOT: the operand itself
            out[name] = r
        assert api.last_error() == ""
        assert api.flush() == 1
    d = delta(api, before)
    # (level 0, ranks 0..3) and (level 1, ranks 0..3); two NOTs ran as NOTs, two as linear combinations
    assert d["lincomb_launches"] == 8 and d["lincomb_ops"] == 8 and d["linear_ops"] == 10 and d["flushes"] == 1
    gate_w = gate.words()
    for name, x, y in (("inputs", src_w[0], src_w[1]), ("gates", gate_w[0], gate_w[1])):
        got = out[name].words()
        nx = combine([-1], [x], 0)
        l1 = combine([3, INT32_MIN, -5], [nx, y, src_w[2]], 7)
        l2 = combine([2, 1], [l1, x], 1 << 31)
        l3 = combine([-1, INT32_MAX, 9], [l2, l1, l2], -1)
        for i, want in enumerate((nx, l1, l2, l3, combine([-1], [l3], 0), x)):
            assert (got[i] == want).all(), (name, i)
    # 128 AND results summed as eight 16-ary combinations and one 8-ary: one recording, ranks 0 and 1
    before = api.stats()
    with deferred(api):
        a = api.CiphertextArray(pp, 128).encrypt(rng.integers(0, 2, 128), ks)
        b = api.CiphertextArray(pp, 128).encrypt(rng.integers(0, 2, 128), ks)
        g = api.CiphertextArray(pp, 128)
        api.gate_batch("AND", g, a, b, ks)
        part, total = api.CiphertextArray(pp, 8), api.CiphertextArray(pp, 1)
        for k in range(8):
            api.linear(part.at(k), [g.at(16 * k + t) for t in range(16)], [2] * 16, 0, ks)
        api.linear(total.at(0), [part.at(k) for k in range(8)], [1] * 8, 1 << 30, ks)
        assert api.flush() == 1
    d = delta(api, before)
    assert d["flushes"] == 1 and d["lincomb_launches"] == 2 and d["lincomb_ops"] == 9 and d["blind_rotates"] == 128
    assert (total.words()[0] == combine([2] * 128, list(g.words()), 1 << 30)).all()
    for x in list(out.values()) + [bits, src, gate, a, b, g, part, total]:
        x.close()


def test_linear_results_feed_a_gate_and_a_lut_bootstrap(api, sets, oracle):
    from peba1_amd import lib
    L = lib.load()
    pp, ks = sets("P128")
    oks = oracle.KeySet(oracle.params("P128"), T.KEY_SEED)
    w = oks.encrypt(oracle.Rng(4242), [1, 0, 1, 1])
    v = T.lut_words({"kind": "sectors", "seed": 31, "slots": 8}, pp.N)
    lut = api.Lut(pp, v)
    with deferred(api):
        a = api.CiphertextArray(pp, 4).set_words(w)
        lin = api.CiphertextArray(pp, 2)
        api.linear(lin.at(0), [a.at(0), a.at(1), a.at(2)], [1, 1, -1], 1 << 27, ks)
        api.linear(lin.at(1), [a.at(3), a.at(0)], [2, -1], -(1 << 26), ks)
        r = api.CiphertextArray(pp, 2)
        L.bootsAND(r.at(0), lin.at(0), lin.at(1), ks.cloud)
        api.lut_bootstrap(lut, r.at(1), [lin.at(0)], [1], 12345, ks)
        assert api.last_error() == ""
        assert api.flush() == 1
    l0 = combine([1, 1, -1], [w[0], w[1], w[2]], 1 << 27)
    l1 = combine([2, -1], [w[3], w[0]], -(1 << 26))
    assert (lin.words() == np.stack([l0, l1])).all()
    got = r.words()
    assert (got[0] == oks.gate("AND", l0, l1, 2)).all()
    want, _, _ = T.oracle_lut_bootstrap(oracle, oks, T.linear([1], np.stack([l0]), 12345), v)
    assert (got[1] == want).all()
    for x in (a, lin, r, lut):
        x.close()
    oks.close()


def test_immediate_mode_is_complete_on_return(api, sets):
    pp, ks = sets("P80")
    rng = np.random.default_rng(9)
    w = random_words(rng, 3, pp.words)
    a = api.CiphertextArray(pp, 3).set_words(w)
    r = api.CiphertextArray(pp, 2)
    with deferred(api, False):
        clear_error()
        api.linear(r.at(0), [a.at(0), a.at(1), a.at(2)], [INT32_MIN, -3, 1], -1, ks)
        want = combine([INT32_MIN, -3, 1], list(w), -1)
        s = r.at(0).contents                                   # the host mirror, without an export or a decrypt
        assert [s.a[i] for i in (0, 1, pp.n - 1)] == [int(want[i]) for i in (0, 1, pp.n - 1)] and s.b == int(want[-1])
        api.linear_batch(r, [a, a], [5, 1], 1 << 31, ks)       # a batch is complete on return as well
        assert api.last_error() == ""
        want = combine([5, 1], [w[:2], w[:2]], 1 << 31)
        for i in range(2):
            s = r.at(i).contents
            assert s.a[0] == int(want[i][0]) and s.a[pp.n - 1] == int(want[i][pp.n - 1]) and s.b == int(want[i][-1])
        assert (r.words() == want).all()
    for x in (a, r):
        x.close()


def test_two_key_flush_with_linear_ops_over_both_keys_results(api, sets):
    from peba1_amd import lib
    L = lib.load()
    pp, k1 = sets("P128")
    k2 = api.SecretKeySet(pp, 23, device=True)
    was = L.tfhe_hip_set_batch_keys(1)
    try:
        L.tfhe_hip_set_encrypt_seed(66)
        before = api.stats()
        with deferred(api):
            a1 = api.CiphertextArray(pp, 2).encrypt([1, 1], k1)
            a2 = api.CiphertextArray(pp, 2).encrypt([1, 0], k2)
            g = api.CiphertextArray(pp, 2)
            L.bootsAND(g.at(0), a1.at(0), a1.at(1), k1.cloud)
            L.bootsXOR(g.at(1), a2.at(0), a2.at(1), k2.cloud)
            r = api.CiphertextArray(pp, 3)
            api.linear(r.at(0), [g.at(0), g.at(1)], [3, -2], 1, k1)
            api.linear(r.at(1), [r.at(0), g.at(1), a1.at(0)], [1, INT32_MAX, 4], -1, k2)
            L.bootsNOT(r.at(2), r.at(1), k1.cloud)
            assert api.last_error() == ""
            assert api.flush() == 1
        d = delta(api, before)
        assert api.last_flush_keys() == 2 and d["flushes"] == 1
        assert d["lincomb_ops"] == 3 == d["lincomb_launches"] and d["blind_rotates"] == 2
        gw, aw = g.words(), a1.words()
        r0 = combine([3, -2], [gw[0], gw[1]], 1)
        r1 = combine([1, INT32_MAX, 4], [r0, gw[1], aw[0]], -1)
        assert (r.words() == np.stack([r0, r1, combine([-1], [r1], 0)])).all()
        assert g.decrypt(k1)[0] == 1 and api.phase(g.at(1), k2) > 0
    finally:
        L.tfhe_hip_set_batch_keys(was)
        k2.close()


def signed(ph):
    return (np.asarray(ph) + 0.5) % 1 - 0.5


def test_parity_of_four_and_of_five_bits_in_one_bootstrap(api, sets):
    """Every pattern of 4 and of 5 bits, each bit a bootsAND output (so it carries bootstrap noise): t = c0 + 2 * sum in
    ONE linear combination, then one sign bootstrap (the constant test polynomial 2^29, coefficient 1).  With the bits at
    +-1/8 the doubled sum of an even number of them stands at 0 or 1/2, and c0 = 2^30 = 1/4 moves it to +-1/4: + for an
    even number of ones.  The doubled sum of an odd number stands at +-1/4 already (+ for an odd number of ones), where
    c0 = 2^30 would put it ON the boundaries 0 and 1/2; so the five-bit case takes c0 = 0.  The margin is printed, not
    asserted: computed 2 sqrt(5) 0.005 = 0.022 against 1/4."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks = sets("P128")
    L.tfhe_hip_set_encrypt_seed(404)
    lut = api.Lut.constant(pp, 1 << 29)
    patterns = [(k, p) for k in (4, 5) for p in range(1 << k)]
    nbits = sum(k for k, _ in patterns)
    bits = np.array([(p >> i) & 1 for k, p in patterns for i in range(k)])
    before = api.stats()
    with deferred(api):
        raw = api.CiphertextArray(pp, nbits).encrypt(bits, ks)
        one = api.CiphertextArray(pp, nbits).encrypt([1] * nbits, ks)
        x = api.CiphertextArray(pp, nbits)
        api.gate_batch("AND", x, raw, one, ks)
        t, r = api.CiphertextArray(pp, len(patterns)), api.CiphertextArray(pp, len(patterns))
        at = 0
        for j, (k, _) in enumerate(patterns):
            api.linear(t.at(j), [x.at(at + i) for i in range(k)], [2] * k, (1 << 30) if k == 4 else 0, ks)
            api.lut_bootstrap(lut, r.at(j), [t.at(j)], [1], 0, ks)
            at += k
        assert api.last_error() == ""
        assert api.flush() == 2
    d = delta(api, before)
    assert d["blind_rotates"] == nbits + len(patterns)             # one per input AND, then ONE per parity
    assert d["lincomb_ops"] == len(patterns) and d["lincomb_launches"] == 1
    got = r.decrypt(ks)
    ones = np.array([bin(p).count("1") for _, p in patterns])
    want = np.array([(1 - s % 2) if k == 4 else s % 2 for (k, _), s in zip(patterns, ones)])
    assert (got == want).all()
    ph = signed(np.array([api.phase(t.at(j), ks) for j in range(len(patterns))]) / 2.0 ** 32)
    assert ((ph > 0).astype(int) == want).all()
    margin = np.minimum(np.abs(ph), 0.5 - np.abs(ph))
    print(f"\nparity in one bootstrap: {len(patterns)} patterns; smallest distance of the linear result's phase from the "
          f"decision boundaries 0 and 1/2 (ideal 1/4): {margin.min():.4f}  (4 bits {margin[:16].min():.4f}, 5 bits {margin[16:].min():.4f})")
    for a in (raw, one, x, t, r, lut):
        a.close()


def test_two_bit_message_decomposed_and_recombined(api, sets):
    """m at phase (2m+1)/16, encrypted by tfhe_hip_sym_encrypt_torus; one rotation gives lo and hi at {0, 1/8} (the
    full adder's tables); lo + 2 hi + 1/16 is (2m+1)/16 again, as one linear combination."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks = sets("P128")
    L.tfhe_hip_set_encrypt_seed(808)
    msgs = np.array([m for m in range(4) for _ in range(4)])
    mo = api.LutMulti.from_tables(pp, 1 << 29, [[0, 1, 0, 1], [0, 0, 1, 1]])
    with deferred(api):
        a = api.CiphertextArray(pp, len(msgs))
        for i, m in enumerate(msgs):
            api.encrypt_torus(a.at(i), T.centre(m), ks)
        lo, hi, back = (api.CiphertextArray(pp, len(msgs)) for _ in range(3))
        api.lut_bootstrap_multi_batch(mo, [lo, hi], [a], [1], 0, ks)
        api.linear_batch(back, [lo, hi], [1, 2], 1 << 28, ks)
        assert api.flush() == 1
    ph = np.array([api.phase(back.at(i), ks) & 0xFFFFFFFF for i in range(len(msgs))]) / 2.0 ** 32
    assert (T.decode(ph) == msgs).all()
    assert (back.words() == combine([1, 2], [lo.words(), hi.words()], 1 << 28)).all()
    print(f"\n2-bit message recombined: smallest distance from a sector edge {T.edge_distance(ph).min():.4f} (ideal 1/16)")
    for x in (a, lo, hi, back, mo):
        x.close()


def test_counters_with_one_dead_linear_op(api, sets):
    from peba1_amd import lib
    L = lib.load()
    pp, ks = sets("P80")
    rng = np.random.default_rng(3)
    w = random_words(rng, 2, pp.words)
    before = api.stats()
    with deferred(api):
        a = api.CiphertextArray(pp, 2).set_words(w)
        r = api.CiphertextArray(pp, 3)
        api.linear(r.at(0), [a.at(0), a.at(1)], [1, 1], 0, ks)
        api.linear(r.at(1), [r.at(0)], [5], 0, ks)                 # read by nothing once its handle is overwritten: dead
        api.linear(r.at(1), [a.at(1)], [-1], 3, ks)
        L.bootsNOT(r.at(2), a.at(0), ks.cloud)
        assert api.flush() == 0
    d = delta(api, before)
    assert d["dead_gates"] == 1 and d["lincomb_ops"] == 2 and d["linear_ops"] == 3 and d["lincomb_launches"] == 1
    assert d["reused_gates"] == 0 and d["folded_gates"] == 0
    want = np.stack([combine([1, 1], list(w), 0), combine([-1], [w[1]], 3), combine([-1], [w[0]], 0)])
    assert (r.words() == want).all()
    for x in (a, r):
        x.close()


POOL_WORKER = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from peba1_amd import api, lib
L = lib.load()
pp = api.ParameterSet(80)
ks = api.SecretKeySet(pp, 7, device=True)
L.tfhe_hip_set_encrypt_seed(5)
w = api.CiphertextArray(pp, 2).encrypt([1, 0], ks)
api.linear(w.at(1), [w.at(0)], [1], 0, ks)                 # first use of the key: the slot pool exists from here on
assert (w.words()[1] == w.words()[0]).all()
w.close()
held, refused = [], None
for i in range(200):                 # 64-slot pool: materialised samples pin one slot each
    a = api.CiphertextArray(pp, 1).encrypt([1], ks)
    L.tfhe_hip_clear_error()
    if L.tfhe_hip_import_samples(a.ptr, 1, pp.ptr, a.words().ctypes.data_as(lib.I32P)) != 0:
        refused = i
        break
    held.append(a)
assert refused is not None and "slot pool exhausted" in L.tfhe_hip_last_error().decode()
r = api.CiphertextArray(pp, 1).encrypt([0], ks)
before = r.words().copy()
L.tfhe_hip_clear_error()
api.linear(r.at(0), [held[0].at(0), held[1].at(0)], [2, 3], 1, ks)
assert "slot pool exhausted" in api.last_error(), api.last_error()
assert (r.words() == before).all() and r.at(0).contents.slot == -1
for a in held[:8]:
    a.close()
L.tfhe_hip_clear_error()
api.linear(r.at(0), [held[8].at(0), held[9].at(0)], [2, 3], 1, ks)
assert api.last_error() == ""
w = np.stack([held[8].words()[0], held[9].words()[0]]).view(np.uint32)
want = np.uint32(2) * w[0] + np.uint32(3) * w[1]
want[-1] += np.uint32(1)
assert (r.words()[0].view(np.uint32) == want).all()
print("POOL-OK", refused)
'''


def test_pool_exhaustion_refuses_the_call_without_effect():
    """The pool's size is read when the process starts, hence a process of its own."""
    env = dict(os.environ, TFHE_HIP_POOL_SLOTS="64")
    out = subprocess.run([sys.executable, "-c", POOL_WORKER % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "POOL-OK" in out.stdout
