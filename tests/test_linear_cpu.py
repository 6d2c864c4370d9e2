"""CPU tests of the recorded linear combinations (tfhe_hip_linear): the level plan of recordings that hold them, through
the host-logic entry tfhe_hip_test_level_plan_lin (which runs the recorder's own graph, levelling and plan code over a
plain slot table); the refusals that need no device; tfhe_hip_sym_encrypt_torus and tfhe_hip_sym_phase on host-only
keysets.  The words themselves are checked on the GPU (tests/test_gpu_linear.py)."""
import ctypes as C

import numpy as np
import pytest

I32 = np.int32
P32 = C.POINTER(C.c_int32)
AND, XOR, NOT, LIN = 2, 4, 17, 66
INT32_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from peba1_amd import api
    return api


def p(a):
    return a.ctypes.data_as(P32)


class Recording:
    """Records of tfhe_hip_test_level_plan_lin: ids name samples; an id used as a destination is renamed like a result."""

    def __init__(self):
        self.ops, self.terms = [], []

    def gate(self, kind, dst, a, b=-1, c=-1):
        self.ops.append([kind, dst, a, b, c] + [0] * 11)
        return len(self.ops) - 1

    def lin(self, dst, terms, c0=0):
        first = len(self.terms)
        self.terms += [list(t) for t in terms]
        self.ops.append([LIN, dst, -1, -1, -1, first, len(terms), 0, 0, c0] + [0] * 6)
        return len(self.ops) - 1


def plan(L, rec, keys=None, nkeys=1, unit=256, balance=0, reuse=1, dead=()):
    ops = np.ascontiguousarray(rec.ops, dtype=I32).reshape(-1, 16)
    terms = np.ascontiguousarray(rec.terms + [[0, 0]], dtype=I32)
    count = len(ops)
    keys = np.zeros(count, dtype=I32) if keys is None else np.ascontiguousarray(keys, dtype=I32)
    ndead = len(dead)
    dead = np.ascontiguousarray(list(dead) + [0], dtype=I32)
    levels, ranks, shared, sizes = np.zeros(count, I32), np.zeros(count, I32), np.zeros(count, I32), np.zeros(6, I32)
    rot_off, ks_off = np.zeros(count + 1, I32), np.zeros(count + 1, I32)
    rot_koff, ks_koff = np.zeros(count * nkeys + 1, I32), np.zeros(count * nkeys + 1, I32)
    rot_key, rots, kss = np.zeros(2 * count, I32), np.zeros((2 * count, 10), I32), np.zeros((4 * count, 4), I32)
    lin_sizes, level_off = np.zeros(2, I32), np.zeros(count + 2, I32)
    launch_off, launch_rank, descs = np.zeros(count + 1, I32), np.zeros(count, I32), np.zeros((count, 35), I32)
    depth = L.tfhe_hip_test_level_plan_lin(p(ops), p(keys), count, nkeys, unit, balance, reuse, p(dead), ndead, p(terms),
                                           len(rec.terms), p(levels), p(ranks), p(shared), p(sizes), p(rot_off), p(ks_off),
                                           p(rot_koff), p(ks_koff), p(rot_key), p(rots), p(kss), p(lin_sizes), p(level_off),
                                           p(launch_off), p(launch_rank), p(descs))
    assert depth >= 0, L.tfhe_hip_last_error().decode()
    nlaunch, ndesc = int(lin_sizes[0]), int(lin_sizes[1])
    launches = []                      # (level, rank, [(dst, c0, [(slot, coef), ...]), ...]) in launch order
    for lvl in range(depth + 1):
        for j in range(level_off[lvl], level_off[lvl + 1]):
            ds = [(int(d[0]), int(d[2]), [(int(d[3 + t]), int(d[19 + t])) for t in range(d[1])])
                  for d in descs[launch_off[j]:launch_off[j + 1]]]
            launches.append((lvl, int(launch_rank[j]), ds))
    assert level_off[depth + 1] == nlaunch and (nlaunch == 0 or launch_off[nlaunch] == ndesc)
    return {"depth": depth, "levels": levels.tolist(), "ranks": ranks.tolist(), "shared": shared.tolist(),
            "rotations": int(sizes[1]), "keyswitches": int(sizes[2]), "keys": int(sizes[5]), "launches": launches,
            "rots": rots[:sizes[1]], "kss": kss[:sizes[2]], "rot_off": rot_off[:depth + 1].tolist()}


# ---- levels and ranks --------------------------------------------------------------------------------------------------
def test_level_zero_on_inputs_and_level_of_the_gates_it_reads(L):
    r = Recording()
    r.lin(10, [(0, 3), (1, -1)], c0=7)                 # inputs only
    r.gate(AND, 11, 0, 1)                              # level 1
    r.gate(XOR, 12, 11, 2)                             # level 2
    r.lin(13, [(11, 2), (0, 1)])                       # rides on level 1
    r.lin(14, [(12, 1), (11, 1), (0, 5)])              # rides on level 2
    out = plan(L, r)
    assert out["levels"] == [0, 1, 2, 1, 2] and out["ranks"] == [0, 0, 0, 0, 0]
    assert [(lv, rk) for lv, rk, _ in out["launches"]] == [(0, 0), (1, 0), (2, 0)]
    assert out["launches"][0][2] == [(10, 7, [(0, 3), (1, -1)])]
    assert out["launches"][2][2] == [(14, 0, [(12, 1), (11, 1), (0, 5)])]
    assert out["rotations"] == 2 == out["keyswitches"]             # a linear combination takes neither


@pytest.mark.parametrize("on_gates", [False, True])
def test_a_chain_of_three_gets_ranks_0_1_2_and_three_launches(L, on_gates):
    r = Recording()
    base = 0
    if on_gates:
        r.gate(AND, 20, 0, 1)
        base = 1
    src = 20 if on_gates else 0
    r.lin(10, [(src, 1), (1, 1)])
    r.lin(11, [(10, 2), (2, 1)])
    r.lin(12, [(11, -1), (10, 1), (11, 3)])
    r.lin(13, [(src, 5)])                              # independent: rank 0, in the first launch
    out = plan(L, r)
    lv = 1 if on_gates else 0
    assert out["levels"][base:] == [lv] * 4 and out["ranks"][base:] == [0, 1, 2, 0]
    assert [(a, b, [d[0] for d in ds]) for a, b, ds in out["launches"]] == [(lv, 0, [10, 13]), (lv, 1, [11]), (lv, 2, [12])]


def test_an_operand_a_pending_not_writes_is_its_origin_with_the_sign_flipped(L):
    r = Recording()
    r.gate(AND, 10, 0, 1)
    r.gate(NOT, 11, 10)                                # pending NOT of a gate result
    r.gate(NOT, 12, 2)                                 # pending NOT of an input
    r.lin(13, [(11, 3), (12, INT32_MIN), (12, -5), (0, 1)], c0=9)
    out = plan(L, r, dead=(11, 12))                    # the NOTs' own handles go: nothing else reads them
    assert out["launches"] == [(1, 0, [(13, 9, [(10, -3), (2, INT32_MIN), (2, 5), (0, 1)])])]
    assert out["levels"] == [1, -1, -1, 1]            # both NOTs eliminated: the combination does not depend on them
    alive = plan(L, r)
    assert alive["levels"] == [1, 1, 0, 1] and alive["launches"] == out["launches"]


def test_a_not_of_a_pending_linear_result_is_the_result_times_minus_one(L):
    r = Recording()
    r.lin(10, [(0, 2), (1, 2)], c0=1 << 30)
    r.gate(NOT, 11, 10)
    r.gate(NOT, 12, 11)                                # and again: a third link of the chain, no aliasing needed
    r.gate(AND, 13, 12, 0)
    out = plan(L, r)
    assert out["levels"] == [0, 0, 0, 1] and out["ranks"] == [0, 1, 2, 0]
    assert out["launches"] == [(0, 0, [(10, 1 << 30, [(0, 2), (1, 2)])]), (0, 1, [(11, 0, [(10, -1)])]),
                               (0, 2, [(12, 0, [(11, -1)])])]
    assert out["rots"][0][:2].tolist() == [12, 0]


def test_a_gate_that_reads_a_linear_result_of_level_l_is_at_l_plus_1(L):
    r = Recording()
    r.gate(AND, 10, 0, 1)
    r.gate(AND, 11, 2, 3)
    r.lin(12, [(10, 2), (11, 2)], c0=1 << 30)          # level 1
    r.lin(13, [(12, 1), (0, 1)])                       # level 1, rank 1
    r.gate(XOR, 14, 13, 0)                             # level 2
    r.gate(AND, 15, 0, 1)                              # an equal gate is still shared next to linear ops
    out = plan(L, r)
    assert out["levels"] == [1, 1, 1, 1, 2, 1] and out["ranks"] == [0, 0, 0, 1, 0, 0]
    assert out["shared"] == [-1, -1, -1, -1, -1, 0]
    assert out["rot_off"] == [0, 2, 3]


def test_a_dead_linear_op_and_what_only_it_read_are_eliminated(L):
    r = Recording()
    r.gate(AND, 10, 0, 1)                              # read by the dead combination only
    r.gate(AND, 11, 2, 3)                              # read by a live one too
    r.lin(12, [(10, 1), (11, 1)])
    r.lin(13, [(11, 1), (0, 1)])
    out = plan(L, r, dead=(12, 10))
    assert out["levels"] == [-1, 1, -1, 1] and out["ranks"] == [-1, 0, -1, 0]
    assert out["launches"] == [(1, 0, [(13, 0, [(11, 1), (0, 1)])])] and out["rotations"] == 1


def test_two_equal_linear_ops_are_both_kept(L):
    r = Recording()
    r.lin(10, [(0, 1), (1, 1)], c0=5)
    r.lin(11, [(0, 1), (1, 1)], c0=5)
    for reuse in (0, 1):
        out = plan(L, r, reuse=reuse)
        assert out["shared"] == [-1, -1] and out["levels"] == [0, 0]
        assert [d[0] for _, _, ds in out["launches"] for d in ds] == [10, 11]


def test_a_multi_key_recording_keeps_one_level_sequence(L):
    r = Recording()
    r.gate(AND, 10, 0, 1)                              # key 0
    r.gate(AND, 11, 2, 3)                              # key 1
    r.lin(12, [(10, 1), (11, -1)])                     # over results of both keys
    r.gate(XOR, 13, 12, 0)                             # key 1
    r.lin(14, [(13, 1), (12, 1)])
    out = plan(L, r, keys=[0, 1, 0, 1, 1], nkeys=2)
    assert out["depth"] == 2 and out["levels"] == [1, 1, 1, 2, 2]
    assert [(a, b) for a, b, _ in out["launches"]] == [(1, 0), (2, 0)]
    assert out["keys"] == 3                            # one key index per rotation; none for the linear ops


def test_a_128_term_sum_as_a_tree_stays_one_recording(L):
    r = Recording()
    for i in range(128):
        r.gate(AND, 1000 + i, 2 * i, 2 * i + 1)
    for g in range(8):
        r.lin(2000 + g, [(1000 + 16 * g + t, 2) for t in range(16)])
    r.lin(3000, [(2000 + g, 1) for g in range(8)], c0=1 << 30)
    out = plan(L, r)
    # one plan holds all of it (the entry returns one level sequence: nothing forced the recording to be cut)
    assert out["depth"] == 1 and out["levels"] == [1] * 137 and out["rotations"] == 128
    assert out["ranks"][128:] == [0] * 8 + [1]
    assert [(a, b, len(ds)) for a, b, ds in out["launches"]] == [(1, 0, 8), (1, 1, 1)]


def test_ranks_follow_the_levels_the_balancer_really_gives(L):
    """Random DAGs through the slack-aware balancer (unit 1, so it is active): whatever levels come out, an op runs
    after everything it reads -- a later level, or for two linear ops of one level a higher rank -- and a gate runs a
    level after a linear result it reads."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        r = Recording()
        made, kind_of = list(range(4)), {}
        for i in range(40):
            dst = 100 + i
            if rng.random() < 0.4:
                terms = [(int(rng.choice(made)), int(rng.integers(-3, 4))) for _ in range(int(rng.integers(1, 6)))]
                r.lin(dst, terms)
                kind_of[dst] = (LIN, [t[0] for t in terms])
            else:
                a, b = (int(x) for x in rng.choice(made, 2))
                r.gate(AND, dst, a, b)
                kind_of[dst] = (AND, [a, b])
            made.append(dst)
        out = plan(L, r, unit=1, balance=1, reuse=0)
        level = {100 + i: out["levels"][i] for i in range(40)}
        rank = {100 + i: out["ranks"][i] for i in range(40)}
        for dst, (kind, srcs) in kind_of.items():
            for s in srcs:
                if s < 100:
                    continue
                if kind == AND:
                    assert level[dst] > level[s], (trial, dst, s)
                elif kind_of[s][0] == AND:
                    assert level[dst] >= level[s], (trial, dst, s)
                else:
                    assert level[dst] > level[s] or (level[dst] == level[s] and rank[dst] > rank[s]), (trial, dst, s)
        # the launches hold every linear op once, in (level, rank) order
        order = [(a, b) for a, b, _ in out["launches"]]
        assert order == sorted(set(order))
        assert sorted(d[0] for _, _, ds in out["launches"] for d in ds) == sorted(d for d, k in kind_of.items() if k[0] == LIN)


def test_stats_end_with_the_two_new_counters(api):
    """The two counters were appended at the END of TfheHipStats as it was then: behind everything the mirror held before,
    8 bytes each.  What was appended since (the key-switch form counters) stands behind them in turn, at the new end."""
    from peba1_amd import lib
    ks = ["ks_pergate_launches", "ks_strip_launches", "ks_index_launches"]
    assert lib.STATS_FIELDS[-6:] == ["multi_outputs", "lincomb_ops", "lincomb_launches"] + ks and lib.STATS_FIELDS[2] == "linear_ops"
    assert len(set(lib.STATS_FIELDS)) == len(lib.STATS_FIELDS)
    assert lib.StatsAll.lincomb_ops.offset == C.sizeof(lib.Stats) == 8 * len(lib.Stats._fields_)
    assert lib.StatsAll.lincomb_launches.offset == C.sizeof(lib.Stats) + 8 and C.sizeof(lib.StatsAll) == 8 * len(lib.STATS_FIELDS)
    assert lib.StatsAll.multi_outputs.offset == C.sizeof(lib.Stats) - 8
    assert [getattr(lib.StatsAll, f).offset for f in ks] == [C.sizeof(lib.Stats) + 16 + 8 * i for i in range(3)]
    s = api.stats()                                    # reads the whole struct, without a device
    assert list(s) == lib.STATS_FIELDS and s["lincomb_ops"] == 0 == s["lincomb_launches"]
    assert all(s[f] == 0 for f in ks)


# ---- refusals that need no device -------------------------------------------------------------------------------------
def _foreign_sample(n):
    from peba1_amd import lib
    buf = np.zeros(n + 16, dtype=np.int32)
    s = lib.LweSample()
    s.a = C.cast(buf.ctypes.data + 8 * 4, C.POINTER(C.c_int32))
    s.slot = 5
    return s, buf


def test_refusals_set_the_message_and_leave_the_result_untouched(api, L):
    """Refused before the key is touched: with a host-only keyset nothing reaches a GPU.  (Pool exhaustion needs one:
    tests/test_gpu_linear.py.)"""
    from peba1_amd import lib
    pp, p80 = api.ParameterSet(128), api.ParameterSet(80)
    ks = api.SecretKeySet(pp, 11, device=False)
    L.tfhe_hip_set_encrypt_seed(3)
    r = api.CiphertextArray(pp, 1).encrypt([1], ks)
    a = api.CiphertextArray(pp, 17).encrypt([0] * 17, ks)
    small = api.CiphertextArray(p80, 1)
    foreign, keep = _foreign_sample(pp.n)
    LS = lib.LS
    before = (r.at(0).contents.slot, r.words().copy())
    ones = np.ones(17, dtype=I32)
    ins = (LS * 17)(*[a.at(i) for i in range(17)])
    with_null = (LS * 17)(a.at(0), None, a.at(2))
    with_foreign = (LS * 17)(a.at(0), C.pointer(foreign))
    with_small = (LS * 17)(a.at(0), small.at(0))
    rows = ((r.at(0), 0, ins, p(ones), ks.cloud, "nin must be 1..16"),
            (r.at(0), 17, ins, p(ones), ks.cloud, "nin must be 1..16"),
            (r.at(0), -1, ins, p(ones), ks.cloud, "nin must be 1..16"),
            (None, 2, ins, p(ones), ks.cloud, "null result"),
            (r.at(0), 2, None, p(ones), ks.cloud, "null operand or coefficient list"),
            (r.at(0), 2, ins, None, ks.cloud, "null operand or coefficient list"),
            (r.at(0), 3, with_null, p(ones), ks.cloud, "null operand"),
            (r.at(0), 2, ins, p(ones), None, "null cloud key"),
            (r.at(0), 2, with_foreign, p(ones), ks.cloud, "not allocated by new_gate_bootstrapping_ciphertext_array"),
            (C.pointer(foreign), 2, ins, p(ones), ks.cloud, "not allocated by new_gate_bootstrapping_ciphertext_array"),
            (r.at(0), 2, with_small, p(ones), ks.cloud, "different LWE dimension"),
            (small.at(0), 2, ins, p(ones), ks.cloud, "different LWE dimension"))
    for res, nin, operands, coefs, bk, match in rows:
        L.tfhe_hip_clear_error()
        L.tfhe_hip_linear(res, nin, operands, coefs, 5, bk)
        assert match in api.last_error(), (match, api.last_error())
        assert r.at(0).contents.slot == before[0] and (r.words() == before[1]).all()
        assert foreign.slot == 5 and not keep.any() and small.at(0).contents.slot == -2
    # the batch form: in[k] are arrays; the same refusals, -1
    arrays = (LS * 17)(*[a.ptr] * 17)
    for res, nin, operands, coefs, bk, match in ((r.ptr, 0, arrays, p(ones), ks.cloud, "nin must be 1..16"),
                                                 (r.ptr, 17, arrays, p(ones), ks.cloud, "nin must be 1..16"),
                                                 (None, 1, arrays, p(ones), ks.cloud, "null result"),
                                                 (r.ptr, 2, (LS * 17)(a.ptr, None), p(ones), ks.cloud, "null operand"),
                                                 (r.ptr, 2, arrays, None, ks.cloud, "null operand or coefficient list"),
                                                 (r.ptr, 1, arrays, p(ones), None, "null cloud key"),
                                                 (r.ptr, 2, (LS * 17)(a.ptr, small.ptr), p(ones), ks.cloud, "different LWE dimension"),
                                                 (r.ptr, 2, (LS * 17)(a.ptr, C.pointer(foreign)), p(ones), ks.cloud, "not allocated")):
        L.tfhe_hip_clear_error()
        assert L.tfhe_hip_linear_batch(res, nin, operands, coefs, 5, 1, bk) == -1
        assert match in api.last_error(), (match, api.last_error())
        assert r.at(0).contents.slot == before[0] and (r.words() == before[1]).all()
    L.tfhe_hip_clear_error()
    ks.close()


# ---- encrypt and phase --------------------------------------------------------------------------------------------------
def _sets(api):
    return {"P128": api.ParameterSet(128), "P80": api.ParameterSet(80), "P2048": api.ParameterSet(p2048=True)}


def test_encrypt_torus_at_one_eighth_is_boots_sym_encrypt(api, L):
    for pname, pp in _sets(api).items():
        ks = api.SecretKeySet(pp, 21, device=False)
        bits = [1, 0, 0, 1, 1]
        L.tfhe_hip_set_encrypt_seed(99)
        want = api.CiphertextArray(pp, len(bits)).encrypt(bits, ks).words()
        L.tfhe_hip_set_encrypt_seed(99)
        got = api.CiphertextArray(pp, len(bits))
        for i, b in enumerate(bits):
            api.encrypt_torus(got.at(i), (1 << 29) if b else -(1 << 29), ks)
        assert api.last_error() == ""
        assert (got.words() == want).all(), pname
        assert got.decrypt(ks).tolist() == bits
        ks.close()


def test_phase_of_an_encryption_of_mu_is_mu_within_two_to_the_minus_ten(api, L):
    """The built-in sets encrypt with a deviation of at most 2^-15: 2^-10 is over 30 deviations."""
    rng = np.random.default_rng(8)
    mus = [0, 1 << 29, -(1 << 29), INT32_MIN, (1 << 31) - 1, 1 << 28, 3 << 28, 5 << 28] + \
        rng.integers(-2 ** 31, 2 ** 31, 24).tolist()
    for pname, pp in _sets(api).items():
        ks = api.SecretKeySet(pp, 22, device=False)
        L.tfhe_hip_set_encrypt_seed(100)
        ct = api.CiphertextArray(pp, len(mus))
        key = ks.lwe_key().astype(np.int64)
        for i, mu in enumerate(mus):
            api.encrypt_torus(ct.at(i), mu, ks)
            ph = api.phase(ct.at(i), ks)
            diff = ((ph - mu + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
            assert abs(diff) < (1 << 22), (pname, mu, ph)                  # 2^-10 of the torus = 2^22
            w = ct.words()[i].astype(np.int64)
            want = int((w[-1] - w[:-1] @ key) & 0xFFFFFFFF)
            assert ph & 0xFFFFFFFF == want                                   # and exactly b - <a, s>
        assert api.last_error() == ""
        # the refusals: a null key, a foreign sample
        foreign, _ = _foreign_sample(pp.n)
        for call, match in ((lambda: L.tfhe_hip_sym_phase(ct.at(0), None), "null key"),
                            (lambda: L.tfhe_hip_sym_encrypt_torus(ct.at(0), 1, None), "null key"),
                            (lambda: L.tfhe_hip_sym_phase(C.pointer(foreign), ks.ptr), "not allocated"),
                            (lambda: L.tfhe_hip_sym_encrypt_torus(C.pointer(foreign), 1, ks.ptr), "not allocated")):
            L.tfhe_hip_clear_error()
            assert not call() and match in api.last_error()
        L.tfhe_hip_clear_error()
        ks.close()
