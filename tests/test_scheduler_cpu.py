"""Host logic of the deferred executor (peba1_amd/csrc/scheduler.cpp), no GPU: the slack-aware
levelisation must respect every dependency, keep the DAG's depth, and flatten a
"fat head + narrow tail" DAG of the kind the reference's Function_f produces."""
import numpy as np
import pytest

NOT, MUX = 17, 16


def schedule(ops, unit, balance):
    from peba1_amd import lib
    a = np.ascontiguousarray(np.array(ops, dtype=np.int32).reshape(-1, 5))
    out = np.zeros(len(a), dtype=np.int32)
    depth = lib.load().tfhe_hip_test_schedule(a.ctypes.data_as(lib.I32P), len(a), unit, 1 if balance else 0,
                                              out.ctypes.data_as(lib.I32P))
    return depth, out


def check_valid(ops, lvl, depth):
    producer = {}
    for i, (kind, dst, a, b, c) in enumerate(ops):
        for s in (a, b, c):
            if s in producer:
                p = producer[s]
                if kind == NOT:
                    assert lvl[i] == lvl[p], (i, p)            # a NOT rides on its operand's level
                else:
                    assert lvl[i] > lvl[p] or (ops[p][0] == NOT and lvl[i] > lvl[p]), (i, p, lvl[i], lvl[p])
        producer[dst] = i
        if kind != NOT:
            assert 1 <= lvl[i] <= depth
        else:
            assert 0 <= lvl[i] <= depth


def random_dag(rng, n, ninputs):
    ops, next_slot = [], ninputs
    avail = list(range(ninputs))
    not_outputs = set()
    for _ in range(n):
        r = rng.random()
        if r < 0.05:
            # the recorder never chains NOT on a pending NOT (it aliases the original operand)
            src = int(rng.choice([s for s in avail if s not in not_outputs]))
            ops.append((NOT, next_slot, src, -1, -1))
            not_outputs.add(next_slot)
        elif r < 0.10:
            a, b, c = (int(x) for x in rng.choice(avail, 3))
            ops.append((MUX, next_slot, a, b, c))
        else:
            # bias towards recent values to get depth
            a = int(avail[-1 - int(rng.integers(0, min(len(avail), 40)))])
            b = int(rng.choice(avail))
            ops.append((int(rng.integers(0, 10)), next_slot, a, b, -1))
        avail.append(next_slot)
        next_slot += 1
    return ops


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_dags_respect_dependencies_and_depth(seed):
    rng = np.random.default_rng(seed)
    ops = random_dag(rng, 3000, 16)
    d0, asap = schedule(ops, 8, False)
    d1, bal = schedule(ops, 8, True)
    assert d0 == d1
    check_valid(ops, asap, d0)
    check_valid(ops, bal, d1)
    assert bal.max() == d1


def head_and_tail_dag(nslots=48, head_depth=6, head_width=20):
    """`nslots` independent fat sub-circuits whose results feed a serial accumulation chain:
    ASAP puts every sub-circuit in the first levels and leaves a narrow tail."""
    ops, slot = [], 100
    results = []
    for _ in range(nslots):
        prev = [0, 1]
        for _ in range(head_depth):
            cur = []
            for w in range(head_width):
                ops.append((2, slot, prev[w % len(prev)], prev[(w + 1) % len(prev)], -1))
                cur.append(slot)
                slot += 1
            prev = cur
        results.append(prev[0])
    acc = results[0]
    for k in range(1, nslots):
        for _ in range(3):                      # 3 serial gates per accumulated slot
            ops.append((4, slot, acc, results[k], -1))
            acc = slot
            slot += 1
    return ops


def test_fat_head_narrow_tail_is_flattened():
    ops = head_and_tail_dag()
    unit = 64
    d0, asap = schedule(ops, unit, False)
    d1, bal = schedule(ops, unit, True)
    assert d0 == d1 == 6 + 3 * 47
    check_valid(ops, bal, d1)
    w_asap = np.bincount(asap, minlength=d0 + 1)
    w_bal = np.bincount(bal, minlength=d1 + 1)
    assert w_asap.max() == 48 * 20                       # everything at once
    assert w_bal.max() <= 4 * unit + 1                   # filled to at most the 4-unit width
    # the tail is no longer almost empty: far fewer nearly idle levels
    assert (w_bal[1:] <= 2).sum() < (w_asap[1:] <= 2).sum() // 2


def test_small_flushes_keep_asap_levels():
    ops = [(2, 10, 0, 1, -1), (4, 11, 10, 1, -1), (NOT, 12, 11, -1, -1), (MUX, 13, 12, 0, 1)]
    d, lvl = schedule(ops, 256, True)
    assert d == 3 and list(lvl) == [1, 2, 2, 3]


# ---- the level plan of a multi-key flush (scheduler.cpp build_level_plan, nkeys > 1) --------------------------------

# prelude constants of the two-input gates, (c0 in eighths, sa, sb) in gate-code order NAND OR AND NOR XOR XNOR ANDNY
# ANDYN ORNY ORYN: tfhe's boot-gates.cpp, restated here so that the single-key plan has a reference of its own
GATE_LIN = [(1, -1, -1), (1, 1, 1), (-1, 1, 1), (-1, -1, -1), (2, 2, 2), (-2, -2, -2),
            (-1, -1, 1), (-1, 1, -1), (1, -1, 1), (1, 1, -1)]
MU = 1 << 29


def level_plan(ops, keys, nkeys, unit=8, balance=False):
    from types import SimpleNamespace
    from peba1_amd import lib
    n = len(ops)
    a = np.ascontiguousarray(np.array(ops, dtype=np.int32).reshape(-1, 5))
    k = np.ascontiguousarray(np.array(keys, dtype=np.int32))
    assert len(k) == n
    buf = {name: np.full(size, -12345, dtype=np.int32) for name, size in (
        ("lvl", n), ("sizes", 6), ("rot_off", n + 1), ("ks_off", n + 1), ("rot_koff", n * nkeys + 1),
        ("ks_koff", n * nkeys + 1), ("rot_key", 2 * n), ("rots", 12 * n), ("kss", 4 * n))}
    p = lambda name: buf[name].ctypes.data_as(lib.I32P)
    levels = lib.load().tfhe_hip_test_level_plan(
        a.ctypes.data_as(lib.I32P), k.ctypes.data_as(lib.I32P), n, nkeys, unit, 1 if balance else 0, p("lvl"), p("sizes"),
        p("rot_off"), p("ks_off"), p("rot_koff"), p("ks_koff"), p("rot_key"), p("rots"), p("kss"))
    assert levels >= 0
    lv, nrot, nks, n_rkoff, n_kkoff, n_rkey = (int(x) for x in buf["sizes"])
    assert lv == levels
    return SimpleNamespace(
        levels=levels, lvl=buf["lvl"], rot_off=buf["rot_off"][:levels + 1], ks_off=buf["ks_off"][:levels + 1],
        rot_koff=buf["rot_koff"][:n_rkoff], ks_koff=buf["ks_koff"][:n_kkoff], rot_key=buf["rot_key"][:n_rkey],
        rots=buf["rots"][:6 * nrot].reshape(-1, 6), kss=buf["kss"][:4 * nks].reshape(-1, 4))


def reference_plan(ops, keys, nkeys, lvl, levels):
    """The plan restated: gates in the order (level, key, recording order), a MUX as two adjacent rotations; u_index /
    u0 / u1 count from the level's first rotation."""
    order = sorted((i for i, op in enumerate(ops) if op[0] != NOT), key=lambda i: (lvl[i], keys[i], i))
    rots, kss, rot_key = [], [], []
    rot_off, ks_off = [0] * (levels + 1), [0] * (levels + 1)
    rot_koff, ks_koff = [0] * (levels * nkeys + 1), [0] * (levels * nkeys + 1)
    for i in order:
        kind, dst, a, b, c = ops[i]
        rot_off[lvl[i]] += 2 if kind == MUX else 1
        ks_off[lvl[i]] += 1
        rot_koff[(lvl[i] - 1) * nkeys + keys[i] + 1] += 2 if kind == MUX else 1
        ks_koff[(lvl[i] - 1) * nkeys + keys[i] + 1] += 1
    for off in (rot_off, ks_off, rot_koff, ks_koff):
        for j in range(1, len(off)):
            off[j] += off[j - 1]
    for i in order:
        kind, dst, a, b, c = ops[i]
        u = len(rots) - rot_off[lvl[i] - 1]
        if kind == MUX:
            rots += [(a, b, 1, 1, -MU, u), (a, c, -1, 1, -MU, u + 1)]
            kss.append((u, u + 1, MU, dst))
            rot_key += [keys[i]] * 2
        else:
            c8, sa, sb = GATE_LIN[kind]
            rots.append((a, b, sa, sb, c8 * MU, u))
            kss.append((u, -1, 0, dst))
            rot_key.append(keys[i])
    i32 = lambda x, cols: np.array(x, dtype=np.int32).reshape(-1, cols)
    return i32(rots, 6), i32(kss, 4), i32(rot_key, 1)[:, 0], i32(rot_off, 1)[:, 0], i32(ks_off, 1)[:, 0], \
        i32(rot_koff, 1)[:, 0], i32(ks_koff, 1)[:, 0]


def keyed_dag(seed, nkeys, sizes, ninputs=8):
    """One random_dag per key on slots of its own (slot s of key k is s * nkeys + k), interleaved at random: the key
    changes from op to op, every op reads values of its own key only.  sizes[k] = ops of key k (0: the key owns none)."""
    rng = np.random.default_rng(seed)
    per_key = []
    for k in range(nkeys):
        dag = random_dag(rng, sizes[k], ninputs) if sizes[k] else []
        m = lambda s, k=k: s * nkeys + k if s >= 0 else -1
        per_key.append([(kind, m(dst), m(a), m(b), m(c)) for kind, dst, a, b, c in dag])
    ops, keys, pos = [], [], [0] * nkeys
    left = [k for k in range(nkeys) if sizes[k]]
    while left:
        k = int(rng.choice(left))
        ops.append(per_key[k][pos[k]])
        keys.append(k)
        pos[k] += 1
        if pos[k] == sizes[k]:
            left.remove(k)
    return ops, keys


def gate_contents(plan, g):
    """Per key switch of level g (0-based): what its gate computes, without any position -- (dst, add_b, its rotations'
    (slot_a, slot_b, sa, sb, c0))."""
    out = []
    for j in range(plan.ks_off[g], plan.ks_off[g + 1]):
        u0, u1, add_b, dst = (int(x) for x in plan.kss[j])
        rr = [tuple(int(x) for x in plan.rots[plan.rot_off[g] + u][:5]) for u in (u0, u1) if u >= 0]
        out.append((dst, add_b, tuple(rr)))
    return out


def check_keyed_plan(ops, keys, K, plan):
    """The properties a multi-key level plan must have, from the ops alone."""
    n_gates = sum(1 for op in ops if op[0] != NOT)
    n_rots = sum(2 if op[0] == MUX else 1 for op in ops if op[0] != NOT)
    assert len(plan.kss) == n_gates and len(plan.rots) == n_rots
    assert len(plan.rot_off) == len(plan.ks_off) == plan.levels + 1
    assert plan.rot_off[0] == 0 and plan.rot_off[-1] == n_rots and plan.ks_off[0] == 0 and plan.ks_off[-1] == n_gates
    assert len(plan.rot_koff) == len(plan.ks_koff) == plan.levels * K + 1 and len(plan.rot_key) == n_rots
    by_dst = {op[1]: i for i, op in enumerate(ops)}
    assert len(by_dst) == len(ops)
    rot_owner = [-1] * n_rots
    seen_gate = set()
    for g in range(plan.levels):
        # the per-key runs tile the level, in key order
        for koff, off in ((plan.rot_koff, plan.rot_off), (plan.ks_koff, plan.ks_off)):
            assert koff[g * K] == off[g] and koff[(g + 1) * K] == off[g + 1], g
            assert (np.diff(koff[g * K:(g + 1) * K + 1]) >= 0).all(), g
        width = int(plan.rot_off[g + 1] - plan.rot_off[g])
        for k in range(K):
            r_lo, r_hi = int(plan.rot_koff[g * K + k]), int(plan.rot_koff[g * K + k + 1])
            assert (plan.rot_key[r_lo:r_hi] == k).all(), (g, k)
            for j in range(int(plan.ks_koff[g * K + k]), int(plan.ks_koff[g * K + k + 1])):
                u0, u1, add_b, dst = (int(x) for x in plan.kss[j])
                i = by_dst[dst]
                kind, _, a, b, c = ops[i]
                assert kind != NOT and i not in seen_gate          # every gate exactly one key switch
                seen_gate.add(i)
                assert keys[i] == k and plan.lvl[i] == g + 1, (g, k, j)
                # it reads extracted samples of its own level, produced by rotations of its own key's run
                us = [u0, u1] if kind == MUX else [u0]
                assert (u1 == u0 + 1) if kind == MUX else (u1 == -1), (g, k, j)
                for u in us:
                    assert 0 <= u < width
                    r = int(plan.rot_off[g]) + u
                    assert r_lo <= r < r_hi, (g, k, j, u)
                    assert int(plan.rots[r][5]) == u              # the rotation writes the sample the key switch reads
                    assert rot_owner[r] == -1
                    rot_owner[r] = i
                want = [(a, b), (a, c)] if kind == MUX else [(a, b)]
                assert [tuple(int(x) for x in plan.rots[int(plan.rot_off[g]) + u][:2]) for u in us] == want
    assert len(seen_gate) == n_gates and min(rot_owner, default=0) >= 0
    # rot_key[r] is the key of the op that owns rotation r, for every r
    assert [int(x) for x in plan.rot_key] == [keys[i] for i in rot_owner]


KEYED_CASES = [(seed, K) for seed in (0, 1, 2) for K in (1, 2, 3, 16)]


@pytest.mark.parametrize("balance", [False, True])
@pytest.mark.parametrize("seed,K", KEYED_CASES)
def test_level_plan_groups_every_level_by_key(seed, K, balance):
    rng = np.random.default_rng(1000 + seed)
    sizes = [int(x) for x in rng.integers(40, 1600 // K + 41, K)]
    ops, keys = keyed_dag(seed, K, sizes)
    plan = level_plan(ops, keys, K, unit=8, balance=balance)
    depth, lvl = schedule(ops, 8, balance)
    assert plan.levels == depth and (plan.lvl == lvl).all()       # the keys do not enter the levelisation
    check_valid(ops, plan.lvl, depth)
    ref = reference_plan(ops, keys, K, [int(x) for x in plan.lvl], plan.levels)
    one = level_plan(ops, [0] * len(ops), 1, unit=8, balance=balance)
    assert len(one.rot_key) == len(one.rot_koff) == len(one.ks_koff) == 0     # one key: no key tables at all
    if K == 1:
        # the single-key plan, byte for byte: against the restated rule (counting sort by level in recording order)
        for got, want in zip((plan.rots, plan.kss, plan.rot_off, plan.ks_off), (ref[0], ref[1], ref[3], ref[4])):
            assert got.tobytes() == want.tobytes()
        for got, want in zip((plan.rots, plan.kss, plan.rot_off, plan.ks_off, plan.rot_key, plan.rot_koff, plan.ks_koff),
                             (one.rots, one.kss, one.rot_off, one.ks_off, one.rot_key, one.rot_koff, one.ks_koff)):
            assert got.tobytes() == want.tobytes()
        return
    check_keyed_plan(ops, keys, K, plan)
    for got, want in zip((plan.rots, plan.kss, plan.rot_key, plan.rot_off, plan.ks_off, plan.rot_koff, plan.ks_koff), ref):
        assert got.tobytes() == want.tobytes()
    # grouping by key moves gates inside their level and changes nothing else: same offsets, same gates per level
    assert (plan.rot_off == one.rot_off).all() and (plan.ks_off == one.ks_off).all()
    for g in range(plan.levels):
        assert sorted(gate_contents(plan, g)) == sorted(gate_contents(one, g)), g


@pytest.mark.parametrize("seed,K", [(0, 2), (1, 3), (2, 16)])
def test_level_plan_relabelled_keys_permute_the_runs(seed, K):
    sizes = [60 + 25 * k for k in range(K)]
    ops, keys = keyed_dag(seed, K, sizes)
    perm = [int(x) for x in np.random.default_rng(77 + seed).permutation(K)]
    if perm == list(range(K)):
        perm = perm[1:] + perm[:1]
    a = level_plan(ops, keys, K)
    b = level_plan(ops, [perm[k] for k in keys], K)
    check_keyed_plan(ops, [perm[k] for k in keys], K, b)
    assert (a.lvl == b.lvl).all() and (a.rot_off == b.rot_off).all() and (a.ks_off == b.ks_off).all()

    def run(plan, g, k):      # the gates of key k's run at level g, in run order, without positions
        out = []
        for j in range(int(plan.ks_koff[g * K + k]), int(plan.ks_koff[g * K + k + 1])):
            u0, u1, add_b, dst = (int(x) for x in plan.kss[j])
            out.append((dst, add_b, tuple(tuple(int(x) for x in plan.rots[int(plan.rot_off[g]) + u][:5]) for u in (u0, u1) if u >= 0)))
        return out

    for g in range(a.levels):
        assert sorted(gate_contents(a, g)) == sorted(gate_contents(b, g)), g
        for k in range(K):
            assert run(a, g, k) == run(b, g, perm[k]), (g, k)
            assert a.rot_koff[g * K + k + 1] - a.rot_koff[g * K + k] == b.rot_koff[g * K + perm[k] + 1] - b.rot_koff[g * K + perm[k]]


def test_level_plan_with_a_key_that_owns_no_op():
    ops, keys = keyed_dag(5, 3, [300, 0, 200])
    assert 1 not in keys
    for balance in (False, True):
        plan = level_plan(ops, keys, 3, unit=8, balance=balance)
        check_keyed_plan(ops, keys, 3, plan)
        for g in range(plan.levels):
            assert plan.rot_koff[3 * g + 1] == plan.rot_koff[3 * g + 2] and plan.ks_koff[3 * g + 1] == plan.ks_koff[3 * g + 2]
        ref = reference_plan(ops, keys, 3, [int(x) for x in plan.lvl], plan.levels)
        for got, want in zip((plan.rots, plan.kss, plan.rot_key, plan.rot_off, plan.ks_off, plan.rot_koff, plan.ks_koff), ref):
            assert got.tobytes() == want.tobytes()


def test_level_plan_when_one_keys_circuit_ends_early():
    """Key 0: three levels (4 gates, a MUX of three of them, one more gate); key 1: a NOT and one gate; key 2: a chain of
    six.  Key 1 has no share from level 2 on, levels 4..6 hold key 2 alone: the empty runs have zero length in place."""
    ops = [(2, 100, 0, 1, -1), (4, 200, 20, 21, -1), (NOT, 110, 10, -1, -1), (1, 101, 1, 2, -1), (7, 201, 200, 20, -1),
           (5, 102, 2, 3, -1), (1, 111, 110, 11, -1), (0, 103, 3, 0, -1), (4, 202, 201, 21, -1), (MUX, 104, 100, 101, 102),
           (4, 203, 202, 20, -1), (9, 204, 203, 21, -1), (3, 205, 204, 20, -1), (6, 105, 103, 104, -1)]
    keys = [0, 2, 1, 0, 2, 0, 1, 0, 2, 0, 2, 2, 2, 0]
    plan = level_plan(ops, keys, 3, unit=256, balance=True)
    assert plan.levels == 6
    check_keyed_plan(ops, keys, 3, plan)
    assert list(np.diff(plan.rot_off)) == [6, 3, 2, 1, 1, 1] and list(np.diff(plan.ks_off)) == [6, 2, 2, 1, 1, 1]
    assert list(np.diff(plan.rot_koff)) == [4, 1, 1, 2, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
    assert list(np.diff(plan.ks_koff)) == [4, 1, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
    assert list(plan.rot_key) == [0, 0, 0, 0, 1, 2, 0, 0, 2, 0, 2, 2, 2, 2]
    # the MUX: two adjacent rotations under key 0, first of level 2
    assert [tuple(r) for r in plan.rots[6:8]] == [(100, 101, 1, 1, -MU, 0), (100, 102, -1, 1, -MU, 1)]
    assert tuple(plan.kss[6]) == (0, 1, MU, 104)


def test_level_plan_refuses_a_key_index_out_of_range():
    from peba1_amd import lib
    ops = [(2, 10, 0, 1, -1)]
    a = np.array(ops, dtype=np.int32)
    k = np.array([2], dtype=np.int32)
    z = [np.zeros(16, dtype=np.int32) for _ in range(9)]
    rc = lib.load().tfhe_hip_test_level_plan(a.ctypes.data_as(lib.I32P), k.ctypes.data_as(lib.I32P), 1, 2, 8, 0,
                                             *[x.ctypes.data_as(lib.I32P) for x in z])
    assert rc == -1
