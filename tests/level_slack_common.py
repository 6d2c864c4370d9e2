"""For tests/test_level_slack_cpu.py: random DAGs in the 5-word record form of
tfhe_hip_test_schedule, the cost-table entries, and a restatement of the table's interpolation.

`python tests/level_slack_common.py` records tests/golden/level_slack_parent_levels.npz: the levels
tfhe_hip_test_schedule(balance = 1, unit = UNIT) gives every DAG of SEEDS.  The committed file was recorded at the commit
before the cost-driven pass existed, through that same entry."""
import ctypes as C
import os

import numpy as np

NOT, MUX = 17, 16
UNIT = 8
SEEDS = range(200)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level_slack_parent_levels.npz")


def random_dag(seed):
    """50 .. 2,000 ops: 5 % NOTs (never of a NOT's result: the recorder aliases those), 8 % MUXes (two rotations), none, 20 % or
    50 % gates of two old operands (early ASAP level, often unused: slack), and two-input gates whose first operand is one of
    the last `window` results (the window decides between deep and wide)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 2001))
    window = int(rng.choice([3, 12, 40, 400]))
    free = float(rng.choice([0.0, 0.2, 0.5]))
    ninputs = 8
    kind_draw, gate_kind = rng.random(n), rng.integers(0, 10, n)
    back, anywhere = rng.integers(0, 1 << 30, n), rng.integers(0, 1 << 30, (n, 3))
    is_not_out = np.zeros(ninputs + n, dtype=bool)
    ops = np.full((n, 5), -1, dtype=np.int32)
    for i in range(n):
        have, dst = ninputs + i, ninputs + i
        if kind_draw[i] < 0.05:
            src = int(anywhere[i, 0] % have)
            while is_not_out[src]:
                src = (src + 1) % have                                  # slot 0 is an input: the walk ends
            ops[i] = (NOT, dst, src, -1, -1)
            is_not_out[dst] = True
        elif kind_draw[i] < 0.13:
            ops[i] = (MUX, dst, anywhere[i, 0] % have, anywhere[i, 1] % have, anywhere[i, 2] % have)
        elif kind_draw[i] < 0.13 + free:
            early = max(ninputs, have // 4)                              # a gate of old operands: early ASAP level, slack
            ops[i] = (gate_kind[i], dst, anywhere[i, 0] % early, anywhere[i, 1] % early, -1)
        else:
            ops[i] = (gate_kind[i], dst, have - 1 - back[i] % min(have, window), anywhere[i, 1] % have, -1)
    return ops


def rotations(ops):
    return np.where(ops[:, 0] == MUX, 2, np.where(ops[:, 0] == NOT, 0, 1))


def parent_schedule(ops, unit=UNIT, balance=1):
    from peba1_amd import lib
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    out = np.zeros(len(ops), dtype=np.int32)
    depth = lib.load().tfhe_hip_test_schedule(ops.ctypes.data_as(lib.I32P), len(ops), unit, balance, out.ctypes.data_as(lib.I32P))
    return depth, out


def level_slack(ops, table, level_slack=1, unit=UNIT, period=0):
    """tfhe_hip_test_level_slack: (depth, level of every op, rotations per level [depth + 1], sum of the levels' costs,
    the same sum for the levels without the pass).  table = [(width, cost), ...], widths ascending."""
    from peba1_amd import lib
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    w = np.ascontiguousarray([t[0] for t in table], dtype=np.int32)
    c = np.ascontiguousarray([t[1] for t in table], dtype=np.float64)
    lvl = np.zeros(len(ops), dtype=np.int32)
    widths = np.zeros(len(ops) + 2, dtype=np.int32)
    cost = np.zeros(2, dtype=np.float64)
    depth = lib.load().tfhe_hip_test_level_slack(ops.ctypes.data_as(lib.I32P), len(ops), unit, level_slack,
                                                 w.ctypes.data_as(lib.I32P), c.ctypes.data_as(C.POINTER(C.c_double)), len(w), period,
                                                 lvl.ctypes.data_as(lib.I32P), widths.ctypes.data_as(lib.I32P),
                                                 cost.ctypes.data_as(C.POINTER(C.c_double)))
    assert depth >= 0, lib.load().tfhe_hip_last_error()
    return depth, lvl, widths[:depth + 1].copy(), float(cost[0]), float(cost[1])


def table_cost(table, width, period=0):
    """launch_plan.hpp level_cost_at, restated: 0 for an empty level, the first entry below it, linear between entries;
    beyond the table the last segment's slope (period 0), or the last `period` rotations again and again."""
    if width <= 0:
        return 0.0
    ws, cs = [t[0] for t in table], [float(t[1]) for t in table]
    if width <= ws[0] or len(ws) == 1:
        return cs[0]
    if width > ws[-1] and 0 < period <= ws[-1] - ws[0]:
        fold = -((ws[-1] - width) // period)
        return table_cost(table, width - fold * period) + fold * (cs[-1] - table_cost(table, ws[-1] - period))
    j = min(int(np.searchsorted(ws, width, side="left")), len(ws) - 1)
    return cs[j - 1] + (cs[j] - cs[j - 1]) * (width - ws[j - 1]) / (ws[j] - ws[j - 1])


def compiled_cost(width, cus=256, params=(630, 1024, 1, 3, 7, 8, 2)):
    """tfhe_hip_test_level_cost: launch_plan.hpp level_cost_us under the default tunings; -1 = no table"""
    from peba1_amd import lib
    us = C.c_double(0)
    assert lib.load().tfhe_hip_test_level_cost(*params, cus, width, C.byref(us)) == 0
    return us.value


def check_levels(ops, lvl, depth):
    """Every gate after all its inputs, a NOT on its operand's level, every level within the depth."""
    producer = {}
    for i, (kind, dst, a, b, c) in enumerate(ops.tolist()):
        for s in (a, b, c):
            p = producer.get(s)
            if p is None:
                continue
            if kind == NOT:
                assert lvl[i] == lvl[p], (i, p)
            else:
                assert lvl[i] > lvl[p], (i, p, lvl[i], lvl[p])
        producer[dst] = i
        assert (0 if kind == NOT else 1) <= lvl[i] <= depth, (i, lvl[i])


if __name__ == "__main__":
    levels = [parent_schedule(random_dag(s))[1].astype(np.int16) for s in SEEDS]
    np.savez_compressed(GOLDEN, offsets=np.cumsum([0] + [len(x) for x in levels]).astype(np.int64), levels=np.concatenate(levels))
    print("recorded", GOLDEN, os.path.getsize(GOLDEN), "bytes")
