"""The cost-driven levelling pass (peba1_amd/csrc/scheduler.cpp relevel_by_cost, tuning "level_slack") on the CPU, through
tfhe_hip_test_level_slack: a case worked by hand under a synthetic step table, and 200 random DAGs -- dependencies, depth,
the set of gates, the sum of costs never above the levels without the pass, and `level_slack` 0 giving the levels recorded
at the commit before the pass existed (tests/golden/level_slack_parent_levels.npz)."""
import numpy as np
import pytest

from level_slack_common import (GOLDEN, SEEDS, UNIT, check_levels, compiled_cost, level_slack, parent_schedule, random_dag,
                                rotations, table_cost)

# cost(w) = 3 for w <= 4, 4 for w <= 8 (then 5 for w <= 12): a step every four rotations
STEP_TABLE = [(1, 3.0), (4, 3.0), (5, 4.0), (8, 4.0), (9, 5.0), (12, 5.0)]


def chains_and_cloud():
    """Two chains of six gates (two gates on every level, none movable) and a cloud of eight gates of the inputs whose results
    nobody reads (movable anywhere)."""
    ops, slot = [], 10
    for chain in range(2):
        prev = chain
        for _ in range(6):
            ops.append((2, slot, prev, 2, -1))
            prev = slot
            slot += 1
    for g in range(8):
        ops.append((4, slot, g % 3, 3, -1))
        slot += 1
    return np.array(ops, dtype=np.int32)


def test_hand_worked_case_reaches_the_optimum():
    """Unit 5: the list scheduling fills 5, 5, 4, 2, 2, 2 -- two levels one gate past the step, 4 + 4 + 3 + 3 + 3 + 3 = 20.
    Every level holds its two chain gates, so no levelling costs less than 6 x 3 = 18; 4, 4, 4, 4, 2, 2 does cost 18, and
    the pass gets there by handing the surplus on from level to level."""
    ops = chains_and_cloud()
    depth, base, wbase, cbase, _ = level_slack(ops, STEP_TABLE, 0, unit=5)
    assert depth == 6 and list(wbase[1:]) == [5, 5, 4, 2, 2, 2] and cbase == 20.0
    depth1, lvl, widths, cost, cost_without = level_slack(ops, STEP_TABLE, 1, unit=5)
    assert depth1 == 6                                               # the depth is kept
    assert cost == 18.0 and cost_without == 20.0
    assert widths[1:].max() <= 4 and widths[1:].sum() == 20          # nothing lost, nothing twice
    assert list(lvl[:12]) == [1, 2, 3, 4, 5, 6] * 2                  # the chains stay
    check_levels(ops, lvl, depth)
    assert (lvl[12:] >= base[12:]).all() and (lvl != base).any()     # gates only ever move later


def test_no_table_and_no_gain_leave_the_levels_alone():
    ops = chains_and_cloud()
    _, base, _, _, _ = level_slack(ops, STEP_TABLE, 0, unit=5)
    assert (level_slack(ops, [], 1, unit=5)[1] == base).all()                        # unknown cost: as without the pass
    flat = [(1, 3.0), (64, 3.0)]                                                      # nothing to gain anywhere
    _, lvl, _, cost, without = level_slack(ops, flat, 1, unit=5)
    assert (lvl == base).all() and cost == without == 18.0


def one_level(width):
    return np.array([(2, 10 + i, 0, 1, -1) for i in range(width)], dtype=np.int32)


@pytest.mark.parametrize("period", [0, 8, 20])
def test_table_interpolation_through_the_c_entry(period):
    """One level of w gates: the entry's sum is level_cost_at(w).  Below the first entry, at entries, inside segments, and
    beyond the table with the last slope (period 0) or with the last `period` rotations repeated."""
    table = [(4, 2.0), (10, 3.0), (30, 7.0), (32, 8.5)]
    want = {1: 2.0, 4: 2.0, 7: 2.5, 10: 3.0, 20: 5.0, 30: 7.0, 31: 7.75, 32: 8.5}
    # cost(12) = 3.4, cost(13) = 3.6, cost(24) = 5.8, cost(25) = 6.0; a period adds cost(32) - cost(32 - period) each time
    want.update({0: {33: 9.25, 40: 14.5, 100: 59.5},                                  # the last slope, 0.75 a rotation
                 8: {33: 6.0 + 2.7, 40: 8.5 + 2.7, 41: 6.0 + 2 * 2.7},
                 20: {33: 3.6 + 5.1, 52: 8.5 + 5.1, 53: 3.6 + 2 * 5.1}}[period])
    for w, c in want.items():
        assert table_cost(table, w, period) == pytest.approx(c), w
        _, _, widths, cost, _ = level_slack(one_level(w), table, 0, unit=1, period=period)
        assert list(widths) == [0, w] and cost == pytest.approx(c), (w, period)


def test_levelling_under_a_periodic_table():
    """Widths beyond the table: under (two rounds, period = one round) the pass prices every level as the table continued
    by hand does (the folded branch of level_cost_at), takes its candidates from the shifted steps (level_cost_steps), and
    what it returns is a valid levelling that costs no more than before."""
    unit = 4
    one = [(1, 30.0), (unit, 31.0), (unit + 1, 48.0), (2 * unit, 50.0)]                  # one round: a dear first half
    base = one + [(w + 2 * unit, c + 50.0) for w, c in one]
    long = [(w + 2 * unit * k, c + 50.0 * k) for k in range(600) for w, c in one]
    changed = 0
    for seed in (4, 7, 9, 11, 1):
        ops = random_dag(seed)
        depth, lvl, widths, cost, without = level_slack(ops, base, 1, unit=unit, period=2 * unit)
        assert widths.max() > 4 * unit                                                   # past the table
        check_levels(ops, lvl, depth)
        assert (np.bincount(lvl, weights=rotations(ops), minlength=depth + 1).astype(np.int64) == widths).all()
        assert cost == pytest.approx(sum(table_cost(long, int(w)) for w in widths[1:]))
        _, _, w0, c0, _ = level_slack(ops, base, 0, unit=unit, period=2 * unit)
        assert without == pytest.approx(c0) == pytest.approx(sum(table_cost(long, int(w)) for w in w0[1:]))
        assert cost <= c0
        changed += cost < c0
    assert changed > 0


def measured_table():
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "level_cost_P128.json")) as f:
        t = json.load(f)
    us = [r["us"] for r in t["levels"]]
    for j in range(len(us) - 2, -1, -1):                 # tools/level_cost_inc.py: never dearer than a wider level
        us[j] = min(us[j], us[j + 1])
    return t, [(r["width"], u) for r, u in zip(t["levels"], us)]


def test_the_built_library_holds_the_measured_table_for_p128():
    """launch_plan.hpp level_cost_us through tfhe_hip_test_level_cost: the library as built has the table of
    profiles/level_cost_P128.json for P128 on 256 CUs under the default tunings -- its entries, linear between them, one
    512-rotation round repeated beyond 2,048 -- and none for another CU count or parameter set."""
    from peba1_amd.kernel_id import kernels_sha16
    t, table = measured_table()
    assert t["kernels_sha16"] == kernels_sha16(), "the table was measured on other kernels: tools/level_cost.py"
    assert t["cus"] == 256 and t["set"] == "P128"
    p = t["params"]
    params = (p["n"], p["N"], p["k"], p["l"], p["Bgbit"], p["ks_t"], p["ks_basebit"])
    assert compiled_cost(256, 256, params) > 0, "the library was built without level_cost_tables.inc"
    for w, us in table:
        assert compiled_cost(w, 256, params) == pytest.approx(us), w
    for w in (3, 100, 300, 700, 1500, 2040, 2049, 2083, 2304, 2560, 2561, 3000, 4053, 4096, 9000):
        assert compiled_cost(w, 256, params) == pytest.approx(table_cost(table, w, 512)), w
    top = dict(table)
    assert compiled_cost(2083, 256, params) == pytest.approx(table_cost(table, 1571) + top[2048] - top[1536])
    assert compiled_cost(0, 256, params) == 0.0
    for cus in (255, 128, 304):
        assert compiled_cost(512, cus, params) == -1.0
    assert compiled_cost(512, 256, (500,) + params[1:]) == -1.0                      # P80
    assert compiled_cost(512, 256, (1024, 2048, 1, 3, 6, 8, 2)) == -1.0              # another ring and gadget
    assert compiled_cost(512, 256, params[:5] + (4, 4)) == -1.0                      # another key switch


@pytest.fixture(scope="module")
def parent_levels():
    g = np.load(GOLDEN)
    return g["offsets"], g["levels"]


@pytest.mark.parametrize("block", range(8))
def test_random_dags(block, parent_levels):
    """25 seeds a case.  The table has the shape of the measured one, scaled to UNIT: a step at every multiple of UNIT, the
    odd ones (a narrow launch or a tail) dearer than the even ones, a small slope inside a step."""
    offsets, golden = parent_levels
    table = []
    for q in range(0, 40):
        base = 1000.0 * (q // 2) + (0 if q % 2 == 0 else 620.0)
        table += [(q * UNIT + 1, base + 620.0 if q % 2 == 0 else base + 380.0)]
        table += [((q + 1) * UNIT, table[-1][1] + 25.0)]
    moved_somewhere = 0
    for seed in list(SEEDS)[25 * block:25 * (block + 1)]:
        ops = random_dag(seed)
        rot = rotations(ops)
        depth0, base, wbase, cbase, _ = level_slack(ops, table, 0)
        want = golden[offsets[seed]:offsets[seed + 1]]
        assert len(want) == len(ops) and (base == want).all(), seed                  # level_slack 0: the parent's levels
        assert (parent_schedule(ops)[1] == base).all()
        depth, lvl, widths, cost, without = level_slack(ops, table, 1)
        assert depth == depth0 and lvl.max() == depth, seed
        check_levels(ops, lvl, depth)
        assert (np.bincount(lvl, weights=rot, minlength=depth + 1).astype(np.int64) == widths).all()   # every gate once
        assert widths.sum() == rot.sum()
        assert cost == pytest.approx(sum(table_cost(table, int(w)) for w in widths[1:]))
        assert without == pytest.approx(cbase) and cost <= cbase, seed
        if (lvl != base).any():
            assert cost < cbase, seed                                                # a change always pays
            moved_somewhere += 1
        _, again, _, _, _ = level_slack(ops, table, 1)
        assert (again == lvl).all()                                                  # deterministic
    assert moved_somewhere > 0
