"""The launch rules (peba1_amd/csrc/launch_plan.hpp), no GPU: which blind-rotate launches a level of a flush turns into
and how its key switches are cut, through tfhe_hip_test_br_plan / tfhe_hip_test_ks_plan.  The rows the GPU tests pin with
the engine's counters on a card of 256 CUs (test_gpu_multikey.WIDE_ROWS, test_gpu_gate3.FORM_ROWS) are restated here as
plans, the rule's properties hold over a grid of gadgets, tunings, CU counts and widths, and the key-switch rule is checked
against cases worked by hand."""
import ctypes as C
import functools

import pytest

import adversarial_common as A
import test_gpu_gate3
import test_gpu_multikey

WIDE4, SPLIT, WAVE8, WAVE2 = A.WIDE4, A.SPLIT, A.WAVE8, A.WAVE2
# name -> (N, l, Bgbit): the built-in sets, the custom gadgets of test_gpu_multikey's sixteen-key test, the adversarial file's
GADGETS = {"l2_Bg10": (1024, 2, 10), "l3_Bg6": (1024, 3, 6)}
GADGETS.update({name: s[:3] for name, s in A.SETS.items()})
# the shapes the key-switch rule reads: (n, N, k, ks_t, ks_basebit)
KS_SETS = {"P128": (630, 1024, 1, 8, 2), "P80": (500, 1024, 1, 8, 2), "P2048": (1024, 2048, 1, 8, 2)}
BR_DEFAULTS = {"br_variant": -1, "br8_max_rotations": 1 << 30, "br_tail8": 1, "br_digit_table": 1}
KS_DEFAULTS = {"ks_target_blocks": 32768, "ks_max_splits": 48, "ks_split_ties": 0, "ks_tile": 16, "ks_index": 1}
STAMPS, ACC_DUMP = 1, 2


@functools.lru_cache(maxsize=None)
def lib():
    from peba1_amd import lib as L
    return L.load()


@functools.lru_cache(maxsize=None)
def admissible(form, N, l, Bgbit, tables):
    return lib().tfhe_hip_test_form_admissible(form, N, l, Bgbit, tables) == 1


def br_plan(gadget, tunings, cu_count, count, flags=0):
    """(form, tables, tail) of a level of `count` rotations; tunings: names of BR_DEFAULTS, the rest at their defaults"""
    N, l, Bgbit = gadget
    t = dict(BR_DEFAULTS, **tunings)
    t4 = (C.c_int32 * 4)(t["br_variant"], t["br8_max_rotations"], t["br_tail8"], t["br_digit_table"])
    out = (C.c_int32 * 3)()
    assert lib().tfhe_hip_test_br_plan(N, l, Bgbit, t4, cu_count, count, flags, out) == 0
    return tuple(out)


def ks_plan(shape, tunings, cu_count, count):
    """(tiled, tile, chunk, splits of the first chunk, splits of the last chunk, partial bytes)"""
    t = dict(KS_DEFAULTS, **tunings)
    t5 = (C.c_int32 * 5)(*(t[k] for k in KS_DEFAULTS))
    out = (C.c_int64 * 6)()
    assert lib().tfhe_hip_test_ks_plan(*shape, t5, cu_count, count, out) == 0
    return tuple(out)


def ks_plan7(shape, tunings, cu_count, count):
    """the same six words and the kernel form (tfhe_hip_test_ks_plan_form)"""
    t = dict(KS_DEFAULTS, **tunings)
    t5 = (C.c_int32 * 5)(*(t[k] for k in KS_DEFAULTS))
    out = (C.c_int64 * 7)()
    assert lib().tfhe_hip_test_ks_plan_form(*shape, t5, cu_count, count, out) == 0
    assert tuple(out)[:6] == ks_plan(shape, tunings, cu_count, count)
    return tuple(out)


def counters(plans_and_keys):
    """(br_launches, br8_launches, br8_rotations) a flush adds whose levels have these (count, plan, keys with a share):
    the meaning of the three statistics in include/tfhe_hip.h, as Engine::execute() derives them from a level's plan"""
    br = br8 = rot8 = 0
    for count, (form, tables, tail), keys in plans_and_keys:
        if form in (WIDE4, WAVE8) or keys == 1:
            br += 2 if tail else 1
        else:
            br += keys                                       # no multi-key kernel: one launch per key with a share
        if form == WAVE8:
            br8, rot8 = br8 + 1, rot8 + count
        elif tail:
            br8, rot8 = br8 + 1, rot8 + tail
    return br, br8, rot8


# ---- the GPU tests' rows, as plans at 256 CUs ---------------------------------------------------------------------------
def test_named_plans_of_the_gpu_rows():
    """The levels test_gpu_multikey builds (558 / 7 / 1 rotations) and test_gpu_gate3's (528 / 48), plan by plan."""
    P128, P80, P2048 = GADGETS["P128"], GADGETS["P80"], GADGETS["P2048"]
    for g in (P128, P80):
        assert br_plan(g, {}, 256, 558) == (WIDE4, 1, 46)            # one round of 512 on the 4-wave form + a tail of 46
        assert br_plan(g, {}, 256, 528) == (WIDE4, 1, 16)
        assert br_plan(g, {}, 256, 48) == br_plan(g, {}, 256, 7) == br_plan(g, {}, 256, 1) == (WAVE8, 1, 0)
        assert br_plan(g, {"br_tail8": 0}, 256, 558) == br_plan(g, {"br_tail8": 0}, 256, 528) == (WIDE4, 1, 0)
        assert br_plan(g, {"br_tail8": 0}, 256, 7) == (WAVE8, 1, 0)
        assert br_plan(g, {"br_digit_table": 0}, 256, 558) == (WIDE4, 0, 46)
        assert br_plan(g, {"br_digit_table": 0}, 256, 7) == (WAVE8, 0, 0)
        for count in (558, 528, 48, 7, 1):
            assert br_plan(g, {"br8_max_rotations": 0}, 256, count) == (WIDE4, 1, 0)
            assert br_plan(g, {"br_variant": 2}, 256, count) == (SPLIT, 1, 0)
            assert br_plan(g, {"br_variant": 4}, 256, count) == (WAVE2, 1, 0)
    for count in (558, 528, 48, 7, 1):
        for table in (1, 0, 2):
            assert br_plan(P2048, {"br_digit_table": table}, 256, count) == (SPLIT, table, 0)
        assert br_plan(P2048, {"br_variant": 4}, 256, count) == (SPLIT, 1, 0)    # the 2-wave form is N = 1024 only


@pytest.mark.parametrize("pname,tunings,br8,br,rot8", test_gpu_multikey.WIDE_ROWS)
def test_wide_rows_of_the_multikey_gpu_test(pname, tunings, br8, br, rot8):
    """Three keys; level 1: 231 / 186 / 141 rotations (558), level 2: 5 / 0 / 2 (7), level 3: 1 / 0 / 0."""
    levels = [(558, 3), (7, 2), (1, 1)]
    got = counters([(count, br_plan(GADGETS[pname], tunings, 256, count), keys) for count, keys in levels])
    assert got == (br, br8, rot8)


@pytest.mark.parametrize("pname,tunings,replicas,br,br8,rot8", test_gpu_gate3.FORM_ROWS)
def test_form_rows_of_the_gate3_gpu_test(pname, tunings, replicas, br, br8, rot8):
    count = 48 * replicas
    assert counters([(count, br_plan(GADGETS[pname], tunings, 256, count), 1)]) == (br, br8, rot8)


# ---- properties over a grid ------------------------------------------------------------------------------------------
GRID_TUNINGS = [{}, {"br_tail8": 0}, {"br8_max_rotations": 0}, {"br8_max_rotations": 1}, {"br8_max_rotations": 100},
                {"br_variant": 0}, {"br_variant": 2}, {"br_variant": 4}, {"br_digit_table": 0}, {"br_digit_table": 2},
                {"br_digit_table": 3}, {"br_variant": 2, "br_digit_table": 2}, {"br_variant": 4, "br_digit_table": 0},
                {"br_variant": 0, "br8_max_rotations": 100, "br_tail8": 0}]


@pytest.mark.parametrize("name", sorted(GADGETS))
def test_plan_properties_over_the_grid(name):
    """For every gadget x tunings x CU count in {64, 256, 304} x width 1 .. 4 CUs + 3 x probe flags:
    the planned (form, tables) is admissible for the gadget; the 8-wave form (one workgroup per CU in its LDS, rows split
    over two waves, no stamps, N = 1024) is never planned for more than `cu_count` rotations, for l < 2, with stamps or at
    N = 2048; the tail is the rule of launch_plan.hpp exactly: tail = r = count mod 2 CUs if the form is 4-wave, br_tail8
    is on, count > 2 CUs, 0 < r <= min(br8_max_rotations, CUs), l >= 2, no probe is on and the 8-wave form is admissible
    with the plan's tables, else 0; reading the accumulators back never changes the form, only the tail."""
    gadget = GADGETS[name]
    N, l, Bgbit = gadget
    fn = lib().tfhe_hip_test_br_plan
    out = (C.c_int32 * 3)()
    seen_forms, seen_tails = set(), 0
    for tunings in GRID_TUNINGS:
        t = dict(BR_DEFAULTS, **tunings)
        t4 = (C.c_int32 * 4)(t["br_variant"], t["br8_max_rotations"], t["br_tail8"], t["br_digit_table"])
        for cu in (64, 256, 304):
            for count in range(1, 4 * cu + 4):
                plans = []
                for flags in range(4):
                    assert fn(N, l, Bgbit, t4, cu, count, flags, out) == 0
                    form, tables, tail = out
                    plans.append((form, tables, tail))
                    where = (name, tunings, cu, count, flags, plans[-1])
                    assert 0 <= form < 4 and 0 <= tables <= 2 and admissible(form, N, l, Bgbit, tables), where
                    if form == WAVE8:
                        assert count <= cu and l >= 2 and not flags & STAMPS and N == 1024, where
                    r = count % (2 * cu)
                    split = (form == WIDE4 and t["br_tail8"] != 0 and count > 2 * cu and 0 < r <= min(t["br8_max_rotations"], cu)
                             and l >= 2 and flags == 0 and admissible(WAVE8, N, l, Bgbit, tables))
                    assert tail == (r if split else 0), where
                assert plans[2][:2] == plans[0][:2] and plans[3][:2] == plans[1][:2], (name, tunings, cu, count, plans)
                seen_forms.add(plans[0][0])
                seen_tails += plans[0][2] > 0
    # the grid reaches what it is about: every form that admits the gadget, and tails wherever the 4- and 8-wave forms do
    assert seen_forms == {f for f in range(4) if any(admissible(f, N, l, Bgbit, tb) for tb in range(3))}, seen_forms
    assert (seen_tails > 0) == (admissible(WIDE4, N, l, Bgbit, 0) and admissible(WAVE8, N, l, Bgbit, 0)), seen_tails


def test_eight_wave_form_is_admissible_only_where_the_four_wave_form_is():
    """Engine::execute() plans a multi-key level once, from its total width, and launches forms without a multi-key kernel
    once per key IN THAT FORM.  A per-key decision from each key's smaller share could differ from the level's only by
    choosing the 8-wave form where the level, wider than the CU count, could not; that needs a gadget the 8-wave form admits
    and the 4-wave form does not.  There is none, in any table mode."""
    wave8 = 0
    for N in (1024, 2048):
        for l in range(1, 33):
            for Bgbit in range(1, 13):
                for tables in range(3):
                    if admissible(WAVE8, N, l, Bgbit, tables):
                        wave8 += 1
                        assert admissible(WIDE4, N, l, Bgbit, tables), (N, l, Bgbit, tables)
    assert wave8 > 0


# ---- the key-switch rule -----------------------------------------------------------------------------------------------
def test_ks_ranges_fill_whole_rounds_of_workgroup_slots():
    """Worked from the rule (launch_plan.hpp ks_splits).  P128: ct_stride = 632 words, one thread per 4 words = 158 -> 192
    threads = 3 waves a workgroup.  Index form, tile 24: 12 waves a CU fit (162 VGPRs), so 12 / 3 = 4 workgroups a CU, and
    256 CUs hold 1024 of them.  864 gates = 36 tiles.  The ranges may number 16 (= 1024 coefficients / 64) to 48
    (ks_max_splits); 36 x s workgroups fill ceil(36 s / 1024) rounds of 1024 slots.  One round holds s <= 28 and is fullest
    at 28: 1008 of 1024 = 0.984.  Two rounds hold s <= 56, capped at 48: 1728 of 2048 = 0.844.  So 28 ranges under either
    tie rule -- not 32 (1152 of 2048 = 0.5625) -- and the partial sums take 864 x 28 x 632 words.
    Default tile 16: 16 / 3 = 5 workgroups a CU, 1280 slots.  A full chunk of 8192 gates = 512 tiles; 512 s / 1280 = 0.4 s
    rounds, whole when 5 divides s: every such s fills its rounds completely, and the tie rule picks the smallest (20:
    least partial-sum traffic) or the largest (45) of 20 .. 45."""
    p128 = KS_SETS["P128"]
    for ties in (0, 1):
        assert ks_plan(p128, {"ks_tile": 24, "ks_split_ties": ties}, 256, 864) == (1, 24, 8192, 28, 28, 864 * 28 * 632 * 4)
    assert ks_plan(p128, {}, 256, 8192)[:5] == (1, 16, 8192, 20, 20)
    assert ks_plan(p128, {"ks_split_ties": 1}, 256, 8192)[:5] == (1, 16, 8192, 45, 45)
    # another card: 304 CUs x 5 = 1520 slots; 512 s / 1520 is whole when 95 divides s, which no s <= 48 does; the best
    # s in 16 .. 48 by exhaustion of the rule's own formula
    eff = {s: 512 * s / (-(-512 * s // 1520) * 1520) for s in range(16, 49)}
    best = max(eff.values())
    assert ks_plan(p128, {}, 304, 8192)[3] == min(s for s in eff if eff[s] > best - 1e-9)


def test_ks_tile_clamp_chunks_and_narrow_launches():
    p128 = KS_SETS["P128"]
    # tiles of 24 and 32 exist in the index form only: the strip form runs tiles of 16
    for tile in (24, 32):
        assert ks_plan(p128, {"ks_tile": tile, "ks_index": 1}, 256, 4096)[:2] == (1, tile)
        assert ks_plan(p128, {"ks_tile": tile, "ks_index": 0}, 256, 4096)[:2] == (1, 16)
    # tiled from 2 tiles on; below that, with tile 0, with other key-switch digits or with ranges longer than 64
    # coefficients (1024 / 8 = 128): the per-gate kernel in one launch
    assert ks_plan(p128, {}, 256, 32)[:3] == (1, 16, 8192) and ks_plan(p128, {}, 256, 31)[:3] == (0, 0, 31)
    assert ks_plan(p128, {"ks_tile": 0}, 256, 20000)[:3] == (0, 0, 20000)
    assert ks_plan((630, 1024, 1, 4, 4), {}, 256, 20000)[:3] == (0, 0, 20000)
    assert ks_plan(p128, {"ks_max_splits": 8}, 256, 20000)[:3] == (0, 0, 20000)
    # a tiled launch runs in chunks of 8192 gates: 20000 = 8192 + 8192 + 3616
    tiled, tile, chunk, first, last, nbytes = ks_plan(p128, {}, 256, 20000)
    assert (tiled, tile, chunk) == (1, 16, 8192)
    assert first == ks_plan(p128, {}, 256, 8192)[3] and last == ks_plan(p128, {}, 256, 3616)[3]
    assert nbytes == max(8192 * first, 3616 * last) * 632 * 4
    # narrow launches: ranges double while twice the workgroups stay within ks_target_blocks, past ks_max_splits once
    assert ks_plan(p128, {}, 256, 1)[3:] == (64, 64, 64 * 632 * 4)
    assert ks_plan(p128, {"ks_target_blocks": 64}, 256, 8)[3:] == (8, 8, 8 * 8 * 632 * 4)
    # one range: no partial sums
    for count in (1, 31, 32, 8192, 20000):
        assert ks_plan(p128, {"ks_max_splits": 1}, 256, count)[3:] == (1, 1, 0)
    assert ks_plan(p128, {"ks_target_blocks": 1}, 256, 31)[3:] == (1, 1, 0)


def test_ks_form_of_the_built_in_sets():
    """The kernel form Engine::launch_ks runs and counts (ks_pergate / ks_strip / ks_index_launches) is the plan's seventh
    word: 0 = per gate, 1 = LDS strips, 2 = index.  The built-in sets all have a tiled row width (128, 192, 320 threads)."""
    PERGATE, STRIP, INDEX = 0, 1, 2
    for shape in KS_SETS.values():
        assert ks_plan7(shape, {}, 256, 32)[6] == INDEX and ks_plan7(shape, {}, 256, 31)[6] == PERGATE
        assert ks_plan7(shape, {"ks_index": 0}, 256, 4096)[6] == STRIP
        assert ks_plan7(shape, {"ks_index": 0, "ks_tile": 32}, 256, 4096)[:2] + ks_plan7(shape, {"ks_index": 0, "ks_tile": 32}, 256, 4096)[6:] == (1, 16, STRIP)
        for tile in (24, 32):
            assert ks_plan7(shape, {"ks_tile": tile}, 256, 2 * tile)[6] == INDEX
            assert ks_plan7(shape, {"ks_tile": tile}, 256, 2 * tile - 1)[6] == PERGATE
        for tunings in ({"ks_tile": 0}, {"ks_max_splits": 8}, {"ks_max_splits": 1}):
            assert ks_plan7(shape, tunings, 256, 20000)[6] == PERGATE
        for tunings in ({}, {"ks_index": 0}, {"ks_tile": 24}, {"ks_tile": 0}):
            for count in (1, 31, 32, 64, 8192, 20000):
                p = ks_plan7(shape, tunings, 256, count)
                assert p[0] == (p[6] != PERGATE) and (p[1] > 0) == (p[6] != PERGATE)


@pytest.mark.parametrize("pname", sorted(KS_SETS))
def test_ks_partial_bytes_cover_every_chunk(pname):
    """The partial-sum buffer execute() sizes before anything is enqueued holds count x ranges x ct_stride words of every
    chunk launch_ks then launches (all chunks but the last are full and alike), and no range is longer than 64
    coefficients in a tiled launch."""
    shape = KS_SETS[pname]
    n, N, k = shape[:3]
    stride = (n + 1 + 3) & ~3
    counts = sorted(set(range(1, 200)) | set(range(200, 20000, 389)) |
                    {m * t + d for t in (16, 24, 32) for m in (1, 2, 3, 100, 511, 512, 513) for d in (-1, 0, 1)} |
                    {m * 8192 + d for m in (1, 2, 3) for d in (-1, 0, 1)})
    for tunings in ({}, {"ks_tile": 24}, {"ks_tile": 32}, {"ks_index": 0}, {"ks_tile": 0}, {"ks_max_splits": 32},
                    {"ks_max_splits": 64}, {"ks_split_ties": 1}, {"ks_max_splits": 1}):
        for cu in (64, 256, 304):
            for count in counts:
                tiled, tile, chunk, first, last, nbytes = ks_plan(shape, tunings, cu, count)
                where = (pname, tunings, cu, count)
                nchunks = -(-count // chunk)
                last_cnt = count - (nchunks - 1) * chunk
                assert chunk == (8192 if tiled else count) and 1 <= last_cnt <= chunk, where
                need = [cnt * s * stride * 4 for cnt, s in ((min(chunk, count), first), (last_cnt, last)) if s > 1]
                assert nbytes >= max(need, default=0), where
                assert nbytes == max(need, default=0), where
                if tiled:
                    assert tile in (16, 24, 32) and count >= 2 * tile, where
                    assert max(2, -(-k * N // 64)) <= first <= dict(KS_DEFAULTS, **tunings)["ks_max_splits"], where


# ---- one planner: the words before and after, and what unpack sizes from ---------------------------------------------------
def ks_plan_form2(shape, t7, has_image, cu_count, count):
    out = (C.c_int64 * 7)()
    assert lib().tfhe_hip_test_ks_plan_form2(*shape, (C.c_int32 * 7)(*t7), has_image, cu_count, count, out) == 0
    return list(out)


def test_ks_launch_plan_returns_the_recorded_words_of_the_commit_before():
    """tests/golden/ks_plan_parent.json: the seven words of tfhe_hip_test_ks_plan_form2 over the grid the file states (5 shapes
    x 10 tunings x has_image 0 / 1 x 3 CU counts x 19 widths: 1, the two-tile thresholds 32 / 48 / 64, the matrix thresholds
    64 / 512 and the chunk boundaries 8192 / 16384 with their neighbours, 20000), recorded from the library of the commit
    before plan_ks_launch replaced plan_ks / ks_tiled / ks_splits / ks_partial_bytes and their callers' chunk loops.  Word
    for word.  (The file holds each distinct row of seven words once and, per grid point, its index.)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "ks_plan_parent.json")) as f:
        doc = json.load(f)
    g = doc["grid"]
    assert len(g["shapes"]) == 5 and len(g["tunings"]) == 10 and len(g["widths"]) == 19
    lines = iter(doc["rows"])
    checked = 0
    for sname, shape in g["shapes"].items():
        for tn in g["tunings"]:
            t7 = [tn.get(name, default) for name, default in zip(g["tuning_names"], g["tuning_defaults"])]
            for img in g["has_image"]:
                for cu in g["cu_counts"]:
                    line = next(lines)
                    assert len(line) == len(g["widths"])
                    for width, index in zip(g["widths"], line):
                        want, got = doc["distinct"][index], ks_plan_form2(shape, t7, img, cu, width)
                        assert got == want, ("first differing row", sname, tn, "has_image", img, "CUs", cu, "width", width,
                                             "recorded", want, "now", got)
                        checked += 1
    assert next(lines, None) is None and checked == 5700


@pytest.mark.parametrize("pname", sorted(KS_SETS))
def test_unpack_partial_sums_hold_the_full_chunk_and_the_last_one(pname):
    """Engine::run_unpack runs the key switches of UNPACK_CHUNK + 33 samples by two plans, one of a full chunk (8,192 gates)
    and one of 33 (which may be cut into more ranges), and sizes the partial sums once from the larger of the two: each
    plan's bytes hold gates x ranges x ct_stride words of its own width."""
    UNPACK_CHUNK = 8192                                          # unpack.hpp
    shape = KS_SETS[pname]
    stride = (shape[0] + 1 + 3) & ~3
    for tunings in ({}, {"ks_tile": 0}, {"ks_index": 0}, {"ks_max_splits": 32}):
        for gates in (UNPACK_CHUNK, 33):
            tiled, tile, chunk, first, last, nbytes = ks_plan(shape, tunings, 256, gates)
            assert chunk >= gates and first == last > 1, (pname, tunings, gates)      # one part each
            assert nbytes >= gates * first * stride * 4, (pname, tunings, gates, nbytes)
