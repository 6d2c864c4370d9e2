"""The magnitude model of the lazy wave NTT as tested code (no GPU).

tools/ntt_model_r4.py runs inside the suite and is the scalar reference of tests/ntt_bounds_common.py's vectorised emulation;
the library's three statements of the interval recurrence (pack.hpp pack_forward_bound, br_forms.hpp forward_bound,
ntt_wave.hpp make_inv_plan, through tfhe_hip_test_ntt_bounds) are held to the model's; the searched worst inputs of
tests/golden/ntt_bounds_inputs.npz regenerate, overflow nowhere, stay under the recurrence step by step and reach at least what
random inputs reach; the digit-table first step, which only the blind rotation uses, is searched here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ntt_bounds_common as B

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ntt_bounds_inputs as G   # noqa: E402

M = B.scalar_model()
P0, P1 = B.PRIMES
CONFIGS = [(logn, prime) for logn in (10, 11) for prime in (0, 1)]


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def fixture_arrays():
    return G.load()


def library_bounds(L, logn, x0):
    fwd, plan, out = (C.c_double * 2)(), (C.c_int32 * 25)(), C.c_double()
    assert L.tfhe_hip_test_ntt_bounds(logn, float(x0), fwd, plan, C.byref(out)) == 0
    return fwd[0], fwd[1], list(plan), out.value


# ---- 1. the model is tested code ----
def test_the_scalar_models_own_checks(capsys):
    M.main()
    assert capsys.readouterr().out.rstrip().endswith("ok")


@pytest.mark.parametrize("logn,prime", CONFIGS)
def test_vectorised_emulation_equals_the_scalar_model(logn, prime):
    """same tables, same steps, and on random and the model's own extreme inputs the same elements after the transform and
    the same largest magnitude after every step"""
    f = B.Field.get(prime, logn)
    P, N = f.P, f.N
    W, IW = M.tables(P, N)
    assert (W, IW) == (f.W, f.IW)
    assert M.fwd_steps(logn) == f.fwd_steps and M.inv_steps(logn) == f.inv_steps
    rng = np.random.default_rng(logn * 2 + prime)
    for x in (rng.integers(-2048, 2048, N), np.full(N, 2048), np.full(N, -2048), rng.integers(-(P - 1), P, N),
              np.where(rng.integers(0, 2, N) > 0, P - 1, -(P - 1))):
        want_track, got_track = [], []
        want = M.forward(x, W, P, logn, want_track)
        got = f.forward(x[None], got_track, kernel_form=False)[0]
        assert [int(v) for v in got] == want
        assert [int(t[0]) / P for t in got_track] == want_track
        # the kernel's form of S' (adds x3 (P - w1 w3)): the same residues, under the same bound
        kernel_track = []
        kern = f.forward(x[None], kernel_track)[0]
        assert not ((kern - got) % P).any()
        bound = M.fwd_bound(logn, np.abs(x).max() / P, P)
        assert all(t[0] / P <= b + 1e-9 for t, b in zip(kernel_track, bound))
    renorm, bounds = M.inv_schedule(logn, 4.0, P)
    for y in (rng.integers(-4 * P + 1, 4 * P, N), np.full(N, 4 * P - 1), np.full(N, -(4 * P - 1)),
              np.where(rng.integers(0, 2, N) > 0, 4 * P - 1, -(4 * P - 1))):
        want_track, got_track = [], []
        want = M.inverse(y, IW, P, logn, renorm, want_track)
        got = f.inverse(y[None], renorm, got_track)[0]
        assert [int(v) for v in got] == want
        assert [int(t[0]) / P for t in got_track] == want_track
        assert all(t <= b + 1e-9 for t, b in zip(want_track, bounds))
    # the step-by-step restatements this file's other tests use
    assert np.allclose(B.fwd_bounds(B.Field.get(1, logn), 0.3), M.fwd_bound(logn, 0.3, P1), rtol=1e-14)
    r1, b1 = M.inv_schedule(logn, 4.0, P1)
    assert np.allclose(B.inv_bounds(B.Field.get(1, logn), 4.0, r1), b1, rtol=1e-14)
    # an image word is what the exact transform gives, and words_of_image inverts it
    q = rng.integers(-2048, 2049, N)
    ref = M.ref_fwd([int(v) % P for v in q], W, P)
    assert [int(v) for v in f.image(q[None])[0]] == [v * f.scale % P for v in ref]
    img = rng.integers(0, P, N)
    assert (f.image(f.words_of_image(img[None]))[0] == img).all()


def test_the_emulations_checks_fire():
    f = B.Field.get(1, 10)
    with pytest.raises(B.BoundsViolation):
        f.forward(np.full((1, 1024), B.I32_MIN))                 # an unreduced word: 16 P in, past int32 after a step
    with pytest.raises(B.BoundsViolation):
        f.inverse(np.full((1, 1024), 5 * P1), B.RENORM[10])      # past the 4 P the plan is made for
    with pytest.raises(B.BoundsViolation):
        B.sum64("sum", *[np.array([2 ** 62])] * 2)
    with pytest.raises(B.BoundsViolation):
        f.inverse(np.full((1, 1024), 4 * P1 - 1), [False] * 5)   # no renormalisation at all


@pytest.mark.parametrize("logn", [9, 10, 11])
def test_the_librarys_recurrences_are_the_models(L, logn):
    for x0 in (15, 2 ** 6, 2 ** 11, P1 - 1, 2 ** 31):
        pack, forms, plan, out = library_bounds(L, logn, x0)
        model = M.fwd_bound(logn, x0 / P1, P1)[-1]
        assert abs(pack - model) <= 1e-12 * model and abs(forms - model) <= 1e-12 * model and abs(pack - forms) <= 1e-12 * model
    renorm, bounds = M.inv_schedule(logn, 4.0, P1)
    steps = M.inv_steps(logn)
    assert plan[0] == len(steps)
    assert plan[1:1 + plan[0]] == [2 * len(s) for s in steps] and not any(plan[1 + plan[0]:13])
    assert [bool(r) for r in plan[13:13 + plan[0]]] == renorm and not any(plan[13 + plan[0]:])
    assert abs(out - bounds[-1]) <= 1e-12 * bounds[-1] and out < 1.0
    py = B.Plan.python(logn, 4.0)
    lib = B.Plan.library(L, logn)
    assert (py.nsteps, py.fan, py.renorm) == (lib.nsteps, lib.fan, lib.renorm) and abs(py.out_bound - lib.out_bound) <= 1e-12
    if logn in B.RENORM:
        assert list(B.RENORM[logn]) == lib.renorm
    bad = (C.c_double * 2)(), (C.c_int32 * 25)(), C.c_double()
    assert L.tfhe_hip_test_ntt_bounds(8, 1.0, bad[0], bad[1], C.byref(bad[2])) == -1
    assert L.tfhe_hip_test_ntt_bounds(logn, -1.0, bad[0], bad[1], C.byref(bad[2])) == -1


def test_the_published_constants_follow_from_the_model():
    """ntt_wave.hpp: digits below 2^11 end below 6.1 P / 6.7 P, inputs below P below 7.6 P / 8.2 P; ring_public.hpp: an
    unreduced word would pass 16 P = 2^31; renormalisation at steps 1, 3, 5 of 5 at N = 1024"""
    d10, d11 = M.fwd_bound(10, 2048 / P1, P1)[-1], M.fwd_bound(11, 2048 / P1, P1)[-1]
    assert 6.0 < d10 < 6.1 and 6.6 < d11 < 6.7
    w10, w11 = M.fwd_bound(10, 1.0, P1)[-1], M.fwd_bound(11, 1.0, P1)[-1]
    assert 7.5 < w10 < 7.6 and 8.1 < w11 < 8.2 and w11 * P1 < 2 ** 31
    assert M.fwd_bound(10, 2 ** 31 / P1, P1)[-1] * P1 > 2 ** 31 and 2 ** 31 / P1 > 16.0
    assert M.inv_schedule(10, 4.0, P1)[0] == [True, False, True, False, True]
    # the product bound of ring_public.hpp and the MAC limits of pack.hpp / cmux.hpp
    assert w11 * B.Q + 0.5 < 0.76
    for logn, rows in ((10, 18), (11, 16)):
        for x0 in (15, 2048):
            f = M.fwd_bound(logn, x0 / P1, P1)[-1]
            assert rows * f * B.Q < 3.5 <= (rows + 1) * f * B.Q


# ---- 2. the searched inputs: no overflow, under the recurrence step by step, past what random inputs reach ----
def step_bounds(pipeline, field):
    """{direction: the recurrence's bound after every step, in units of the larger prime}"""
    wide = B.Field.get(1, field.logn)
    if pipeline == "public":
        fwd = B.fwd_bounds(wide, 1.0)
        return {"fwd": fwd, "inv": B.inv_bounds(wide, fwd[-1] * B.Q + 0.5, B.RENORM[field.logn]),
                "img": B.fwd_bounds(wide, B.max_coef(field.N) / P1)}
    rows, lo, hi = G.digit_shape(pipeline, field.logn)
    fwd = B.fwd_bounds(wide, max(-lo, hi) / P1)
    into = rows * fwd[-1] * B.Q + 0.5
    assert into < 4.0                                             # what make_inv_plan is made for
    return {"fwd": fwd, "inv": B.inv_bounds(wide, into, B.RENORM[field.logn])}


def entry_inputs(arrays, base, pipeline, classes):
    """the inputs of one fixture entry, the arrays it does not store at zero"""
    x = {name: np.zeros((1,) + cls[0], dtype=np.int64) for name, cls in classes.items()}
    for name, stored in G.stored(pipeline, base.split("/")[3]).items():
        x[name] = arrays[base + "/" + stored].astype(np.int64)[None]
        assert x[name].shape == (1,) + classes[name][0]
    return x


def admitted(cls, a):
    shape, ext, lo, hi = cls
    return np.isin(a, ext).all() if lo is None else lo <= a.min() and a.max() <= hi


def test_the_digit_pipelines_are_what_the_predicates_admit(L):
    """the rows and digits of the gadget and pack pipelines are the most the library accepts: the MAC limit where a
    constructor reaches it, else the last decomposition before a refusal"""
    ok = L.tfhe_hip_test_form_admissible
    for logn, N in ((10, 1024), (11, 2048)):
        l, bg = G.GADGET[logn]
        assert L.tfhe_hip_test_select_bounds(N, l, bg) == 0 and l * bg <= 32
        assert any(ok(f, N, l, bg, t) == 1 for f in range(4) for t in range(3))
        assert not any(ok(f, N, l + 1, bg, t) == 1 for f in range(4) for t in range(3))       # no parameter set carries l + 1
        assert G.digit_shape("gadget", logn) == (2 * l, -2 ** (bg - 1), 2 ** (bg - 1) - 1)
        for name in G.PACK:
            t, bb = G.PACK[name][logn]
            assert L.tfhe_hip_test_pack_bounds(N, t, bb) == 0 and t * bb <= 32
            assert L.tfhe_hip_test_pack_bounds(N, t + 1, bb) != 0 or (t + 1) * bb > 32
            assert G.digit_shape(name, logn) == (t, 0, 2 ** bb - 1)
    assert G.GADGET[10][0] * 2 == 18 == G.PACK["pack1"][10][0] and G.PACK["pack1"][11][0] == 16      # the MAC limit itself
    assert L.tfhe_hip_test_select_bounds(1024, 10, 3) == 1 and L.tfhe_hip_test_select_bounds(2048, 8, 4) == 0


@pytest.mark.parametrize("logn,prime", CONFIGS)
@pytest.mark.parametrize("pipeline", G.PIPELINES)
def test_searched_inputs_hold_the_bounds_and_reach_past_random_ones(fixture_arrays, pipeline, logn, prime, capsys):
    field = B.Field.get(prime, logn)
    classes, evaluate = G.problem(pipeline, field)
    targets = G.targets_of(pipeline, field)
    bounds = step_bounds(pipeline, field)
    for cls in classes.values():                                  # the admitted sets lie inside what the predicates allow
        assert B.I32_MIN <= min(cls[1]) and max(cls[1]) <= B.I32_MAX and (cls[2] is None or cls[2] <= min(cls[1]) and max(cls[1]) <= cls[3])
    T = B.max_coef(field.N)
    assert field.N * T * 2 ** 31 < B.CRT_EXACT_LIMIT <= field.N * 2 * T * 2 ** 31
    if pipeline in ("public", "negacyclic"):
        assert classes.get("q", classes.get("digits"))[3] == T
    random_val = evaluate(G.random_inputs(pipeline, field, classes))    # 64 uniform inputs; a violation raises
    assert len(random_val) == 64
    all_bounds = [b for d in ("fwd", "inv", "img") if d in bounds for b in bounds[d]]
    assert (random_val <= np.array(all_bounds) * P1).all()
    line, gain = [], {}
    for i, (direction, k) in enumerate(targets):
        base = "%s/%d/p%d/%s/%d" % (pipeline, field.N, prime, direction, k)
        x = entry_inputs(fixture_arrays, base, pipeline, classes)
        for name, cls in classes.items():
            assert admitted(cls, x[name]), (base, name)
        val = evaluate(x)[0]                                      # every check of the emulation ran: a violation raises
        assert all(v <= b * P1 for v, b in zip(val, all_bounds)), (base, val / P1, all_bounds)
        bound = bounds[direction][k] * P1
        reach, random_reach = val[i] / bound, random_val[:, i].max() / bound
        assert reach >= random_reach, (base, reach, random_reach)
        gain[direction] = gain.get(direction, 0.0) + reach - random_reach
        line.append("%s%d %.2f (random %.2f)" % (direction, k, reach, random_reach))
    # strictly past the random inputs the search started from, in every direction: a search that does nothing fails
    assert all(g > 0 for g in gain.values()), gain
    with capsys.disabled():
        print("\nreach %s N = %d prime %d: %s" % (pipeline, field.N, prime, ", ".join(line)))


def test_the_fixture_holds_one_entry_per_target(fixture_arrays):
    want = ["%s/%d/p%d/%s/%d" % (pl, 1 << logn, prime, d, k) for pl in G.PIPELINES for logn, prime in CONFIGS
            for d, k in G.targets_of(pl, B.Field.get(prime, logn))]
    assert G.entries_of(fixture_arrays) == sorted(want)
    assert all(a.dtype == np.int32 for a in fixture_arrays.values())
    files = {G.file_of(name) for name in fixture_arrays}
    assert all(os.path.getsize(f) < 1 << 20 for f in files), {os.path.basename(f): os.path.getsize(f) for f in files}


# ---- 3. the fixture regenerates (a subset at N = 1024), and the greedy moves were accepted, not only the restarts ----
@pytest.mark.parametrize("pipeline,prime", [("public", 0), ("public", 1), ("negacyclic", 0), ("negacyclic", 1), ("gadget", 1),
                                            ("pack1", 0), ("pack4", 1)])
def test_n1024_entries_regenerate_byte_for_byte(fixture_arrays, pipeline, prime):
    report = {}
    out, _ = G.find(pipeline, 10, prime, report)
    assert out
    for name, a in out.items():
        assert a.dtype == fixture_arrays[name].dtype and a.shape == fixture_arrays[name].shape and a.tobytes() == fixture_arrays[name].tobytes(), name
    targets = G.targets_of(pipeline, B.Field.get(prime, 10))
    for direction in {d for d, _ in targets}:
        assert sum(int(report["moves"][i]) for i, (d, _) in enumerate(targets) if d == direction) > 0, (direction, report["moves"])


# ---- the digit-table first step (ntt_wave.hpp forward_digits<TABLE>; br_forms.hpp: |e| <= 1/2 + |d| q) ----
@pytest.mark.parametrize("logn,prime", CONFIGS)
def test_digit_table_first_step(logn, prime):
    field = B.Field.get(prime, logn)
    width = 7
    rows, step = B.table_first_step(field, width)
    d = np.arange(1 << width)
    d = np.where(d < 64, d, d - 128)
    assert (np.abs(rows) <= 0.5 * P1 + np.abs(d) * B.Q).all()                         # every entry, exhaustively
    first = 64 / P1 + 3 * (0.5 + 64 * B.Q / P1)                                       # x0 + A + S: a digit and three entries
    assert first <= 1.5 + (2 ** 6 + 6) / P1                       # ntt_wave.hpp's "1.5 P + 2^6", and three times 64 P / 2^32 <= 2
    rng = np.random.default_rng([3, logn, prime])
    x = np.concatenate([rng.integers(-64, 64, (48, field.N)), rng.choice([-64, 0, 63], (48, field.N))])
    y = step(x)
    assert np.abs(y).max() <= first * P1
    # the same residues as the multiplying first step, and the rest of the transform under the bound from `first`
    full_track, track = [], []
    full = field.forward(x, full_track)
    rest = field.forward(y, track, first=1)
    assert not ((full - rest) % field.P).any()
    bounds = B.fwd_bounds(B.Field.get(1, logn), first, first=1)
    assert all(t.max() <= b * P1 for t, b in zip(track, bounds[1:]))
    assert bounds[-1] < (6.8 if logn == 10 else 7.4)
    # the searched pipeline: first step from the table, the rest of the transform; per step its worst found digits
    classes = {"digits": ((field.N,), np.array([-64, 0, 63]), -64, 63)}

    def evaluate(inp):
        t = []
        y = step(inp["digits"])
        field.forward(y, t, first=1)
        return np.stack([np.abs(y).max(axis=-1)] + t, axis=1).astype(np.float64)

    start = B.uniform_inputs(classes, rng, 64)
    random_val = evaluate(start)
    report = {}
    best, val = B.search(evaluate, classes, len(bounds), rng, start, 64, 60, 8, report)
    again = np.stack([evaluate({"digits": best["digits"][i:i + 1]})[0] for i in range(len(bounds))])
    assert (again <= np.array(bounds) * P1).all() and (np.diag(again) == val).all()
    assert (val >= random_val.max(axis=0)).all() and val.sum() > random_val.max(axis=0).sum() and report["moves"].sum() > 0
