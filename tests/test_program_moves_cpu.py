"""The programs with moves of tests/test_gpu_recorded_programs.py, without a GPU: that the splice leaves the base program
alone, that the four old programs are what they were, that every hazard the moves are there for does occur in every
program the GPU modes run (a census from the call lists alone), and that the sequential replay tells a right model of
the moves from three wrong ones (on the CPU oracle, at the GPU file's n = 16 set with host-only keys).

The census reads a call list by the rules of program_common.pending_walk: an operation recorded since the last flush,
flush_async or observation is pending.  The classes:
  (i)   a move writes a handle that a pending operation reads      (the operation must still read the old sample)
  (ii)  a move writes a handle that a pending operation writes     (the operation must not write the new sample)
  (iii) a move comes directly behind a flush_async                 (the flush in flight, the staging area)
  (iv)  a pack or export covers a handle with a pending result     (the observation runs it first)
  (v)   a moved sample is read by an operation before any flush    (the fresh slot as an operand)
  (vi)  an array holding moved samples is re-allocated             (fresh slots given back)
  (vii) a device-async import, an operation recorded on it, then an observation: nothing waits for the host in between"""
import hashlib

import numpy as np
import pytest

import program_common as PC
import test_gpu_recorded_programs as P

# sha-256 of repr(random_program(seed, calls, keys)) of the four programs this file's parent commit ran
OLD_PROGRAMS = {
    (2026, 180, 1): "d2e9e276e694a85204b44249dd7a2d8027dbc4c781d1c810f1ee83a565627cd7",
    (77, 60, 1): "fae8f95027d22a7095c254be412e86ec65634065c2c794db111b9e29f540300e",
    (303, 180, 3): "f2d2b47e9e086ba891db8545113a92bc655a29965d25b02feade75d7baf587cf",
    (55, 170, 1): "68c045bc9983eb4e21f5eeabe1884449e70d6bec5e83e7c1937d1957d50a60df",
}
MODES = sorted(P.MOVES_PROGRAMS)
WRONG = {"an import that does not rename": PC.wrong_import_without_rename,
         "a pack that does not run what is pending": PC.wrong_pack_before_pending,
         "an unpack lost to a pending result": PC.wrong_unpack_lost_to_pending_result}


def test_the_four_old_programs_are_what_they_were():
    for (seed, ncalls, nkeys), digest in OLD_PROGRAMS.items():
        calls = P.random_program(seed, ncalls, nkeys)
        assert hashlib.sha256(repr(calls).encode()).hexdigest() == digest, (seed, ncalls, nkeys)


@pytest.mark.parametrize("mode", MODES)
def test_the_splice_leaves_the_base_program_in_its_order_and_unchanged(mode):
    base_seed, ncalls, nkeys, seed, nmoves = P.MOVES_PROGRAMS[mode]
    base = P.random_program(base_seed, ncalls, nkeys)
    calls = P.moves_program(mode)
    assert PC.base_of(calls) == base
    assert calls == P.moves_program(mode)                              # a generator of its own: the same list every time
    moves = [c for c in calls if c[0] in PC.MOVE_FORMS]
    assert nmoves <= len(moves) <= nmoves + 1
    for c in moves:                                                     # what the GPU harness relies on
        t = c[3] if c[0] in ("unpack", "unpack_seeded", "import_seeded") else c[2]
        assert 1 <= len(t) <= P.PER and c[1] in PC.MOVE_FORMS[c[0]]
        if c[1] != "scattered":
            assert t == [(t[0][0], t[0][1] + j) for j in range(len(t))] and t[-1][1] < P.PER
        if c[0] in ("unpack", "unpack_seeded") and c[2] is not None:
            top = (2 if c[0] == "unpack" else 1) * 1024
            assert len(c[2]) == len(t) and all(0 <= x < top for x in c[2]) and 0 <= c[4] < nkeys
        if c[0] == "import_seeded":
            assert len(c[2]) == len(t) and all(0 <= x < PC.RECORD for x in c[2])


@pytest.mark.parametrize("mode", MODES)
def test_every_hazard_class_and_every_form_occurs(mode, capsys):
    calls = P.moves_program(mode)
    classes, forms = PC.census(calls)
    with capsys.disabled():
        print(f"\n[program moves] ({mode}) {len(calls)} calls, " + ", ".join(f"({k}) {v}" for k, v in classes.items()))
    assert all(classes[k] >= 3 for k in PC.CLASSES), classes
    assert forms == PC.all_forms(), PC.all_forms() - forms
    # the ring samples' edges, repeated indices, a handle given twice, words that the program exported brought back
    listed = {k: [c[2] for c in calls if c[0] == k and c[2] is not None] for k in ("unpack", "unpack_seeded", "import_seeded")}
    assert {0, 1023, 1024, 2047} <= {x for idx in listed["unpack"] for x in idx}
    assert {0, 1023} <= {x for idx in listed["unpack_seeded"] for x in idx}
    assert any(len(set(idx)) < len(idx) for idx in listed["unpack"] + listed["unpack_seeded"])
    assert any(len(set(idx)) < len(idx) for idx in listed["import_seeded"])
    assert any(c[1] == "scattered" and len(set(c[3])) < len(c[3]) for c in calls if c[0] in listed)
    assert any(c[0] == "import" and c[3][0] == "observed" for c in calls)


def test_the_census_on_programs_written_by_hand():
    A, B, X, Y = (0, 0), (0, 1), (1, 0), (1, 1)
    gate = ("gate", "AND", X, A, B, 0)
    none = dict.fromkeys(PC.CLASSES, 0)
    imp = lambda h, form="host": ("import", form, [h], ("random", 1))
    assert PC.census([gate, imp(A)])[0] == dict(none, i=1)
    assert PC.census([gate, ("flush",), imp(A)])[0] == none
    assert PC.census([gate, ("const", A, 1, 0), imp(A)])[0] == none               # the handle was renamed before the move
    assert PC.census([gate, imp(X)])[0] == dict(none, ii=1)
    assert PC.census([("gate", "AND", A, A, B, 0), imp(A)])[0] == dict(none, ii=1)  # r = AND(r, x): r names the result
    assert PC.census([gate, ("flush_async",), imp(Y)])[0] == dict(none, iii=1)
    assert PC.census([gate, ("pack", "host", [X, Y])])[0] == dict(none, iv=1)
    assert PC.census([gate, ("copy", Y, X, 0), ("export", "device", [Y])])[0] == dict(none, iv=1)
    assert PC.census([imp(A), gate])[0] == dict(none, v=1)
    assert PC.census([imp(A), ("observe", B, "sync"), gate])[0] == none
    assert PC.census([imp(A), ("flush",), ("realloc", 0)])[0] == dict(none, vi=1)
    assert PC.census([imp(A), ("realloc", 1)])[0] == none
    chain = [imp(A, "device_async"), gate, ("export", "device_async", [Y])]
    assert PC.census(chain)[0] == dict(none, v=1, vii=1)
    assert PC.census([chain[0], gate, ("flush",), chain[2]])[0] == dict(none, v=1)
    assert PC.census([chain[0], ("const", A, 0, 0), gate, chain[2]])[0] == none
    assert PC.census(chain)[1] == {("import", "device_async"), ("export", "device_async")}


# ---- the replay tells the right model from three wrong ones -----------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(oracle):
    made = {}

    def get(nkeys):
        if nkeys not in made:
            made[nkeys] = P.Fixture(oracle, nkeys=nkeys, device=False)
        return made[nkeys]

    yield get
    for fx in made.values():
        fx.close()


def differs(a, b):
    return (any((a["final"][h] != b["final"][h]).any() for h in a["final"])
            or any(x.shape != y.shape or (x != y).any() for x, y in zip(a["observed"], b["observed"])))


@pytest.mark.parametrize("mode", MODES)
def test_each_wrong_model_of_the_moves_differs_from_the_replay(fixtures, mode, capsys):
    fx = fixtures(P.MOVES_PROGRAMS[mode][2])
    calls = P.moves_program(mode)
    true = P.replay(fx, calls)
    again = P.replay(fx, calls)
    assert not differs(true, again) and len(true["observed"]) == sum(c[0] in PC.FLUSH_POINTS[2:] for c in calls)
    assert true["keyswitches"] >= sum(len(c[3]) for c in calls if c[0].startswith("unpack")) > 0
    for what, rewrite in WRONG.items():
        rewritten = rewrite(calls)
        assert rewritten != calls, what
        wrong = P.replay(fx, rewritten)
        assert len(wrong["observed"]) == len(true["observed"])
        assert differs(true, wrong), (mode, what)
    with capsys.disabled():
        print(f"\n[program moves] ({mode}) replay: {P.moves_text(true['moves'])}rotations {true['rotations']}, "
              f"key switches {true['keyswitches']}; each of {len(WRONG)} wrong models differs")


def test_the_references_of_the_moves(fixtures):
    """the record's samples, expanded by the restatement the replay uses, are encryptions of bits under key 0 (phase
    +-1/8 within 2^-8: 128 sigma of ks_stdev), and the folded replay of a program with moves still folds"""
    import seeded_lwe_common as SL
    fx = fixtures(1)
    lwe = SL.phases(fx.record_plain, fx.ks[0].lwe_key()[:fx.pp.n])
    assert (np.abs(np.abs(lwe.astype(np.int64)) - (1 << 29)) < (1 << 24)).all()
    calls = P.moves_program("a")
    folded = P.replay(fx, calls, fold=True)
    assert folded["rotations"] < P.replay(fx, calls)["rotations"]
