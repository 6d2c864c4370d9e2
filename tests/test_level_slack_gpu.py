"""The cost-driven levelling pass (tuning "level_slack") on the device: an 8-slot Function_f on 4-bit values under the
small parameter set of tests/test_gpu_recorded_programs.py (n = 16, N = 1024: P128's ring, gadget and key switch with a
16-step rotation), run once with level_slack 0 and once with 1 from the same input words.  The circuit
runs at bitsize 8 (13,584 recorded bootstraps): peba1_euclidean_distance, like the reference, accumulates in 24 samples
whatever the bitsize, so 3 x bitsize must be 24 -- at bitsize 4 it walks past its 12-sample distance array.  No tuning moves
the cost steps of a launch, so a synthetic table set through tfhe_hip_test_set_level_cost puts a step at every eighth
rotation -- inside every width the circuit has.  The result ciphertexts must be the same words in both runs and the CPU
oracle's (tests/golden/level_slack_function_f.npz, written by tests/golden/make_level_slack_fixture.py through the oracle's
own boots* provider and the same circuit library), and the pass must really have moved gates."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ks_common as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level_slack_function_f.npz")
# cost(w) = 20 + 10 ceil(w / 8): a step every eight rotations, flat in between
STEP_TABLE = [(8 * q + e, 20.0 + 10.0 * (q + 1)) for q in range(512) for e in (1, 8)]


def set_table(L, table):
    w = np.ascontiguousarray([t[0] for t in table], dtype=np.int32)
    c = np.ascontiguousarray([t[1] for t in table], dtype=np.float64)
    assert L.tfhe_hip_test_set_level_cost(w.ctypes.data_as(C.POINTER(C.c_int32)), c.ctypes.data_as(C.POINTER(C.c_double)), len(w)) == 0


def last_slack(L):
    out = np.zeros(4, dtype=np.float64)
    assert L.tfhe_hip_last_level_slack(out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return dict(before=out[0], after=out[1], moved=int(out[2]), pool_slots=int(out[3]))


def test_function_f_words_are_the_same_with_gates_moved_and_the_oracles():
    from peba1_amd import api, circuits, lib
    L = lib.load()
    g = np.load(GOLDEN)
    bits, nslots = int(g["bits"]), g["template"].shape[0]
    pp = api.ParameterSet(custom=K.custom_tuple(int(g["n"]), 8, 2))
    ks = api.SecretKeySet(pp, int(g["key_seed"]), device=True)
    runs = {}
    try:
        set_table(L, STEP_TABLE)
        for slack in (0, 1):
            api.set_tuning("level_slack", slack)
            T = [api.CiphertextArray(pp, bits).set_words(g["template"][s]) for s in range(nslots)]
            S = [api.CiphertextArray(pp, bits).set_words(g["probe"][s]) for s in range(nslots)]
            bound = api.CiphertextArray(pp, 3 * bits).set_words(g["bound"])
            rb = api.CiphertextArray(pp, 3 * bits)
            api.reset_stats()
            api.set_deferred(True)
            try:
                circuits.function_f(rb, SimpleNamespace(slots=S), SimpleNamespace(slots=T), bound, bits, ks)
                api.flush()
            finally:
                api.set_deferred(False)
            st, rep = api.stats(), last_slack(L)
            runs[slack] = (rb.words(), st, rep)
            print(f"level_slack {slack}: levels {st['levels']}, rotations {st['blind_rotates']}, launches {st['br_launches']} "
                  f"(8-wave {st['br8_launches']}), table cost {rep['before']:.0f} -> {rep['after']:.0f}, gates moved {rep['moved']}, "
                  f"pool slots at the flush {rep['pool_slots']}")
            del T, S, bound, rb
    finally:
        set_table(L, [])
        api.set_tuning("level_slack", 1)
        ks.close()
    (w0, st0, rep0), (w1, st1, rep1) = runs[0], runs[1]
    assert rep0["moved"] == 0 and rep0["before"] == rep0["after"] == 0          # off: the pass did not run
    assert rep1["moved"] > 0 and rep1["after"] < rep1["before"]                 # on: gates moved, and it paid by the table
    assert st0["levels"] == st1["levels"] and st0["blind_rotates"] == st1["blind_rotates"]
    assert rep0["pool_slots"] == rep1["pool_slots"]                             # moving gates sizes nothing anew
    # sharing and dead-gate elimination drop rotations, never add any (a shared or dropped gate is 1 or 2 rotations)
    assert st1["blind_rotates"] <= int(g["blind_rotates"]) <= st1["blind_rotates"] + 2 * (st1["reused_gates"] + st1["dead_gates"])
    assert w0.shape == g["result"].shape
    assert (w0 == w1).all()
    assert (w0 == g["result"]).all() and (w1 == g["result"]).all()
