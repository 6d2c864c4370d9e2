"""CPU tests of the multi-output LUT bootstrap (tfhe_hip_lut_bootstrap_multi): the numpy restatement of the extract at
index e against the oracle's own extract, the builders and accessors, the error channel, the construction from tables
against the decrypt rule, the level plan of recordings that hold multi-output ops (through the host-logic entry
tfhe_hip_test_level_plan_multi, which runs the recorder's own sharing and elimination code), and the committed digests."""
import ctypes as C

import numpy as np
import pytest

import lut_common as T
import lut_multi_common as M

I32 = np.int32
P32 = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from peba1_amd import api
    return api


def _params(api, pname):
    return {"P128": lambda: api.ParameterSet(128), "P80": lambda: api.ParameterSet(80),
            "P2048": lambda: api.ParameterSet(p2048=True)}[pname]()


def p(a):
    return a.ctypes.data_as(P32)


# ---- the restatement against the oracle's extract -----------------------------------------------------------------------
def rotate_back(poly, e):
    """X^-e * poly in Z[X]/(X^N + 1): coefficient j is poly[j + e] below N, -poly[j + e - N] from N on."""
    N = len(poly)
    j = np.arange(N) + e
    return T.wrap32(np.where(j < N, poly[j % N].astype(np.int64), -poly[j % N].astype(np.int64)))


@pytest.mark.parametrize("pname", ["P128", "P2048"])
def test_extract_at_is_the_oracles_extract_of_the_rotated_accumulator(oracle, pname):
    oks = oracle.KeySet(oracle.params(pname), 3)
    N = oks.N
    rng = np.random.default_rng(17)
    for trial in range(3):
        acc = rng.integers(-2 ** 31, 2 ** 31, 2 * N, dtype=np.int64).astype(I32)
        assert (M.extract_at(acc, 0) == oks.sample_extract(acc)).all()
        for e in [1, N // 2, N - 1] + rng.integers(2, N - 1, 3).tolist():
            rotated = np.concatenate([rotate_back(acc[:N], e), rotate_back(acc[N:], e)])
            assert (M.extract_at(acc, e) == oks.sample_extract(rotated)).all(), e
    # a combination is the sum of its taps' extracts, wrapping, plus the constant on the body
    acc = rng.integers(-2 ** 31, 2 ** 31, 2 * N, dtype=np.int64).astype(I32)
    u = M.output(acc, [(5, -8), (N - 1, 8)], -12345)
    want = -8 * M.extract_at(acc, 5).astype(np.int64) + 8 * M.extract_at(acc, N - 1).astype(np.int64)
    want[N] -= 12345
    assert (u == T.wrap32(want)).all()
    oks.close()


# ---- builders and accessors ------------------------------------------------------------------------------------------------
def test_builder_copies_everything_and_the_accessors_show_it(api):
    pp = _params(api, "P128")
    N = pp.N
    v = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(I32)
    lut = api.Lut(pp, v)
    spec = [([(0, 1), (N - 1, -8)], 77), ([(N // 2, 8)], -(1 << 31)), ([(3, 2)], 0), ([(9, -1), (8, 1), (7, 3)], 5)]
    mo = api.LutMulti(lut, spec)
    lut.close()                                        # the object holds its own copy of the words
    assert mo.nout == 4 and mo.outputs() == spec
    assert (mo.words() == v).all()
    mo.close()
    one = api.LutMulti(api.Lut.constant(pp, 5), M.IDENTITY)
    assert one.nout == 1 and one.outputs() == M.IDENTITY and (one.words() == 5).all()
    one.close()


@pytest.mark.parametrize("slots", [2, 4, 8])
def test_from_tables_gives_the_defined_taps_and_decrypts_to_its_levels(api, slots):
    """For every sector s and every phase p in it, the noiseless decrypt rule applied to the object's own taps, constant
    and polynomial gives step * levels[m][s] -- checked against the definitions, not against the construction."""
    pp = _params(api, "P128")
    N = pp.N
    rng = np.random.default_rng(slots)
    for step, nout in ((1 << 29, 2), (-(1 << 27) + 2, 4), (1 << 26, 1)):
        while True:
            levels = rng.integers(-3, 4, (nout, slots))
            if all(len(set(row.tolist())) > 1 for row in levels):
                break
        mo = api.LutMulti.from_tables(pp, step, levels)
        words, want_spec = M.spec_from_tables(N, step, levels)
        assert mo.outputs() == want_spec and (mo.words() == words).all()
        v = mo.words()
        for m, (taps, c0) in enumerate(mo.outputs()):
            for q in range(N):
                s = q * slots // N
                assert M.noiseless_phase(v, q, taps, c0) == int(T.wrap32(step * int(levels[m][s]))), (slots, m, q)
        mo.close()


def test_two_bit_decomposition_and_full_adder_tables(api):
    pp = _params(api, "P128")
    N = pp.N
    bits = api.LutMulti.from_tables(pp, 1 << 29, [[-1, 1, -1, 1], [-1, -1, 1, 1]])
    assert bits.outputs() == [([(N // 4, -2), (N // 2, 2), (3 * N // 4, -2)], 0), ([(N // 2, -2)], 0)]
    adder = api.LutMulti.from_tables(pp, 1 << 29, [[0, 1, 0, 1], [0, 0, 1, 1]])
    assert adder.outputs() == [([(N // 4, -1), (N // 2, 1), (3 * N // 4, -1)], 1 << 28), ([(N // 2, -1)], 1 << 28)]
    for x in (bits, adder):
        x.close()


def test_builder_errors_go_to_the_error_channel(api, L):
    pp = _params(api, "P128")
    N = pp.N
    lut = api.Lut.constant(pp, 1)
    bad = {"nout must be 1..4": [([(0, 1)], 0)] * 5,
           "1..8 taps": [([(i, 1) for i in range(9)], 0)],
           "outside 0..N-1": [([(N, 1)], 0)],
           "zero or beyond": [([(3, 9)], 0)],
           "same index": [([(3, 1), (4, 1), (3, -1)], 0)]}
    for match, spec in bad.items():
        L.tfhe_hip_clear_error()
        with pytest.raises(ValueError, match=match):
            api.LutMulti(lut, spec)
        assert match in api.last_error()
    for spec in ([], [([], 0)], [([(-1, 1)], 0)], [([(3, 0)], 0)], [([(3, -9)], 0)]):
        L.tfhe_hip_clear_error()
        with pytest.raises(ValueError):
            api.LutMulti(lut, spec)
        assert api.last_error() != ""
    one = np.ones(1, I32)
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_lut_multi(None, 1, p(one), p(one), p(one), None) and "null or deleted LUT" in api.last_error()
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_lut_multi(lut.ptr, 1, None, p(one), p(one), None) and "null tap list" in api.last_error()
    # from tables: odd step, slots that do not divide N, a constant table, a jump beyond 8, more than 8 taps
    for match, (step, levels) in {"step must be even": (3, [[0, 1]]), "divide N": (2, [[0, 1, 2]]),
                                  "needs no tap": (2, [[0, 1], [4, 4]]), "more than 8": (2, [[0, 9]]),
                                  "more than 8 taps": (2, [[i % 2 for i in range(16)]])}.items():
        L.tfhe_hip_clear_error()
        with pytest.raises(ValueError, match=match):
            api.LutMulti.from_tables(pp, step, levels)
        assert match in api.last_error()
    L.tfhe_hip_clear_error()
    assert L.tfhe_hip_lut_multi_nout(None) == -1 and "null or deleted" in api.last_error()
    mo = api.LutMulti(lut, M.IDENTITY)
    L.tfhe_hip_clear_error()
    assert L.tfhe_hip_lut_multi_output(mo.ptr, 1, None, None, None) == -1 and "no such output" in api.last_error()
    cnt = C.c_int32(7)
    assert not L.tfhe_hip_lut_multi_words(None, C.byref(cnt)) and cnt.value == 0
    mo.close()
    lut.close()


def test_bootstrap_argument_errors_leave_the_call_without_effect(api, L):
    """Refused before the key is touched: with a host-only keyset nothing reaches a GPU, and the results are as they were."""
    pp = _params(api, "P128")
    ks = api.SecretKeySet(pp, 11, device=False)
    r = api.CiphertextArray(pp, 2)
    r2 = api.CiphertextArray(pp, 1)
    a = api.CiphertextArray(pp, 3)
    mo = api.LutMulti(api.Lut.constant(pp, 1 << 28), [([(1, 1)], 0), ([(2, 1)], 0)])
    big = api.LutMulti(api.Lut.constant(_params(api, "P2048"), 1 << 28), [([(1, 1)], 0), ([(2, 1)], 0)])
    LS = type(a.ptr)
    before = [(r.at(i).contents.slot, r.at(i).contents.b) for i in range(2)]
    one = np.array([1, 1, 1, 1], dtype=I32)
    ins = (LS * 4)(a.at(0), a.at(1), a.at(2), a.at(0))
    both, same, none = (LS * 4)(r.at(0), r.at(1)), (LS * 4)(r.at(0), r.at(0)), (LS * 4)()
    rows = ((big, both, 1, "holds 2048 words, the key's ring has 1024"), (None, both, 1, "null or deleted multi-output LUT"),
            (mo, both, 0, "nin must be 1, 2 or 3"), (mo, both, 4, "nin must be 1, 2 or 3"),
            (mo, same, 1, "two results are the same sample"), (mo, none, 1, "every result is null"))
    for who, res, n, match in rows:
        L.tfhe_hip_clear_error()
        L.tfhe_hip_lut_bootstrap_multi(who.ptr if who else None, res, n, ins, p(one), 0, ks.cloud)
        assert match in api.last_error(), (match, api.last_error())
        assert [(r.at(i).contents.slot, r.at(i).contents.b) for i in range(2)] == before
        L.tfhe_hip_clear_error()
        arrays = (LS * 4)(r.ptr, r2.ptr) if res is both else (LS * 4)(r.ptr, r.ptr) if res is same else (LS * 4)()
        rc = L.tfhe_hip_lut_bootstrap_multi_batch(who.ptr if who else None, arrays, n, (LS * 4)(a.ptr, a.ptr, a.ptr, a.ptr),
                                                  p(one), 0, 1, ks.cloud)
        assert rc == -1 and match in api.last_error()
    L.tfhe_hip_clear_error()
    L.tfhe_hip_lut_bootstrap_multi(mo.ptr, both, 1, ins, p(one), 0, None)
    assert "null cloud key" in api.last_error()
    L.tfhe_hip_clear_error()
    L.tfhe_hip_lut_bootstrap_multi(mo.ptr, None, 1, ins, p(one), 0, ks.cloud)
    assert "null result list" in api.last_error()
    for x in (mo, big):
        x.close()
    ks.close()


def test_stats_gain_their_fields_at_the_end():
    from peba1_amd import lib
    names = [f for f, _ in lib.Stats._fields_]
    assert names[-3:] == ["lut_rotations", "multi_rotations", "multi_outputs"]


# ---- the level plan ---------------------------------------------------------------------------------------------------
def plan_multi(L, ops16, keys=None, nkeys=1, unit=256, balance=0, reuse=1, dead=()):
    ops = np.ascontiguousarray(ops16, dtype=I32).reshape(-1, 16)
    count = len(ops)
    keys = np.zeros(count, dtype=I32) if keys is None else np.ascontiguousarray(keys, dtype=I32)
    ndead = len(dead)
    dead = np.ascontiguousarray(list(dead) + [0], dtype=I32)
    levels, shared, sizes = np.zeros(count, I32), np.zeros(count, I32), np.zeros(6, I32)
    rot_off, ks_off = np.zeros(count + 1, I32), np.zeros(count + 1, I32)
    rot_koff, ks_koff = np.zeros(count * nkeys + 1, I32), np.zeros(count * nkeys + 1, I32)
    rot_key, rots, kss = np.zeros(2 * count, I32), np.zeros((2 * count, 10), I32), np.zeros((4 * count, 4), I32)
    depth = L.tfhe_hip_test_level_plan_multi(p(ops), p(keys), count, nkeys, unit, balance, reuse, p(dead),
                                             ndead, p(levels), p(shared), p(sizes),
                                             p(rot_off), p(ks_off), p(rot_koff), p(ks_koff), p(rot_key), p(rots), p(kss))
    assert depth >= 0
    nl, nr, nk = sizes[0], sizes[1], sizes[2]
    return dict(depth=depth, levels=levels, shared=shared, rots=rots[:nr], kss=kss[:nk], rot_off=rot_off[:nl + 1],
                ks_off=ks_off[:nl + 1], rot_koff=rot_koff[:sizes[3]], ks_koff=ks_koff[:sizes[4]], rot_key=rot_key[:sizes[5]])


def multi_op(dsts, slots, lut, coefs, c0, spec, nout=None):
    nout = len(dsts) if nout is None else nout
    s = list(slots) + [-1] * (3 - len(slots))
    c = list(coefs) + [0] * (3 - len(coefs))
    return [M.OP_LUTM, -1] + s + [lut] + c + [c0, spec, nout] + list(dsts) + [-1] * (4 - len(dsts))


def lut_op(dst, slots, lut, coefs, c0):
    s = list(slots) + [-1] * (3 - len(slots))
    c = list(coefs) + [0] * (3 - len(coefs))
    return [T.OP_LUT, dst] + s + [lut] + c + [c0, -1, 0, -1, -1, -1, -1]


def gate(kind, dst, a, b=-1, c=-1):
    return [kind, dst, a, b, c] + [0] * 5 + [-1, 0, -1, -1, -1, -1]


def word(spec, *wanted):
    return spec | sum(1 << m for m in wanted) << 24


def test_one_rotation_and_a_key_switch_per_wanted_output_with_consecutive_samples(L):
    ops = [gate(2, 20, 1, 2),                                        # an AND: sample 0
           multi_op([10, 11, 12, 13], [1, 2, 3], 5, [1, -2, 2], -777, 7),   # four outputs: samples 1..4
           lut_op(21, [4], 6, [-1], 123456),                         # sample 5
           multi_op([14, -1, 15], [4], 2, [3], 9, 8),                # three outputs, the second not wanted: samples 6..8
           gate(16, 22, 1, 2, 3)]                                    # a MUX: samples 9, 10
    pl = plan_multi(L, ops)
    assert pl["depth"] == 1 and len(pl["rots"]) == 6 and len(pl["kss"]) == 9
    assert pl["rots"][0].tolist() == [1, 2, 1, 1, -(1 << 29), 0, -1, 0, -1, -1]
    assert pl["rots"][1].tolist() == [1, 2, 1, -2, -777, 1, 3, 2, 5, word(7, 0, 1, 2, 3)]
    assert pl["rots"][2].tolist() == [4, 4, -1, 0, 123456, 5, -1, 0, 6, -1]
    assert pl["rots"][3].tolist() == [4, 4, 3, 0, 9, 6, -1, 0, 2, word(8, 0, 2)]
    assert pl["rots"][4][5] == 9 and pl["rots"][5][5] == 10
    assert pl["kss"].tolist() == [[0, -1, 0, 20], [1, -1, 0, 10], [2, -1, 0, 11], [3, -1, 0, 12], [4, -1, 0, 13],
                                  [5, -1, 0, 21], [6, -1, 0, 14], [8, -1, 0, 15], [9, 10, 1 << 29, 22]]
    assert pl["rot_off"].tolist() == [0, 6] and pl["ks_off"].tolist() == [0, 9]
    # every output becomes available at the op's level: readers of two different outputs sit one level later
    pl = plan_multi(L, [multi_op([10, 11], [1], 0, [1], 0, 0), gate(2, 12, 10, 11), multi_op([13, 14], [11], 0, [1], 0, 0)])
    assert pl["depth"] == 2 and pl["levels"].tolist() == [1, 2, 2] and pl["rot_off"].tolist() == [0, 1, 3]
    assert pl["rots"][2][5] == 1                      # samples are counted per level


def test_dead_outputs_lose_their_key_switch_and_an_all_dead_op_its_rotation(L):
    ops = [multi_op([10, 11, 12], [1], 0, [1], 0, 3), gate(2, 13, 11, 2), multi_op([14, 15], [2], 0, [1], 0, 4)]
    # 12 is held by nobody and read by nobody; 11 is held by nobody but the AND reads it
    pl = plan_multi(L, ops, dead=[11, 12])
    assert len(pl["rots"]) == 3 and pl["rots"][0][9] == word(3, 0, 1)
    assert pl["kss"].tolist() == [[0, -1, 0, 10], [1, -1, 0, 11], [3, -1, 0, 14], [4, -1, 0, 15], [0, -1, 0, 13]]
    assert pl["rots"][1][5] == 3                      # the dead output keeps its place: output m stays at u_index + m
    # the AND dead as well: 11 dies with it
    pl = plan_multi(L, ops, dead=[11, 12, 13])
    assert pl["levels"].tolist() == [1, -1, 1] and pl["rots"][0][9] == word(3, 0) and len(pl["kss"]) == 3
    # all outputs of the second op dead: its rotation goes; all of the first too: it goes with its reader
    pl = plan_multi(L, ops, dead=[14, 15])
    assert pl["levels"].tolist() == [1, 2, -1] and len(pl["rots"]) == 2 and len(pl["kss"]) == 4
    pl = plan_multi(L, ops, dead=[10, 11, 12, 13])
    assert pl["levels"].tolist() == [-1, -1, 1] and len(pl["rots"]) == 1 and pl["kss"].tolist() == [[0, -1, 0, 14], [1, -1, 0, 15]]


def test_sharing_is_output_by_output_and_widens_the_earlier_op(L):
    base = multi_op([10, -1, 12], [1, 2], 3, [1, -1], 42, 6)
    later = multi_op([20, 21, -1], [1, 2], 3, [1, -1], 42, 6)        # wants output 1, which the earlier op dropped
    pl = plan_multi(L, [base, later, gate(2, 30, 20, 21)])
    assert pl["shared"].tolist() == [-1, 0, -1] and len(pl["rots"]) == 2
    assert pl["rots"][0][9] == word(6, 0, 1, 2)       # widened: all three outputs are written by the one rotation
    assert pl["kss"][:3].tolist() == [[0, -1, 0, 10], [1, -1, 0, 21], [2, -1, 0, 12]]
    assert pl["rots"][1][:2].tolist() == [10, 21]     # the reader reads the shared output 0 and the added output 1
    assert pl["levels"].tolist() == [1, 1, 2]
    variants = {"spec": multi_op([20, 21, -1], [1, 2], 3, [1, -1], 42, 7), "lut": multi_op([20, 21, -1], [1, 2], 4, [1, -1], 42, 6),
                "c0": multi_op([20, 21, -1], [1, 2], 3, [1, -1], 43, 6), "coefficient": multi_op([20, 21, -1], [1, 2], 3, [1, 1], 42, 6),
                "operand": multi_op([20, 21, -1], [1, 5], 3, [1, -1], 42, 6)}
    for what, other in variants.items():
        pl = plan_multi(L, [base, other])
        assert pl["shared"].tolist() == [-1, -1] and len(pl["rots"]) == 2, what
    assert plan_multi(L, [base, later], keys=[0, 1], nkeys=2)["shared"].tolist() == [-1, -1]
    assert plan_multi(L, [base, later], reuse=0)["shared"].tolist() == [-1, -1]
    # a single-output LUT op of the same polynomial and operands is another kind: not shared
    assert plan_multi(L, [base, lut_op(20, [1, 2], 3, [1, -1], 42)])["shared"].tolist() == [-1, -1]
    # an output added by widening and then dead is dropped again
    pl = plan_multi(L, [base, later], dead=[21])
    assert pl["rots"][0][9] == word(6, 0, 2) and len(pl["kss"]) == 2


def test_a_dead_reader_releases_its_operands_exactly_once(L):
    """The AND's result (10) lost its handle and is read by a live multi-output op and by two dead gates: each dead reader
    gives back its own reference and no more, so the AND stays exactly as long as the multi-output op does."""
    ops = [gate(2, 10, 1, 2), multi_op([20, 21], [10, 3], 0, [1, 1], 0, 5), gate(4, 11, 10, 3), gate(0, 12, 10, 4)]
    pl = plan_multi(L, ops, dead=[10, 11, 12])
    assert pl["levels"].tolist() == [1, 2, -1, -1] and len(pl["rots"]) == 2
    assert pl["kss"].tolist() == [[0, -1, 0, 10], [0, -1, 0, 20], [1, -1, 0, 21]]
    pl = plan_multi(L, ops, dead=[10, 11])               # the second reader alive: it and the AND stay
    assert pl["levels"].tolist() == [1, 2, -1, 2] and len(pl["rots"]) == 3
    pl = plan_multi(L, ops, dead=[10, 11, 12, 20, 21])   # the last reader gone: the AND goes with it
    assert pl["levels"].tolist() == [-1, -1, -1, -1] and len(pl["rots"]) == 0 and len(pl["kss"]) == 0


def test_a_shared_op_lives_as_long_as_one_handle_of_its_result(L):
    """An XOR recorded three times is one op whose result three handles hold (11, and 12 and 13 re-pointed at it); it is
    dead when the last of them is, and then its producer, which only it read, is dead too."""
    ops = [gate(2, 10, 1, 2), gate(4, 11, 10, 3), gate(4, 12, 10, 3), gate(4, 13, 3, 10)]
    for dead in ([10, 11, 12], [10, 11, 13], [10, 12, 13], [10, 11]):
        pl = plan_multi(L, ops, dead=dead)
        assert pl["shared"].tolist() == [-1, -1, 1, 1] and pl["levels"].tolist() == [1, 2, 2, 2], dead
        assert pl["kss"].tolist() == [[0, -1, 0, 10], [0, -1, 0, 11]], dead
    pl = plan_multi(L, ops, dead=[10, 11, 12, 13])
    assert pl["levels"].tolist() == [-1, -1, -1, -1] and len(pl["rots"]) == 0
    pl = plan_multi(L, ops, dead=[11, 12, 13])           # the producer's own handle lives: it stays alone
    assert pl["levels"].tolist() == [1, -1, -1, -1] and pl["kss"].tolist() == [[0, -1, 0, 10]]


def test_a_dead_widened_output_costs_its_key_switch_not_the_rotation(L):
    base = multi_op([10, -1], [1], 0, [1], 0, 3)
    later = multi_op([-1, 21], [1], 0, [1], 0, 3)                    # widens the op by output 1 (slot 21)
    ops = [base, later, gate(2, 30, 10, 2)]
    pl = plan_multi(L, ops)
    assert pl["shared"].tolist() == [-1, 0, -1] and pl["rots"][0][9] == word(3, 0, 1) and len(pl["kss"]) == 3
    pl = plan_multi(L, ops, dead=[10, 21])                           # 10 is still read by the AND
    assert pl["levels"].tolist() == [1, 1, 2] and len(pl["rots"]) == 2
    assert pl["rots"][0][9] == word(3, 0) and pl["kss"].tolist() == [[0, -1, 0, 10], [0, -1, 0, 30]]


def test_grouping_by_key_with_several_keys(L):
    ops = [multi_op([10, 11], [1], 2, [1], 5, 0), gate(4, 12, 1, 2), multi_op([13, -1, 14, 15], [2, 3], 1, [2, 2], 0, 1),
           gate(16, 16, 1, 2, 3), lut_op(17, [3], 0, [-1], 9)]
    keys = [2, 0, 1, 1, 0]
    pl = plan_multi(L, ops, keys=keys, nkeys=3)
    assert pl["depth"] == 1
    assert pl["rot_koff"].tolist() == [0, 2, 5, 6] and pl["ks_koff"].tolist() == [0, 2, 6, 8]
    assert pl["rot_key"].tolist() == [0, 0, 1, 1, 1, 2]
    # samples: key 0 holds 0, 1; key 1 the four outputs 2..5 and the MUX's 6, 7; key 2 the two outputs 8, 9
    assert pl["rots"][:, 5].tolist() == [0, 1, 2, 6, 7, 8]
    assert pl["rots"][:, 9].tolist() == [-1, -1, word(1, 0, 2, 3), -1, -1, word(0, 0, 1)]
    assert pl["kss"].tolist() == [[0, -1, 0, 12], [1, -1, 0, 17], [2, -1, 0, 13], [4, -1, 0, 14], [5, -1, 0, 15],
                                  [6, 7, 1 << 29, 16], [8, -1, 0, 10], [9, -1, 0, 11]]


def test_the_lut_plan_entry_keeps_its_words(L):
    """tfhe_hip_test_level_plan_lut still gives nine words per rotation although the descriptor has ten."""
    ops = np.array([[T.OP_LUT, 10, 1, 2, 3, 5, 1, -2, 2, -777]], dtype=I32)
    z = lambda n: np.zeros(n, I32)
    levels, shared, sizes, rots = z(1), z(1), z(6), np.full(19, 99, I32)
    bufs = [z(2), z(2), z(2), z(2), z(2)]
    assert L.tfhe_hip_test_level_plan_lut(p(ops), p(z(1)), 1, 1, 256, 0, 1, p(levels), p(shared), p(sizes),
                                          *[p(b) for b in bufs], p(rots), p(z(4))) == 1
    assert rots[:9].tolist() == [1, 2, 1, -2, -777, 0, 3, 2, 5] and (rots[9:] == 99).all()


# ---- the committed digests ----------------------------------------------------------------------------------------------
def test_fixture_file_covers_what_it_must():
    d = M.load_digests()
    indices, nouts, weights, eight, c0s, null_middle, identity = set(), set(), set(), False, False, False, False
    for pname, count in M.CASES.items():
        cases = d["sets"][pname]["cases"]
        N = M.RING[pname]
        assert len(cases) == count and cases == [dict(c, **{k: x[k] for k in x if k.startswith(("sha256", "first"))})
                                                 for c, x in zip(M.case_specs(pname), cases)]
        for c in cases:
            spec = M.spec_of(c)
            M.check_limits(N, spec)
            nouts.add(len(spec))
            for taps, c0 in spec:
                indices |= {("0", "1", "N/2", "N-1")[(0, 1, N // 2, N - 1).index(e)] if e in (0, 1, N // 2, N - 1) else "other"
                            for e, _ in taps}
                weights |= {w for _, w in taps}
                eight |= len(taps) == 8
                c0s |= c0 != 0
            w = c["wanted"]
            null_middle |= any(not w[m] and any(w[:m]) and any(w[m + 1:]) for m in range(len(w)))
            identity |= spec == M.IDENTITY
            assert [s is None for s in c["sha256"]] == [not x for x in w] and len(c["sha256_extracted"]) == len(spec)
    assert indices == {"0", "1", "N/2", "N-1", "other"} and nouts >= {1, 2, 4}
    assert {8, -8} <= weights and min(weights) < 0 < max(weights)
    assert eight and c0s and null_middle and identity


@pytest.mark.parametrize("pname", list(M.CASES))
def test_two_cases_per_set_recomputed_from_the_oracle(oracle, pname):
    d = M.load_digests()
    oks = oracle.KeySet(oracle.params(pname), d["key_seed"])
    cases = d["sets"][pname]["cases"]
    for c in (cases[1], cases[2]):
        cts, us, acc = M.oracle_case(oracle, oks, c)
        assert T.sha256_words(acc) == c["sha256_accumulator"]
        assert [T.sha256_words(u) for u in us] == c["sha256_extracted"]
        for ct, sha, first in zip(cts, c["sha256"], c["first_words"]):
            assert (ct is None) == (sha is None)
            if ct is not None:
                assert T.sha256_words(ct) == sha and [int(x) for x in ct[:4]] == first
    oks.close()


def test_the_one_tap_spec_is_the_lut_bootstrap(oracle):
    """Spec (0, +1) with out_c0 = 0 restated gives the words of the single-output restatement."""
    c = M.load_digests()["sets"]["P128"]["cases"][0]
    assert M.spec_of(c) == M.IDENTITY
    oks = oracle.KeySet(oracle.params("P128"), M.KEY_SEED)
    ct, u, acc = T.oracle_lut_bootstrap(oracle, oks, M.case_lin(oracle, oks, c), T.lut_words(c["lut"], oks.N))
    assert T.sha256_words(ct) == c["sha256"][0] and T.sha256_words(u) == c["sha256_extracted"][0]
    oks.close()
