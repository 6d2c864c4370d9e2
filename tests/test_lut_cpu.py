"""CPU tests of the programmable bootstrap (tfhe_hip_lut_bootstrap): the LUT builders' words, the error channel, the
level plan of recordings that hold LUT ops (through the host-logic entry tfhe_hip_test_level_plan_lut, which applies
the recorder's sharing rule), and the committed digests recomputed from the oracle's pieces."""
import ctypes as C

import numpy as np
import pytest

import lut_common as T

I32 = np.int32


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


# ---- builders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["P128", "P2048"])
def test_builder_words_equal_the_definitions(api, pname):
    pp = _params(api, pname)
    N = pp.N
    v = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(I32)
    lut = api.Lut(pp, v)
    assert (lut.words() == v).all()
    v[0] ^= 1                                          # the LUT holds a copy
    assert lut.words()[0] == v[0] ^ 1
    lut.close()
    for mu in (1 << 29, -12345, 0):
        lut = api.Lut.constant(pp, mu)
        assert (lut.words() == np.full(N, mu, dtype=I32)).all()
        lut.close()
    for slots in (1, 4, 8, N):
        values = np.random.default_rng(slots).integers(-2 ** 31, 2 ** 31, slots, dtype=np.int64).astype(I32)
        lut = api.Lut.from_table(pp, values)
        want = np.array([values[j * slots // N] for j in range(N)], dtype=I32)
        assert (lut.words() == want).all()
        lut.close()


def test_builder_errors_go_to_the_error_channel(api, L):
    pp = _params(api, "P128")
    L.tfhe_hip_clear_error()
    with pytest.raises(ValueError, match="slots must divide N"):
        api.Lut.from_table(pp, np.zeros(3, dtype=I32))
    assert "slots must divide N" in api.last_error()
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_lut_from_table(pp.ptr, np.zeros(4, dtype=I32).ctypes.data_as(C.POINTER(C.c_int32)), 0)
    assert "slots must divide N" in api.last_error()
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_lut(pp.ptr, None) and "null words" in api.last_error()
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_lut_constant(None, 5) and "null parameter set" in api.last_error()
    L.tfhe_hip_clear_error()
    cnt = C.c_int32(7)
    assert not L.tfhe_hip_lut_words(None, C.byref(cnt)) and cnt.value == 0 and "null or deleted LUT" in api.last_error()
    with pytest.raises(ValueError, match="holds 1024 words"):
        api.Lut(pp, np.zeros(2048, dtype=I32))


def test_bootstrap_argument_errors_leave_the_call_without_effect(api, L):
    """A LUT of another N, a null LUT and nin outside 1..3 are refused before the key is touched: with a host-only keyset
    (no device image) nothing reaches a GPU, and the result sample is as it was."""
    pp = _params(api, "P128")
    ks = api.SecretKeySet(pp, 11, device=False)
    p2048 = _params(api, "P2048")
    r = api.CiphertextArray(pp, 1)
    a = api.CiphertextArray(pp, 3)
    lut = api.Lut.constant(pp, 1 << 29)
    big = api.Lut.constant(p2048, 1 << 29)
    before = (r.ptr.contents.slot, r.ptr.contents.b)
    one = np.array([1, 1, 1, 1], dtype=I32)
    for who, n, match in ((big, 1, "holds 2048 words, the key's ring has 1024"), (None, 1, "null or deleted LUT"),
                          (lut, 0, "nin must be 1, 2 or 3"), (lut, 4, "nin must be 1, 2 or 3")):
        L.tfhe_hip_clear_error()
        ins = (type(a.ptr) * 4)(a.at(0), a.at(1), a.at(2), a.at(0))
        L.tfhe_hip_lut_bootstrap(who.ptr if who else None, r.at(0), n, ins, one.ctypes.data_as(C.POINTER(C.c_int32)), 0, ks.cloud)
        assert match in api.last_error(), (match, api.last_error())
        assert (r.ptr.contents.slot, r.ptr.contents.b) == before
        L.tfhe_hip_clear_error()
        rc = L.tfhe_hip_lut_bootstrap_batch(who.ptr if who else None, r.ptr, n, (type(a.ptr) * 4)(a.ptr, a.ptr, a.ptr, a.ptr),
                                            one.ctypes.data_as(C.POINTER(C.c_int32)), 0, 1, ks.cloud)
        assert rc == -1 and match in api.last_error()
    L.tfhe_hip_clear_error()
    L.tfhe_hip_lut_bootstrap(lut.ptr, r.at(0), 1, (type(a.ptr) * 1)(a.at(0)), one.ctypes.data_as(C.POINTER(C.c_int32)), 0, None)
    assert "null cloud key" in api.last_error()
    for x in (lut, big):
        x.close()
    ks.close()


# ---- the level plan ---------------------------------------------------------------------------------------------------
def plan_lut(L, ops10, keys=None, nkeys=1, unit=256, balance=0, reuse=1):
    ops = np.ascontiguousarray(ops10, dtype=I32).reshape(-1, 10)
    count = len(ops)
    keys = np.zeros(count, dtype=I32) if keys is None else np.ascontiguousarray(keys, dtype=I32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    levels, shared, sizes = np.zeros(count, I32), np.zeros(count, I32), np.zeros(6, I32)
    rot_off, ks_off = np.zeros(count + 1, I32), np.zeros(count + 1, I32)
    rot_koff, ks_koff = np.zeros(count * nkeys + 1, I32), np.zeros(count * nkeys + 1, I32)
    rot_key, rots, kss = np.zeros(2 * count, I32), np.zeros((2 * count, 9), I32), np.zeros((count, 4), I32)
    depth = L.tfhe_hip_test_level_plan_lut(p(ops), p(keys), count, nkeys, unit, balance, reuse, p(levels), p(shared), p(sizes),
                                           p(rot_off), p(ks_off), p(rot_koff), p(ks_koff), p(rot_key), p(rots), p(kss))
    assert depth >= 0
    nl, nr, nk = sizes[0], sizes[1], sizes[2]
    return dict(depth=depth, levels=levels, shared=shared, rots=rots[:nr], kss=kss[:nk], rot_off=rot_off[:nl + 1],
                ks_off=ks_off[:nl + 1], rot_koff=rot_koff[:sizes[3]], ks_koff=ks_koff[:sizes[4]], rot_key=rot_key[:sizes[5]])


def lut_op(dst, slots, lut, coefs, c0):
    s = list(slots) + [-1] * (3 - len(slots))
    c = list(coefs) + [0] * (3 - len(coefs))
    return [T.OP_LUT, dst] + s + [lut] + c + [c0]


def test_lut_op_is_one_rotation_and_one_key_switch_with_its_words(L):
    ops = [lut_op(10, [1, 2, 3], 5, [1, -2, 2], -777),
           lut_op(11, [4], 6, [-1], 123456),
           lut_op(12, [1, 2], 0, [2, -1], 0),
           [2, 13, 1, 2, -1, 0, 0, 0, 0, 0]]              # an AND beside them
    pl = plan_lut(L, ops)
    assert pl["depth"] == 1 and len(pl["rots"]) == 4 and len(pl["kss"]) == 4
    assert pl["rots"][0].tolist() == [1, 2, 1, -2, -777, 0, 3, 2, 5]
    # one operand: slot_b names A again with coefficient 0 (the kernels read its words whatever sb is)
    assert pl["rots"][1].tolist() == [4, 4, -1, 0, 123456, 1, -1, 0, 6]
    assert pl["rots"][2].tolist() == [1, 2, 2, -1, 0, 2, -1, 0, 0]
    assert pl["rots"][3].tolist() == [1, 2, 1, 1, -(1 << 29), 3, -1, 0, -1]      # gates keep the constant test vector
    assert pl["kss"].tolist() == [[0, -1, 0, 10], [1, -1, 0, 11], [2, -1, 0, 12], [3, -1, 0, 13]]
    # a LUT op that reads another's result sits one level later
    pl = plan_lut(L, [lut_op(10, [1], 0, [1], 0), lut_op(11, [10], 1, [1], 0)])
    assert pl["depth"] == 2 and pl["levels"].tolist() == [1, 2] and pl["rot_off"].tolist() == [0, 1, 2]


def test_sharing_needs_equal_lut_operands_coefficients_constant_and_key(L):
    base = lut_op(10, [1, 2], 3, [1, -1], 42)
    variants = {"lut": lut_op(11, [1, 2], 4, [1, -1], 42), "c0": lut_op(11, [1, 2], 3, [1, -1], 43),
                "coefficient": lut_op(11, [1, 2], 3, [1, 1], 42), "operand": lut_op(11, [1, 5], 3, [1, -1], 42),
                "operand order": lut_op(11, [2, 1], 3, [-1, 1], 42)}
    for what, other in variants.items():
        pl = plan_lut(L, [base, other])
        assert pl["shared"].tolist() == [-1, -1] and len(pl["rots"]) == 2, what
    same = lut_op(11, [1, 2], 3, [1, -1], 42)
    pl = plan_lut(L, [base, same, lut_op(12, [11], 0, [1], 0)])
    assert pl["shared"].tolist() == [-1, 0, -1] and len(pl["rots"]) == 2 and len(pl["kss"]) == 2
    assert pl["rots"][1][0] == 10                        # the reader of the shared result reads the first op's slot
    assert pl["levels"].tolist() == [1, 1, 2]
    # another key: not shared; sharing off: not shared
    assert plan_lut(L, [base, same], keys=[0, 1], nkeys=2)["shared"].tolist() == [-1, -1]
    assert plan_lut(L, [base, same], reuse=0)["shared"].tolist() == [-1, -1]
    # gates share by the rule they always had
    pl = plan_lut(L, [[2, 10, 1, 2, -1, 0, 0, 0, 0, 0], [2, 11, 2, 1, -1, 0, 0, 0, 0, 0]])
    assert pl["shared"].tolist() == [-1, 0] and len(pl["rots"]) == 1


def test_per_key_runs_hold_with_lut_ops(L):
    ops = [lut_op(10, [1], 2, [1], 5), [4, 11, 1, 2, -1, 0, 0, 0, 0, 0], lut_op(12, [2, 3], 1, [2, 2], 0),
           [16, 13, 1, 2, 3, 0, 0, 0, 0, 0], lut_op(14, [3], 0, [-1], 9)]
    keys = [2, 0, 1, 1, 0]
    pl = plan_lut(L, ops, keys=keys, nkeys=3)
    assert pl["depth"] == 1
    assert pl["rot_koff"].tolist() == [0, 2, 5, 6] and pl["ks_koff"].tolist() == [0, 2, 4, 5]
    assert pl["rot_key"].tolist() == [0, 0, 1, 1, 1, 2]
    assert pl["rots"][:, 8].tolist() == [-1, 0, 1, -1, -1, 2]                    # the LUT index travels with its rotation
    assert pl["rots"][5].tolist() == [1, 1, 1, 0, 5, 5, -1, 0, 2]
    assert pl["kss"][:, 3].tolist() == [11, 14, 12, 13, 10]


def test_existing_plan_entries_keep_their_words(L):
    """tfhe_hip_test_level_plan3 still gives eight words per rotation although the descriptor has nine."""
    ops = np.array([[32 + 8 * 1 + 5, 10, 1, 2, 3]], dtype=I32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    z = lambda n: np.zeros(n, I32)
    levels, sizes, rots = z(1), z(6), np.full(17, 99, I32)
    bufs = [z(2), z(2), z(2), z(2), z(2)]
    kss = z(4)
    assert L.tfhe_hip_test_level_plan3(p(ops), p(z(1)), 1, 1, 256, 0, p(levels), p(sizes), *[p(b) for b in bufs], p(rots), p(kss)) == 1
    assert rots[:8].tolist() == [1, 2, 2, -2, 0, 0, 3, 2] and (rots[8:] == 99).all()


# ---- the committed digests ----------------------------------------------------------------------------------------------
def test_fixture_file_covers_what_it_must():
    d = T.load_digests()
    for pname, count in T.CASES.items():
        cases = d["sets"][pname]["cases"]
        assert len(cases) == count
        N = {"P128": 1024, "P80": 1024, "P2048": 2048}[pname]
        assert [c["bbar"] for c in cases[:6]] == [0, 1, N - 1, N, N + 1, 2 * N - 1]
        assert {c["lut"]["kind"] for c in cases} == {"random", "sectors", "constant"}
        assert all(c["lut"]["mu"] != 1 << 29 for c in cases if c["lut"]["kind"] == "constant")
        assert {len(c["coefs"]) for c in cases} == {1, 2, 3}
        flat = [s for c in cases for s in c["coefs"]]
        assert min(flat) < 0 and 2 in flat and -2 in flat
    ch = d["chain"]
    assert ch["messages"] == 16 and ch["hops"] == 4 and ch["smallest_edge_distance"] > 1 / 32


@pytest.mark.parametrize("pname", list(T.CASES))
def test_three_cases_per_set_recomputed_from_the_oracle(oracle, pname):
    O = oracle
    d = T.load_digests()
    oks = O.KeySet(O.params(pname), d["key_seed"])
    cases = d["sets"][pname]["cases"]
    specs = T.case_specs(pname, oks.N)
    for i in (0, 4, len(cases) - 1):
        c = cases[i]
        assert {k: c[k] for k in ("coefs", "lut", "enc_seed", "bits", "force_bbar")} == \
               {k: specs[i][k] for k in ("coefs", "lut", "enc_seed", "bits", "force_bbar")}
        lin = T.linear(c["coefs"], T.case_inputs(O, oks, c), c["c0"])
        assert T.modswitch(lin[-1], oks.N) == c["bbar"] == O.lib().orc_modswitch(int(lin[-1]), 2 * oks.N)
        ct, u, acc = T.oracle_lut_bootstrap(O, oks, lin, T.lut_words(c["lut"], oks.N))
        assert T.sha256_words(ct) == c["sha256"] and [int(x) for x in ct[:4]] == c["first_words"]
        assert T.sha256_words(u) == c["sha256_extracted"] and T.sha256_words(acc) == c["sha256_accumulator"]
    oks.close()


def test_restatement_with_the_gate_polynomial_is_the_oracle_gate(oracle):
    """With v = 2^29 (1 + ... + X^(N-1)) the restatement reproduces the oracle's own bootstrap + key switch and its AND,
    in both exact evaluators."""
    O = oracle
    oks = O.KeySet(O.params("P128"), T.KEY_SEED)
    a, b = oks.encrypt(O.Rng(3), [1, 0])
    v = np.full(oks.N, 1 << 29, dtype=I32)
    lin = T.linear([1, 1], np.stack([a, b]), -(1 << 29))
    for mode in (1, 2):
        ct, u, _ = T.oracle_lut_bootstrap(O, oks, lin, v, mode=mode)
        assert (u == oks.bootstrap_woks(lin)).all()
        assert (ct == oks.gate("AND", a, b)).all()
    oks.close()
