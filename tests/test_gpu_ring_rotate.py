"""GPU tests of the ring LUT bootstrap (include/tfhe_hip.h "ring LUT bootstrap"; peba1_amd/csrc/ring_rotate.hip): the raw
launch word for word against the numpy restatement (tests/ring_rotate_common.py), against the tuned rotation kernels on a
noiseless table, against n successive launches of the rotating CMUX; a shared table; the row path through the planner's key
switch across a chunk boundary; decryption of an encrypted table under fresh and under server-computed indices; recorded
gates around the call.

The restatement is exact numpy: one step of N = 1,024 is twelve int64 convolutions, so the rotations at a set's own n are
few (three at n = 630, one at N = 2,048) and run on threads; the wide counts run at n = 2."""
import numpy as np
import pytest

import lut_common as T
import ring_rotate_common as R
import select_common as S
import unpack_common as U
from test_gpu_noise import predicted_variance

pytestmark = pytest.mark.gpu
I32 = np.int32
GADGET = {1024: (3, 7), 2048: (3, 6)}
FRONTIER = {1024: (9, 3), 2048: (7, 4)}              # the gadgets tests/golden/ntt_bounds_inputs_gadget_*.npz were searched at


@pytest.fixture(scope="module")
def api():
    from peba1_amd import api
    was = api.get_deferred()
    api.set_deferred(True)
    yield api
    api.set_deferred(was)


@pytest.fixture(scope="module")
def keys(api):
    """(N, n, gadget or None) -> (parameter set, device keyset, raw bootstrapping rows [n][2 l][2][N]); n = 0: the built-in set"""
    made = {}

    def get(N, n, gadget=None):
        k = (N, n, gadget)
        if k not in made:
            if n == 0:
                pp = api.ParameterSet(128) if N == 1024 else api.ParameterSet(p2048=True)
            else:
                pp = api.ParameterSet(custom=S.custom_tuple(n, N=N, gadget=gadget or GADGET[N]))
            ks = api.SecretKeySet(pp, 0x207A + N + n, device=True)
            made[k] = (pp, ks, R.bk_rows_of(ks.bk(), pp.n, pp.l, N).copy())
        return made[k]
    yield get
    for _, ks, _ in made.values():
        ks.close()


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6])


def frontier_sample(N, l, Bgbit):
    """A ring sample c with X^N c - c = -2 c carrying searched digit fields: rotated by abar = N its difference IS the
    magnitude-frontier word of one searched entry of the fixture, whose bits below the digits are zero."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_bounds_inputs_gadget_%d.npz" % N)
    with np.load(path) as z:
        names = sorted(k for k in z.files if k.endswith("/digits"))
        dig = z[names[-1]].astype(np.int64)
    assert dig.shape == (2 * l, N)
    off = S.decomp_offset(l, Bgbit)
    c = []
    for u in range(2):
        fields = sum((dig[u * l + p] + 2 ** (Bgbit - 1)) << (32 - (p + 1) * Bgbit) for p in range(l))
        diff = (fields - off) % 2 ** 32
        assert (diff % 2 == 0).all()
        c.append((-(diff // 2)) % 2 ** 32)                # -2 c = diff mod 2^32
    c = S.to_i32(np.stack(c))
    assert (np.concatenate([S.decompose(S.to_i32(-2 * c[u].astype(np.int64)), l, Bgbit) for u in range(2)]) == dig).all()
    return c


def inputs(rng, N, n, count, nring):
    """tables [nring][2][N], LWE words [count][n + 1]: sample 0 switches to abar_0 = N (with the frontier table: its digits),
    sample 1 to abar_0 = 0 and, where there is one, abar_1 = N + 5; the others are random"""
    lwe = np.stack([R.lwe_with_bars(rng, n, N, [N, 0][:n] + [0] if j == 0 else ([0, N + 5][:n] if j == 1 else [])) for j in range(count)])
    return S.random_ring(rng, nring, N), lwe


# (N, n or 0 = the set's own, counts): the wide counts at n = 2; 300 is more workgroups than the card has CUs, and the
# launcher does not chunk (a launch takes up to 65,536 rotations)
PARITY = [(1024, 1, (1, 3)), (1024, 2, (1, 3, 300)), (1024, 0, (3,)), (2048, 2, (1, 3)), (2048, 0, (1,))]


@pytest.mark.parametrize("N,n,counts", PARITY, ids=lambda v: str(v))
def test_raw_launch_word_for_word_against_the_restatement(api, keys, N, n, counts):
    pp, ks, rows = keys(N, n)
    rng = np.random.default_rng(N + n)
    for count in counts:
        tables, lwe = inputs(rng, N, pp.n, count, count)
        want = R.blind_rotate_many(rows, tables, None, lwe, pp.l, pp.Bgbit)
        bars = [R.switched(w, N) for w in lwe]
        assert bars[0][0] == N and (count < 2 or bars[1][0] == 0) and (count < 2 or pp.n < 2 or bars[1][1] >= N)
        assert_words(api.kernel_ring_rotate(ks, tables, lwe).reshape(count, 2, N), want, (N, pp.n, count, "ring"))
        assert_words(api.kernel_ring_rotate(ks, tables, lwe, rows=True), R.extract0(want), (N, pp.n, count, "rows"))
    assert api.last_error() == ""


@pytest.mark.parametrize("N", [1024, 2048])
def test_raw_launch_on_the_magnitude_frontier_digits(api, keys, N):
    """the searched digits of the CMUX fixture as the digits of a step's rotated difference, at the fixture's gadget"""
    l, Bgbit = FRONTIER[N]
    pp, ks, rows = keys(N, 2, (l, Bgbit))
    rng = np.random.default_rng(N)
    c = frontier_sample(N, l, Bgbit)
    lwe = np.stack([R.lwe_with_bars(rng, 2, N, [N, 0, 0]), R.lwe_with_bars(rng, 2, N, [0, N, 0]), R.lwe_with_bars(rng, 2, N, [N, 1, 0])])
    want = R.blind_rotate_many(rows, [c] * 3, None, lwe, l, Bgbit)
    assert_words(api.kernel_ring_rotate(ks, c[None], lwe, ring_index=[0, 0, 0]).reshape(3, 2, N), want, (N, "frontier"))


def test_noiseless_table_rows_equal_the_tuned_kernels(api, keys):
    """on (0, v) the rows are tfhe_hip_kernel_lut_bootstrap_woks', word for word (the restatement equals the oracle's LUT
    rotation: tests/test_ring_rotate_cpu.py)"""
    pp, ks, _ = keys(1024, 0)
    N, rng = pp.N, np.random.default_rng(5)
    polys = rng.integers(-2 ** 31, 2 ** 31, (3, N), dtype=np.int64).astype(I32)
    lin = np.stack([R.lwe_with_bars(rng, pp.n, N, b) for b in ([], [0, N + 1], [N], [2 * N - 1, 1])])
    which = np.array([0, 1, 2, 1], dtype=I32)
    want = api.kernel_lut_bootstrap_woks(ks, lin, which, polys)
    tables = np.stack([np.zeros_like(polys), polys], axis=1)
    assert_words(api.kernel_ring_rotate(ks, tables, lin, ring_index=which, rows=True), want, "rows on (0, v)")


def test_the_loop_equals_successive_rotating_cmux_launches(api, keys):
    """n = 3: the selector is made from the same key rows; X^(abar) is X^(-(2N - abar)), which the CMUX launch takes for
    abar above N (rot in 1 .. N - 1); bbar = 0"""
    pp, ks, rows = keys(1024, 3)
    N, rng = pp.N, np.random.default_rng(9)
    bars = [N + 1, 2 * N - 1, N + 700]
    tables = S.random_ring(rng, 2, N)
    lwe = np.stack([R.lwe_with_bars(rng, 3, N, bars + [0])] * 2)
    sel = api.Selector(pp, rows)
    try:
        acc = tables.reshape(2, -1)
        for i, a in enumerate(bars):
            acc = api.kernel_ring_cmux_rotate(sel, i, 2 * N - a, acc)
    finally:
        sel.close()
    assert_words(api.kernel_ring_rotate(ks, tables, lwe), acc, "composition")


def test_many_samples_rotate_one_table(api, keys):
    pp, ks, _ = keys(1024, 2)
    N, rng = pp.N, np.random.default_rng(11)
    tables, lwe = inputs(rng, N, 2, 6, 3)
    index = np.array([2, 0, 0, 1, 2, 0], dtype=I32)
    got = api.kernel_ring_rotate(ks, tables, lwe, ring_index=index)
    for j, t in enumerate(index):
        assert_words(got[j], api.kernel_ring_rotate(ks, tables[t][None], lwe[j][None])[0], ("shared table", j))


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("count", [1, 8193])
def test_row_path_word_for_word_across_a_chunk(api, keys, count, device):
    """tfhe_hip_ring_lut_bootstrap = the restatement's Extract_0, then the key-switch restatement of the unpack tests.
    run_rows chunks at 8,192 rows (UNPACK_CHUNK), above the 1,025 the issue names: 8,193 crosses it.  The 8,193 rotations
    name 2 tables and 4 distinct index words in every combination, so the restatement runs 8 rotations."""
    import torch
    pp, ks, rows = keys(1024, 2)
    N, rng = pp.N, np.random.default_rng(13 + count)
    tables, lwe4 = inputs(rng, N, 2, 4, 2)
    j = np.arange(count)
    which, index = (j % 4), ((j // 4) % 2).astype(I32)
    ref = R.blind_rotate_many(rows, tables, [t for t in (0, 1) for _ in range(4)], [lwe4[s] for _ in (0, 1) for s in range(4)], pp.l, pp.Bgbit)
    want8 = U.keyswitch_rows(ks.ksk(), R.extract0(ref), pp.n, N, pp.ks_t, pp.ks_basebit)
    ins = api.CiphertextArray(pp, count).set_words(lwe4[which])
    out = api.CiphertextArray(pp, count)
    src = torch.from_numpy(tables.reshape(-1)).cuda() if device else tables
    before = api.stats()["keyswitches"]
    api.ring_lut_bootstrap(src, ins, ks, out, ring_index=index, device=device)
    assert_words(out.words(), want8[index * 4 + which], ("row path", count, device))
    assert api.stats()["keyswitches"] - before == count and api.last_error() == ""
    for o in (ins, out):
        o.close()


def _table_sample(api, ks, table, seed):
    """an encrypted table of 2-bit values: entry m on the block of N / len(table) coefficients from m N / len(table), value v
    at phase (2 v + 1) / 16"""
    N = ks.params.N
    mu = np.repeat((2 * np.asarray(table, dtype=np.int64) + 1) << 28, N // len(table))
    return api.ring_encrypt(S.to_i32(mu), ks, seed=seed).reshape(1, -1)


def _stdevs(pp):
    return (pp.ptr.contents.in_out_params.contents.alpha_min, pp.ptr.contents.tgsw_params.contents.tlwe_params.contents.alpha_min)


def _check_lookups(api, pp, ks, out, want_phase, what):
    ph = U.lwe_phases(out.words(), ks.lwe_key()).astype(np.int64)
    err = np.abs(S.to_i32(ph - np.asarray(want_phase, dtype=np.int64))) / 2.0 ** 32
    ks_stdev, bk_stdev = _stdevs(pp)
    worst, typical, _ = predicted_variance(pp, ks_stdev, bk_stdev)      # (worst case, typical, the per-key mean's scale)
    print("%s: largest phase error %.3g, computed sigma %.3g typical, %.3g worst case (rotation and key switch, plus the table's own), "
          "half a sector %.3g" % (what, err.max(), (typical + bk_stdev ** 2) ** 0.5, (worst + bk_stdev ** 2) ** 0.5, 1 / 32))
    assert (err < 1 / 32).all(), (what, err)


def test_encrypted_table_decrypts_under_fresh_and_computed_indices(api, keys):
    """P128, an encrypted table of eight 2-bit values.  Every index m = 0 .. 7 as a fresh tfhe_hip_sym_encrypt_torus sample
    at phase (m + 1/2) / 16, the centre of block m on the negacyclic half torus: result m decrypts to table[m].  Then the
    index as tfhe_hip_linear of two gate outputs, 4.5/16 + g1 + g2 with g = +-1/8: phases 0.5/16, 4.5/16 and 8.5/16 --
    entries 0, 4 and, past the half torus, entry 0 NEGATED (X^N = -1).  The index of two gate outputs has sigma
    sqrt(2) 4.7e-3 = 6.6e-3 against the half block 1/32: 4.7 sigma; coefficients (1, 2) would reach four entries at 3
    sigma, too close to assert.  Only correct decryption is asserted; the phase errors are printed beside the computed
    sigma."""
    from peba1_amd import lib
    L = lib.load()
    pp, ks, _ = keys(1024, 0)
    L.tfhe_hip_set_encrypt_seed(31)
    table = np.random.default_rng(3).integers(0, 4, 8)
    ring = _table_sample(api, ks, table, seed=404)
    centre = (2 * table.astype(np.int64) + 1) << 28
    idx = api.CiphertextArray(pp, 8)
    for m in range(8):
        api.encrypt_torus(idx.at(m), (2 * m + 1) << 27, ks)
    out = api.CiphertextArray(pp, 8)
    api.ring_lut_bootstrap(ring, idx, ks, out, ring_index=[0] * 8)
    _check_lookups(api, pp, ks, out, centre, "fresh indices")
    bits = [(0, 0), (0, 1), (1, 0), (1, 1)]
    a = api.CiphertextArray(pp, 4).encrypt([b[0] for b in bits], ks)
    b = api.CiphertextArray(pp, 4).encrypt([b[1] for b in bits], ks)
    g1, g2, lin, out2 = (api.CiphertextArray(pp, 4) for _ in range(4))
    api.gate_batch("AND", g1, a, b, ks)
    api.gate_batch("OR", g2, a, b, ks)
    api.linear_batch(lin, [g1, g2], [1, 1], 9 << 27, ks)          # 4.5/16 + g1 + g2, recorded: the call flushes it
    api.ring_lut_bootstrap(ring, lin, ks, out2, ring_index=[0] * 4)
    m16 = [4.5 + 2 * ((2 * (x & y) - 1) + (2 * (x | y) - 1)) for x, y in bits]      # index phases in sixteenths
    want = [centre[int(m)] if m < 8 else -centre[int(m) - 8] for m in m16]
    assert sorted(set(m16)) == [0.5, 4.5, 8.5]
    _check_lookups(api, pp, ks, out2, want, "indices made by linear of two gate outputs")
    for o in (idx, out, a, b, g1, g2, lin, out2):
        o.close()


def test_recorded_gates_stay_recorded_and_results_are_gate_operands(api, keys):
    """a gate recorded before the call, on samples the call does not touch, is still recorded after it; two results are then
    the operands of a bootsAND that decrypts right"""
    from peba1_amd import lib
    L = lib.load()
    pp, ks, _ = keys(1024, 0)
    L.tfhe_hip_set_encrypt_seed(32)
    # entries at +-1/8, the gates' own encoding: table bit 1 -> 1/8, bit 0 -> -1/8
    tbits = [1, 0, 1, 1, 0, 0, 1, 0]
    mu = np.repeat(np.where(np.array(tbits) == 1, 1 << 29, -(1 << 29)).astype(np.int64), pp.N // 8)
    ring = api.ring_encrypt(S.to_i32(mu), ks, seed=405).reshape(1, -1)
    x = api.CiphertextArray(pp, 2).encrypt([1, 1], ks)
    early = api.CiphertextArray(pp, 1)
    L.bootsNAND(early.at(0), x.at(0), x.at(1), ks.cloud)
    before = api.stats()["blind_rotates"]
    idx = api.CiphertextArray(pp, 2)
    for j, m in enumerate((2, 3)):
        api.encrypt_torus(idx.at(j), (2 * m + 1) << 27, ks)
    out = api.CiphertextArray(pp, 2)
    api.ring_lut_bootstrap(ring, idx, ks, out, ring_index=[0, 0])
    assert api.stats()["blind_rotates"] == before, "the recorded NAND has not run"
    res = api.CiphertextArray(pp, 1)
    L.bootsAND(res.at(0), out.at(0), out.at(1), ks.cloud)
    assert api.flush() >= 1
    assert api.stats()["blind_rotates"] == before + 2
    assert list(out.decrypt(ks)) == [tbits[2], tbits[3]] and list(res.decrypt(ks)) == [tbits[2] & tbits[3]] and list(early.decrypt(ks)) == [0]
    for o in (x, early, idx, out, res):
        o.close()


def test_rotation_timing_between_stream_events(api, keys):
    from peba1_amd import lib
    pp, ks, _ = keys(1024, 2)
    rng = np.random.default_rng(17)
    tables, lwe = inputs(rng, pp.N, 2, 2, 2)
    ins = api.CiphertextArray(pp, 2).set_words(lwe)
    L = lib.load()
    L.tfhe_hip_set_kernel_timing(1)
    try:
        api.ring_blind_rotate(tables, ins, ks)
        assert api.last_ring_rotate_ms() > 0
    finally:
        L.tfhe_hip_set_kernel_timing(0)
    assert_words(api.ring_blind_rotate(tables, ins, ks), api.kernel_ring_rotate(ks, tables, lwe), "pool samples against caller words")
    ins.close()


def test_tree_lut_over_all_sixteen_inputs(api, keys):
    """circuits.tree_lut on a random 4 x 4 -> 2-bit table, every pair (hi, lo) of digits as fresh samples at phase
    (m + 1/2) / 8: all sixteen results decrypt to tables[hi][lo].  S = 4 stands: the COMPUTED variance of a result
    (circuits.tree_lut_variance, at P128) is 2 V + pack with V = 1.2e-5 the typical variance of one gate bootstrap's output
    (rotation 6.3e-6 with E[dig^2] = Bg^2 / 12, key switch 5.7e-6) and pack = n t N E[d^2] bk^2 + (n / 2) prec^2 / 3 = 2.2e-8
    for the N samples of one pack: sigma 4.9e-3, six of them 0.029, under the half sector 1/16 = 0.0625.  The blocks are N / S
    copies of one sample, so the figure does not depend on S and the fallback S = 2 is not needed.  An index digit is a fresh
    sample: its sigma in coefficients is sqrt((1 + n / 2) / 12) = 5.1 from the modulus switch against the half block 128."""
    from peba1_amd import circuits, lib
    pp, ks, _ = keys(1024, 0)
    lib.load().tfhe_hip_set_encrypt_seed(33)
    side = 4
    sigma = circuits.tree_lut_variance(pp) ** 0.5
    print("tree_lut: computed sigma %.3g, six sigma %.3g, half a sector %.3g" % (sigma, 6 * sigma, 1 / 16))
    assert 6 * sigma < 1 / 16
    tables = np.random.default_rng(21).integers(0, 4, (side, side))
    pairs = [(h, lo) for h in range(side) for lo in range(side)]
    x_hi, x_lo = api.CiphertextArray(pp, 16), api.CiphertextArray(pp, 16)
    for i, (h, lo) in enumerate(pairs):
        api.encrypt_torus(x_hi.at(i), circuits.digit_phase(h, side), ks)
        api.encrypt_torus(x_lo.at(i), circuits.digit_phase(lo, side), ks)
    pkey = api.PackingKey(ks, seed=77)
    out = circuits.tree_lut(tables, x_hi, x_lo, ks, pkey)
    want = np.array([(2 * int(tables[h][lo]) + 1) << 28 for h, lo in pairs], dtype=np.int64)
    ph = U.lwe_phases(out.words(), ks.lwe_key()).astype(np.int64)
    err = np.abs(S.to_i32(ph - want)) / 2.0 ** 32
    print("tree_lut: largest phase error %.3g" % err.max())
    assert [int(x) for x in T.decode((ph % 2 ** 32) / 2.0 ** 32)] == [int(tables[h][lo]) for h, lo in pairs]
    pkey.close()
    for o in (x_hi, x_lo, out):
        o.close()


def test_protocol_ring_lut_run(api):
    """protocol.py --ring-lut: every digit's lookup under the server-computed index decrypts to the table's entry"""
    from peba1_amd import protocol
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    table, perm = [3, 0, 2, 1, 1, 3, 0, 2], [5, 2, 7, 0, 3, 6, 1, 4]
    outs = list(protocol.run_ring_lut(pp, ks, table, perm))
    assert len(outs) == 8 and all(o["decrypted"] == o["plain"] == table[perm[o["x"]]] for o in outs), outs
    ks.close()
