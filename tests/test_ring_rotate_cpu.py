"""The ring LUT bootstrap without a GPU: the new symbols, the restatement (tests/ring_rotate_common.py) against the oracle's
own LUT blind rotation on a noiseless table (0, v), the rotation X^(-r) for every kind of r against a direct negacyclic
product, every refusal that is decided before the device is looked at, and decryption of the restatement's output for all
eight indices of an eight-entry table under a real key."""
import ctypes as C
import time

import numpy as np
import pytest

import lut_common as T
import ring_rotate_common as R
import select_common as S
import unpack_common as U

N = 1024
L_GADGET, BGBIT = 3, 7
NEW_SYMBOLS = ("tfhe_hip_ring_blind_rotate", "tfhe_hip_ring_blind_rotate_device", "tfhe_hip_ring_lut_bootstrap",
               "tfhe_hip_ring_lut_bootstrap_device", "tfhe_hip_kernel_ring_rotate", "tfhe_hip_last_ring_rotate_ms")


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_the_new_symbols_exist(L):
    from peba1_amd import api
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ("ring_blind_rotate", "ring_lut_bootstrap", "kernel_ring_rotate", "last_ring_rotate_ms"):
        assert callable(getattr(api, name)), name


@pytest.mark.parametrize("n", [4, 9])
def test_restatement_on_a_noiseless_table_is_the_oracles_lut_rotation(oracle, n):
    """(0, v) rotated by the restatement = the oracle's LUT blind rotation before the key switch, word for word: the
    accumulator and the extracted sample.  The modulus switch used is the oracle's on every word of the inputs."""
    oks = oracle.KeySet(oracle.custom_params(n=n, N=N, l=L_GADGET, Bgbit=BGBIT), 0xB11D + n)
    rng = np.random.default_rng(100 + n)
    rows = R.bk_rows_of(oks.bk(), n, L_GADGET, N)
    for case in range(3):
        v = rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(np.int32)
        # case 1 forces abar_0 = 0 (a skipped step) and abar_1 >= N
        lin = R.lwe_with_bars(rng, n, N, [0, N + 3] if case == 1 else [])
        assert R.switched(lin, N) == [oracle.lib().orc_modswitch(int(x), 2 * N) for x in lin]
        _, want_u, want_acc = T.oracle_lut_bootstrap(oracle, oks, lin, v)
        c = np.stack([np.zeros(N, dtype=np.int32), v])
        got = R.blind_rotate_ref(rows, c, lin, L_GADGET, BGBIT)
        assert np.array_equal(got.reshape(-1), want_acc), (n, case, np.flatnonzero(got.reshape(-1) != want_acc)[:4])
        assert np.array_equal(R.extract0(got)[0], want_u), (n, case)
    oks.close()


@pytest.mark.parametrize("r", [0, 1, N - 1, N, N + 1, 2 * N - 1])
def test_rotation_against_a_direct_negacyclic_product(r):
    """X^(-r) c = c times the monomial X^(2N - r) in Z[X]/(X^N + 1), X^N = -1; and ACC_0 of a rotation whose mask words all
    switch to zero (every step skipped) is X^(-bbar) c."""
    rng = np.random.default_rng(r)
    c = S.random_ring(rng, 1, N)[0]
    s = (2 * N - r) % (2 * N)
    mono = np.zeros(N, dtype=np.int64)
    mono[s % N] = -1 if s >= N else 1
    want = U.to_i32(np.stack([S.negacyclic(c[u], mono) for u in range(2)]))
    assert np.array_equal(R.rotate_any(c, r), want)
    lwe = R.lwe_with_bars(rng, 2, N, [0, 0, r])
    rows = S.random_ring(rng, 2 * 2 * L_GADGET, N).reshape(2, 2 * L_GADGET, 2, N)
    assert np.array_equal(R.blind_rotate_ref(rows, c, lwe, L_GADGET, BGBIT), want)


def test_a_computed_zero_step_leaves_the_words_of_a_skipped_one():
    rng = np.random.default_rng(8)
    c = S.random_ring(rng, 1, N)[0]
    G = S.random_ring(rng, 2 * L_GADGET, N)
    assert np.array_equal(S.cmux(G, R.rotate_any(c, 0), c, L_GADGET, BGBIT), c)


def test_argument_errors_are_decided_on_the_host(L):
    """every refusal of the new entries that is decided before the device is looked at (this test runs without one): -1, a
    message, samples with their values and without slots, raw outputs untouched"""
    from peba1_amd import api
    n = 11
    pp = api.ParameterSet(custom=S.custom_tuple(n))
    ks = api.SecretKeySet(pp, 0x0707, device=False)
    cts = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    res = api.CiphertextArray(pp, 4).encrypt([0, 0, 1, 0], ks)
    held, held_res = cts.words().copy(), res.words().copy()
    other_pp = api.ParameterSet(custom=S.custom_tuple(n + 2))
    other_cts = api.CiphertextArray(other_pp, 4)
    ring = S.random_ring(np.random.default_rng(4), 3, N).reshape(-1)
    lwe = np.zeros((4, n + 1), dtype=np.int32)
    out = np.full((4, 2 * N), 7, dtype=np.int32)

    def refused(rc, needle):
        assert rc == -1 and needle in api.last_error(), (rc, needle, api.last_error())
        for a, h in ((cts, held), (res, held_res)):
            assert [a.at(j).contents.slot for j in range(4)] == [-1] * 4 and np.array_equal(a.words(), h)
        assert (out == 7).all()
        L.tfhe_hip_clear_error()

    def idx(*v):
        a = np.array(v, dtype=np.int32)
        return a, _i32p(a)

    for device in (False, True):
        src = C.c_void_p(ring.ctypes.data) if device else _i32p(ring)
        dst = C.c_void_p(out.ctypes.data) if device else _i32p(out)
        rot = L.tfhe_hip_ring_blind_rotate_device if device else L.tfhe_hip_ring_blind_rotate
        lut = L.tfhe_hip_ring_lut_bootstrap_device if device else L.tfhe_hip_ring_lut_bootstrap
        for call, last in ((rot, dst), (lut, res.ptr)):
            refused(call(None, src, 3, None, cts.ptr, 2, last), "null cloud key")
            for count in (0, -1, 65537):
                refused(call(ks.cloud, src, 3, None, cts.ptr, count, last), "count must be in 1..65536")
            refused(call(ks.cloud, src, 0, None, cts.ptr, 1, last), "nring must be at least 1")
            refused(call(ks.cloud, src, 3, None, cts.ptr, 4, last), "count runs past the last of the ring samples")
            for bad in ((0, 3), (-1, 0), (2, 1 << 20)):
                keep, p = idx(*bad)
                refused(call(ks.cloud, src, 3, p, cts.ptr, 2, last), "is outside 0..2")
            refused(call(ks.cloud, None, 3, None, cts.ptr, 2, last), "null ring words")
            refused(call(ks.cloud, src, 3, None, None, 2, last), "null ring words")
            refused(call(ks.cloud, src, 3, None, cts.ptr, 2, None), "null ring words")
            refused(call(ks.cloud, src, 3, None, other_cts.ptr, 2, last), "LWE dimension")
            keep, p = idx(0, 0, 0, 0, 0)
            refused(call(ks.cloud, src, 3, p, cts.ptr, 5, last), "past the end of the index samples' array")
        refused(lut(ks.cloud, src, 3, None, cts.ptr, 2, other_cts.ptr), "LWE dimension")
        keep, p = idx(0, 0, 0, 0)
        refused(lut(ks.cloud, src, 3, p, cts.ptr, 4, res.at(1)), "past the end of the result array")
    refused(L.tfhe_hip_ring_blind_rotate_device(ks.cloud, C.c_void_p(ring.ctypes.data + 4), 3, None, cts.ptr, 2, C.c_void_p(out.ctypes.data)),
            "16-byte aligned")
    refused(L.tfhe_hip_ring_blind_rotate_device(ks.cloud, C.c_void_p(ring.ctypes.data), 3, None, cts.ptr, 2, C.c_void_p(ring.ctypes.data + 16 * N)),
            "overlaps")
    refused(L.tfhe_hip_ring_lut_bootstrap_device(ks.cloud, C.c_void_p(ring.ctypes.data + 4), 3, None, cts.ptr, 2, res.ptr), "16-byte aligned")
    raw = L.tfhe_hip_kernel_ring_rotate
    refused(raw(None, _i32p(ring), 3, None, _i32p(lwe), 2, _i32p(out), None), "null cloud key")
    refused(raw(ks.cloud, _i32p(ring), 3, None, _i32p(lwe), 0, _i32p(out), None), "count must be in 1..65536")
    keep, p = idx(0, 3)
    refused(raw(ks.cloud, _i32p(ring), 3, p, _i32p(lwe), 2, _i32p(out), None), "is outside 0..2")
    refused(raw(ks.cloud, None, 3, None, _i32p(lwe), 2, _i32p(out), None), "null argument")
    refused(raw(ks.cloud, _i32p(ring), 3, None, None, 2, _i32p(out), None), "null argument")
    refused(raw(ks.cloud, _i32p(ring), 3, None, _i32p(lwe), 2, None, None), "null argument")
    assert L.tfhe_hip_last_ring_rotate_ms() == -1.0
    for o in (cts, res, other_cts):
        o.close()
    ks.close()


def test_a_ring_the_kernel_is_not_built_for_is_refused_by_the_entries(L):
    """k != 1 and N outside {1024, 2048}: a host-only keyset of such a set exists (no device image is asked for), and every
    new entry refuses it by the ring, on the host, before anything else about the operands is looked at"""
    from peba1_amd import api
    for custom in (S.custom_tuple(5, N=512), (5, 1024, 2) + S.custom_tuple(5)[3:]):
        L.tfhe_hip_clear_error()
        pp = api.ParameterSet(custom=custom)
        ks = api.SecretKeySet(pp, 3, device=False)
        cts, res = api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 1)
        ring = np.zeros(2 * (pp.k + 1) * pp.N, dtype=np.int32)
        out = np.zeros_like(ring)
        lwe = np.zeros(pp.n + 1, dtype=np.int32)
        for call in (lambda: L.tfhe_hip_ring_blind_rotate(ks.cloud, _i32p(ring), 1, None, cts.ptr, 1, _i32p(out)),
                     lambda: L.tfhe_hip_ring_lut_bootstrap(ks.cloud, _i32p(ring), 1, None, cts.ptr, 1, res.ptr),
                     lambda: L.tfhe_hip_kernel_ring_rotate(ks.cloud, _i32p(ring), 1, None, _i32p(lwe), 1, _i32p(out), None)):
            rc = call()
            assert rc == -1 and "N = 1024 or 2048 and k = 1" in api.last_error(), (custom[:3], rc, api.last_error())
            L.tfhe_hip_clear_error()
        assert not out.any() and res.at(0).contents.slot < 0
        for o in (cts, res):
            o.close()
        ks.close()


def test_every_index_of_an_eight_entry_table_decrypts(oracle):
    """An encrypted table of eight 2-bit values, entry m on the block of N / 8 coefficients from m N / 8 at amplitude
    (2 v + 1) / 16, looked up under a real P128 key (n = 630) by the restatement for every index m = 0 .. 7, the index
    sample at phase (m + 1/2) / 16 (the negacyclic half torus, centred on its block): Extract_0 of the result decrypts to
    table[m] under the ring key.  630 steps of six exact products take about ten seconds a rotation in numpy; the eight
    rotations run on as many threads."""
    oks = oracle.KeySet(oracle.params("P128"), 0x7AB1E)
    n, rng = oks.n, np.random.default_rng(77)
    table = rng.integers(0, 4, 8)
    msg = np.repeat((2 * table + 1) << 28, N // 8).astype(np.int64)
    skey, lkey = np.asarray(oks.tlwe_key(), dtype=np.int64), np.asarray(oks.lwe_key(), dtype=np.int64)
    a = rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64)
    e = np.rint(rng.normal(0, 2.0 ** -25, N) * 2.0 ** 32).astype(np.int64)
    b = S.negacyclic(a % 2 ** 32 >> 16, skey) * 65536 + S.negacyclic(a % 2 ** 16, skey) + msg + e
    c = U.to_i32(np.stack([a, b]))
    assert np.abs(U.to_i32(S.ring_phases(c, skey).astype(np.int64) - msg)).max() < 1 << 12     # (6 sigma of 2^-25 is 2^9.6)
    lwes = []
    for m in range(8):
        am = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64)
        em = int(np.rint(rng.normal(0, 2.0 ** -15) * 2.0 ** 32))
        lwes.append(U.to_i32(np.append(am, (am % 2 ** 32) @ lkey + ((2 * m + 1) << 27) + em)))
    rows = R.bk_rows_of(oks.bk(), n, L_GADGET, N)
    t0 = time.time()
    acc = R.blind_rotate_many(rows, [c] * 8, None, lwes, L_GADGET, BGBIT, workers=8)
    print("eight rotations at n = %d in %.1f s" % (n, time.time() - t0))
    ph = U.extracted_phases(R.extract0(acc), skey).astype(np.int64) % 2 ** 32
    assert [int(x) for x in T.decode(ph / 2.0 ** 32)] == [int(v) for v in table]
    err = np.abs(U.to_i32(ph - ((2 * table + 1) << 28)))
    print("largest phase error %.3g (torus; half a sector is 1/16)" % (err.max() / 2.0 ** 32))
    oks.close()
