"""Encrypted inner products without a GPU: the polynomial TGSW encryptor against the bit encryptor, the definitions of
include/tfhe_hip.h restated in numpy and Python integers (tests/inner_common.py over tests/select_common.py) -- the product
decrypts to p t, coefficient e w is the entry's inner product and no other entry enters it --, the error channel of the
new entries and the decision band against hand-computed values, on host-only keysets."""
import ctypes as C

import numpy as np
import pytest

import inner_common as K
import select_common as S

N, L_GADGET, BGBIT = S.SETS["P128"]
N_LWE = 11
BK_STDEV = S.STDEVS[1]


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def small():
    from peba1_amd import api
    pp = api.ParameterSet(custom=S.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, 0x1AE2, device=False)
    yield pp, ks
    ks.close()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_constant_polynomials_give_the_bit_encryptors_words(small):
    """the seeded polynomial encryptor on the constant polynomials 0 / 1 equals tfhe_hip_tgsw_encrypt_bits_seeded word for word"""
    from peba1_amd import api
    pp, ks = small
    bits = [1, 0, 1]
    polys = np.zeros((3, N), dtype=np.int32)
    polys[:, 0] = bits
    got, want = api.tgsw_encrypt_polys(polys, ks, seed=0x77), api.tgsw_encrypt_bits(bits, ks, seed=0x77)
    assert got.shape == want.shape == (3, 2 * L_GADGET, 2, N) and np.array_equal(got, want)
    assert not np.array_equal(got, api.tgsw_encrypt_polys(polys, ks, seed=0x78))
    assert not np.array_equal(api.tgsw_encrypt_polys(polys, ks), api.tgsw_encrypt_polys(polys, ks))


def test_rows_of_a_polynomial_sample_carry_the_shifted_polynomial(small):
    """row (u = k, r) decrypts to p[j] << (32 - (r+1) Bgbit) at every coefficient j, up to the fresh noise (7 sigma)"""
    from peba1_amd import api
    pp, ks = small
    p = np.random.default_rng(2).integers(-3, 4, N)
    G = api.tgsw_encrypt_polys(p[None, :], ks, seed=5)[0]
    ph = S.ring_phases(G, ks.tlwe_key()).astype(np.int64)
    for r in range(L_GADGET):
        want = S.to_i32(p.astype(np.int64) << (32 - (r + 1) * BGBIT)).astype(np.int64)
        err = (ph[L_GADGET + r] - want + 2 ** 31) % 2 ** 32 - 2 ** 31
        assert np.abs(err).max() < 7 * BK_STDEV * 2 ** 32, r


@pytest.mark.parametrize("w", [1, 16, 128, 1024])
def test_the_product_decrypts_to_p_t_and_coefficient_ew_is_the_inner_product(small, w):
    """G (.) c through the exact external product of the restatement, for a random +-1 probe and a gallery sample of bits at
    amplitude Delta: every coefficient of the phase is that of p t (Python integers, from the definition) within 7 sigma of
    the header's variance; coefficient e w is sum_i s_i t[e w + i]; zeroing one entry changes that entry's coefficient
    among the coefficients e w and no other"""
    from peba1_amd import api, identify
    pp, ks = small
    rng = np.random.default_rng(100 + w)
    per, delta = N // w, identify.inner_delta(w)
    s = 1 - 2 * rng.integers(0, 2, w)
    bits = rng.integers(0, 2, (per, w))
    if w > 1:
        bits[:, 0] = 1                                           # (every entry has weight: zeroing it must show)
    else:
        bits[:] = 1
    t = (bits.reshape(-1) * delta).astype(np.int64)
    p = K.probe_poly(s, N)
    assert np.array_equal(p, identify.hamming_probe_poly((1 - s) // 2, N))
    pt = K.negacyclic_python(p, t)
    for e in range(per):
        assert pt[e * w] == sum(int(s[i]) * int(t[e * w + i]) for i in range(w)), e
    # no other entry's coefficients contribute: zero entry z, only coefficient z w of the coefficients e w changes
    z = per // 2
    t0 = t.copy()
    t0[z * w:(z + 1) * w] = 0
    pt0 = K.negacyclic_python(p, t0)
    changed = [e for e in range(per) if pt0[e * w] != pt[e * w]]
    assert changed == [z] and pt0[z * w] == 0
    # the ciphertext level
    G = api.tgsw_encrypt_polys(p[None, :].astype(np.int32), ks, seed=300 + w)[0]
    # (centred for the decomposition, as pack_gallery_inner leaves a gallery: without the half step the truncation's mean
    # eps shows as a bias of sum(s) (1 + N/2) eps, beyond 7 sigma at w = 128)
    c = identify.inner_round_gallery(api.ring_encrypt(t.astype(np.int32), ks, seed=400 + w), pp).reshape(2, N)
    assert np.array_equal(c.astype(np.int64) - api.ring_encrypt(t.astype(np.int32), ks, seed=400 + w).reshape(2, N), np.full((2, N), 2 ** 10))
    out = K.product(G, c, L_GADGET, BGBIT)
    ph = S.ring_phases(out, ks.tlwe_key()).astype(np.int64)
    err = (ph - np.array([v % 2 ** 32 for v in pt], dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31
    sigma = K.inner_variance(N, L_GADGET, BGBIT, BK_STDEV, float(w), BK_STDEV ** 2) ** 0.5
    assert np.abs(err).max() < 7 * sigma * 2 ** 32, (w, np.abs(err).max() / 2.0 ** 32, sigma)
    # the SAME sample as tfhe_hip_ring_encrypt leaves it, not centred: the error is the header's bias, to the same 7 sigma
    # (the dropped bits have the variance eps^2 / 3 either way) -- and at w = 128 the bias alone is beyond them
    raw = api.ring_encrypt(t.astype(np.int32), ks, seed=400 + w).reshape(2, N)
    ph_raw = S.ring_phases(K.product(G, raw, L_GADGET, BGBIT), ks.tlwe_key()).astype(np.int64)
    err_raw = (ph_raw - np.array([v % 2 ** 32 for v in pt], dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31
    bias = K.truncation_bias(p, ks.tlwe_key(), L_GADGET, BGBIT)
    assert np.abs(err_raw - bias).max() < 7 * sigma * 2 ** 32, (w, np.abs(err_raw - bias).max() / 2.0 ** 32)
    assert np.abs(bias).max() <= abs(int(s.sum())) * (1 + N // 2) * 2 ** 10 + w * 2 ** 10
    if w == 128:
        assert np.abs(err_raw).max() > 7 * sigma * 2 ** 32
    # and the extracted row of entry e has the phase of coefficient e w
    rows = K.inner_rows(out[None], min(per, 5), w)
    assert np.array_equal(K.row_phases(rows, ks.tlwe_key()), S.to_i32(ph[np.arange(min(per, 5)) * w]))


def test_header_variance_at_p128():
    """the figures the header quotes: 2.2e-8 + 2.5e-9 + 1e-13, sigma ~ 1.6e-4 at w = 128"""
    eps = 2.0 ** -(L_GADGET * BGBIT + 1)
    key, rnd, inp = 2 * L_GADGET * N * 64.0 ** 2 * BK_STDEV ** 2, (1 + N) * 128 * eps ** 2 / 3, 128 * BK_STDEV ** 2
    assert abs(key - 2.2e-8) < 1e-9 and abs(rnd - 2.5e-9) < 1e-10 and abs(inp - 1.1e-13) < 1e-14
    assert abs(K.inner_variance(N, L_GADGET, BGBIT, BK_STDEV, 128.0, BK_STDEV ** 2) ** 0.5 - 1.6e-4) < 1e-5


def test_encryptor_errors_leave_the_output_untouched(small, L):
    from peba1_amd import api
    pp, ks = small
    polys = np.ones((21, N), dtype=np.int32)
    out = np.full(8, 7, dtype=np.int32)                          # (a refused call writes nothing: eight words are enough)
    for args, needle in (((ks.ptr, _i32p(polys), 0, _i32p(out)), "count must be in 1..20"),
                         ((ks.ptr, _i32p(polys), 21, _i32p(out)), "count must be in 1..20"),
                         ((None, _i32p(polys), 1, _i32p(out)), "null argument"),
                         ((ks.ptr, None, 1, _i32p(out)), "null argument"),
                         ((ks.ptr, _i32p(polys), 1, None), "null argument")):
        for entry, extra in ((L.tfhe_hip_tgsw_encrypt_polys, ()), (L.tfhe_hip_tgsw_encrypt_polys_seeded, (5,))):
            assert entry(*args, *extra) == -1 and needle in api.last_error(), (needle, api.last_error())
            L.tfhe_hip_clear_error()
            assert (out == 7).all()


def test_center_words_adds_half_a_step_and_refuses_without_effect(small, L):
    from peba1_amd import api, identify
    pp, ks = small
    w = np.array([0, -1, 2 ** 31 - 1, -2 ** 31, 12345], dtype=np.int32)
    got = identify.inner_round_gallery(w, pp)
    assert np.array_equal(got, S.to_i32(w.astype(np.int64) + 2 ** (31 - L_GADGET * BGBIT))) and w[1] == -1      # (a copy)
    held = w.copy()
    for args, needle in (((None, _i32p(w), 5), "null argument"), ((pp.ptr, None, 5), "null argument"),
                         ((pp.ptr, _i32p(w), -1), "count must not be negative")):
        assert L.tfhe_hip_ring_center_words(*args) == -1 and needle in api.last_error()
        L.tfhe_hip_clear_error()
        assert np.array_equal(w, held)
    assert L.tfhe_hip_ring_center_words(pp.ptr, _i32p(w), 0) == 0 and np.array_equal(w, held)
    with pytest.raises(ValueError):
        identify.hamming_probe([0, 1, 1], 128, ks)


def test_inner_argument_errors_leave_results_untouched(small, L):
    """every refusal of tfhe_hip_ring_inner and of the two raw entries that is decided before the device is looked at (this
    test runs without one): -1, a message, results with their values and without slots, raw outputs untouched"""
    from peba1_amd import api
    pp, ks = small
    cts = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    held = cts.words().copy()
    other_pp = api.ParameterSet(custom=S.custom_tuple(N_LWE + 2))
    other_cts = api.CiphertextArray(other_pp, 4)
    pp2048 = api.ParameterSet(custom=S.custom_tuple(N_LWE, N=2048, gadget=(3, 6)))
    ring = S.random_ring(np.random.default_rng(4), 2, N).reshape(-1)
    words = S.random_ring(np.random.default_rng(5), 2 * 2 * L_GADGET, N).reshape(2, 2 * L_GADGET, 2, N)
    sel = api.Selector(pp, words)
    sel2048 = api.Selector(pp2048, S.random_ring(np.random.default_rng(6), 6, 2048))
    dead = api.Selector(pp, words)
    dead_ptr = dead.ptr
    dead.close()
    raw_out = np.full((2, 2 * N), 7, dtype=np.int32)

    def refused(rc, needle):
        assert rc == -1 and needle in api.last_error(), (rc, needle, api.last_error())
        assert [cts.at(j).contents.slot for j in range(4)] == [-1] * 4 and np.array_equal(cts.words(), held)
        assert (raw_out == 7).all()
        L.tfhe_hip_clear_error()

    for entry in (L.tfhe_hip_ring_inner, L.tfhe_hip_ring_inner_device):
        src = _i32p(ring) if entry is L.tfhe_hip_ring_inner else C.c_void_p(ring.ctypes.data)
        refused(entry(sel.ptr, 0, ks.cloud, None, 2, N, cts.ptr), "null ring words or result")
        refused(entry(sel.ptr, 0, ks.cloud, src, 2, N, None), "null ring words or result")
        refused(entry(sel.ptr, 0, None, src, 2, N, cts.ptr), "null cloud key")
        refused(entry(None, 0, ks.cloud, src, 2, N, cts.ptr), "null or deleted selector")
        refused(entry(dead_ptr, 0, ks.cloud, src, 2, N, cts.ptr), "null or deleted selector")
        refused(entry(sel.ptr, 2, ks.cloud, src, 2, N, cts.ptr), "sample_index must be in 0..1")
        refused(entry(sel.ptr, -1, ks.cloud, src, 2, N, cts.ptr), "sample_index must be in 0..1")
        refused(entry(sel2048.ptr, 0, ks.cloud, src, 2, N, cts.ptr), "different rings")
        for width in (0, 3, 96, 2 * N, -4):
            refused(entry(sel.ptr, 0, ks.cloud, src, 2, width, cts.ptr), "width must be a power of two in 1..1024")
        refused(entry(sel.ptr, 0, ks.cloud, src, 0, N, cts.ptr), "M must be at least 1")
        refused(entry(sel.ptr, 0, ks.cloud, src, 5, 512, cts.ptr), "past the end of the result array")
        refused(entry(sel.ptr, 0, ks.cloud, src, 2, N, other_cts.ptr), "LWE dimension")
    refused(L.tfhe_hip_ring_inner_device(sel.ptr, 0, ks.cloud, C.c_void_p(ring.ctypes.data + 4), 2, N, cts.ptr), "16-byte aligned")
    prod, rows = L.tfhe_hip_kernel_ring_product, L.tfhe_hip_kernel_ring_inner_rows
    refused(prod(None, 0, _i32p(ring), 2, _i32p(raw_out)), "null or deleted selector")
    refused(prod(sel.ptr, 0, None, 2, _i32p(raw_out)), "null argument")
    refused(prod(sel.ptr, 0, _i32p(ring), 2, None), "null argument")
    refused(prod(sel.ptr, 2, _i32p(ring), 2, _i32p(raw_out)), "bit_index must be in 0..1")
    refused(prod(sel.ptr, 0, _i32p(ring), 0, _i32p(raw_out)), "count must be in 1..65536")
    refused(rows(sel.ptr, 0, _i32p(ring), 2, 2, 48, _i32p(raw_out)), "width must be a power of two")
    refused(rows(sel.ptr, 0, _i32p(ring), 2, 8, 128, _i32p(raw_out)), "M must name an entry of the last")
    refused(rows(sel.ptr, 0, _i32p(ring), 2, 17, 128, _i32p(raw_out)), "M must name an entry of the last")
    refused(rows(sel.ptr, 0, _i32p(ring), 2, 9, 128, None), "null argument")
    for o in (sel, sel2048):
        o.close()
    for o in (cts, other_cts):
        o.close()


def test_decision_band_against_hand_computed_values():
    """P128: key switch 1024 * 8 * 2^-30 = 7.629e-6 and (1024 / 2) 2^-34 / 3 = 9.9e-9, modulus switch 316 / (12 * 2048^2) =
    6.278e-6: sigma_dec = 3.731e-3, 6 sigma = 2.238e-2.  w = 128: Delta = 2^-9, 6 sigma / Delta = 11.46 -> g = 12 (11.5
    Delta = 2.246e-2).  w = 16: Delta = 2^-6, 1.43 -> g = 2."""
    from peba1_amd import api, identify
    pp = api.ParameterSet(128)
    sigma = identify.inner_decision_sigma(pp)
    assert abs(sigma - 3.731e-3) < 2e-6
    assert identify.inner_decision_band(pp, 128) == 12 and identify.inner_decision_band(pp, 16) == 2
    for w, g in ((128, 12), (16, 2)):
        delta = 2.0 ** -(int(np.log2(w)) + 2)
        assert identify.inner_delta(w) == int(delta * 2 ** 32)
        assert (g - 0.5) * delta >= 6 * sigma > (g - 1.5) * delta
    assert abs(1.9 - sigma / 2.0 ** -9) < 0.02                  # "1.9 Delta at w = 128"
