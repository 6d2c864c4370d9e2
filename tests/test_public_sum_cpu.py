"""Public products over several ring samples without a GPU: the new symbols, every refusal that is decided before the device
is looked at, the bounds as the header states them, the numpy restatement (tests/public_sum_common.py) against
public_common's product at terms = 1, the gallery builders of peba1_amd.identify, the masked decision identity in plain
integers and the computed decision band, on host-only keysets."""
import ctypes as C

import numpy as np
import pytest

import public_common as K
import public_sum_common as Q

N = 1024
N_LWE = 11
NEW_SYMBOLS = ("tfhe_hip_ring_mul_public_sum", "tfhe_hip_ring_mul_public_sum_device", "tfhe_hip_ring_inner_public_sum",
               "tfhe_hip_ring_inner_public_sum_device", "tfhe_hip_kernel_ring_public_sum_product",
               "tfhe_hip_kernel_ring_public_sum_rows", "tfhe_hip_test_public_sum_bounds")


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def small():
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, 0x9B1D, device=False)
    yield pp, ks
    ks.close()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_the_new_symbols_exist(L):
    from peba1_amd import api, identify
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in ("ring_mul_public_sum", "ring_inner_public_sum", "kernel_ring_public_sum_product", "kernel_ring_public_sum_rows"):
        assert callable(getattr(api, name)), name
    for name in ("clear_gallery_polys_long", "hamming_probe_ring_long", "match_clear_gallery_long", "masked_gallery_polys",
                 "masked_probe_ring", "match_clear_gallery_masked", "clear_decision_band"):
        assert callable(getattr(identify, name)), name
    assert api.PUBLIC_MAX_TERMS == Q.MAX_TERMS == 8


@pytest.mark.parametrize("n_ring", [1024, 2048])
def test_bounds_as_the_header_states_them(L, n_ring):
    """MAX_TERMS is the largest power of two under the MAC bound at both ring sizes (14 / 13 products, restated in floats);
    a group's maxima may sum to T = 2048 / 1024 and not to T + 1, whatever the term count"""
    from peba1_amd import api
    assert Q.mac_terms(1024) == 14 and Q.mac_terms(2048) == 13
    assert Q.MAX_TERMS <= min(Q.mac_terms(1024), Q.mac_terms(2048)) < 2 * Q.MAX_TERMS
    T = K.max_coef(n_ring)
    assert T == {1024: 2048, 2048: 1024}[n_ring]
    bounds = L.tfhe_hip_test_public_sum_bounds
    for terms in range(1, Q.MAX_TERMS + 1):
        assert bounds(n_ring, terms, T) == 0 and bounds(n_ring, terms, T + 1) == 1, terms
        assert bounds(n_ring, terms, 0) == 0 and bounds(n_ring, terms, 1) == 0 and bounds(n_ring, terms, 2 ** 40) == 1
    assert api.last_error() == ""
    # the worst case the header names reaches N T 2^31 exactly, inside the CRT's exact range
    polys, ring, coef = Q.worst_group(n_ring, Q.MAX_TERMS)
    assert int(np.abs(polys).max(axis=1).sum()) == T
    assert max(abs(v) for v in coef) == coef[n_ring - 1] == n_ring * T * 2 ** 31 < K.CRT_EXACT_LIMIT
    for args in ((512, 1, 4), (n_ring, 0, 4), (n_ring, Q.MAX_TERMS + 1, 4), (n_ring, 2, -1), (4096, 1, 1)):
        assert bounds(*args) == -1 and "bad arguments" in api.last_error(), args
        L.tfhe_hip_clear_error()


def test_restatement_at_one_term_equals_public_commons_product():
    rng = np.random.default_rng(11)
    T = K.max_coef(N)
    polys = rng.integers(-T, T + 1, (3, N))
    ring = K.random_ring(rng, 3, N)
    ring[2] = K.I32_MIN
    for t in range(3):
        assert np.array_equal(Q.sum_product(polys[t:t + 1], ring[t:t + 1]), K.product(polys[t], ring[t]))
    # and a sum is the wrapped sum of its terms' products
    want = Q.wrap32(sum(K.product(polys[t], ring[t]).astype(np.int64) for t in range(3)))
    assert np.array_equal(Q.sum_product(polys, ring), want)
    assert np.array_equal(Q.sum_products(polys, ring[:1], 1), np.stack([K.product(polys[g], ring[0]) for g in range(3)]))
    assert np.array_equal(Q.sum_rows(polys, ring[:1], 1, 9, 128), K.rows(polys, ring[0], 9, 128))
    # the worst group against the closed form
    wp, wr, coef = Q.worst_group(N, Q.MAX_TERMS)
    want = K.to_i32(np.array([v % 2 ** 32 for v in coef], dtype=np.int64))
    assert np.array_equal(Q.sum_product(wp, wr), np.stack([want, want]))


def test_gallery_builders_round_trip():
    """long: entry i's bits come back from the group's polynomials term by term, and the summed product's coefficient e w is
    agree - disagree; masked: the two polynomials of a chunk are -den sigma n and (den - 2 num) n, and the summed product's
    coefficient e w is D"""
    from peba1_amd import identify
    rng = np.random.default_rng(5)
    w, terms = 256, 2
    S = N // w
    entries = rng.integers(0, 2, (S + 2, terms * w))
    q = identify.clear_gallery_polys_long(entries, w, N, terms)
    assert q.shape == (2 * terms, N) and q.dtype == np.int32
    for i, e in enumerate(entries):
        back = np.concatenate([q[(i // S) * terms + t, (i % S) * w:(i % S + 1) * w] for t in range(terms)])
        assert np.array_equal(back, e), i
    assert not q[terms:, 2 * w:].any()
    assert np.array_equal(identify.clear_gallery_polys_long(entries[:, :w], w, N, 1), identify.clear_gallery_polys(entries[:, :w], w, N))
    bits = rng.integers(0, 2, terms * w)
    probe = np.stack([identify.probe_layout(1 - 2 * bits[t * w:(t + 1) * w], N) for t in range(terms)])
    assert np.array_equal(probe[0], identify.hamming_probe_poly(bits[:w], N))
    for i in (0, S - 1, S):
        group = (i // S) * terms
        coef = sum(K.negacyclic_python(probe[t], q[group + t])[(i % S) * w] for t in range(terms))
        assert coef == int(entries[i].sum()) - 2 * int((entries[i] & bits).sum())
    for bad in (lambda: identify.clear_gallery_polys_long(entries, w, N, 3), lambda: identify.clear_gallery_polys_long(entries, 96, N, 2),
                lambda: identify.clear_gallery_polys_long(entries[:, :5], w, N, 2), lambda: identify.clear_gallery_polys_long(entries, w, N, 16)):
        with pytest.raises(ValueError):
            bad()
    # masked
    num, den, chunks = 8, 25, 2
    codes, masks = rng.integers(0, 2, (S + 1, chunks * w)), rng.integers(0, 2, (S + 1, chunks * w))
    mq = identify.masked_gallery_polys(codes, masks, w, N, num, den)
    assert mq.shape == (2 * 2 * chunks, N)
    for i in range(S + 1):
        for c in range(chunks):
            at = slice((i % S) * w, (i % S + 1) * w)
            g, n = codes[i, c * w:(c + 1) * w], masks[i, c * w:(c + 1) * w]
            assert np.array_equal(mq[(i // S) * 2 * chunks + 2 * c, at], -den * (1 - 2 * g) * n)
            assert np.array_equal(mq[(i // S) * 2 * chunks + 2 * c + 1, at], (den - 2 * num) * n)
    assert int(np.abs(mq).max(axis=1)[:2 * chunks].sum()) == chunks * (den + den - 2 * num) <= K.max_coef(N)
    b, m = rng.integers(0, 2, chunks * w), rng.integers(0, 2, chunks * w)
    mprobe = []
    for c in range(chunks):
        at = slice(c * w, (c + 1) * w)
        mprobe += [identify.probe_layout((1 - 2 * b[at]) * m[at], N), identify.probe_layout(m[at], N)]
    for i in (1, S):
        group = (i // S) * 2 * chunks
        coef = sum(K.negacyclic_python(mprobe[t], mq[group + t])[(i % S) * w] for t in range(2 * chunks))
        assert coef == identify.masked_decision(b, codes[i], m, masks[i], num, den)
    for bad in (lambda: identify.masked_gallery_polys(codes, masks[:, :w], w, N, num, den), lambda: identify.masked_gallery_polys(codes, masks, w, N, 25, 25),
                lambda: identify.masked_gallery_polys(codes[:, :w + 3], masks[:, :w + 3], w, N, num, den),
                lambda: identify.masked_gallery_polys(np.zeros((1, 5 * w)), np.zeros((1, 5 * w)), w, N, num, den)):
        with pytest.raises(ValueError):
            bad()


def test_masked_decision_identity_in_plain_integers():
    """200 random (b, g, m, n) of 64 bits: D <= 0 iff den disagree <= num valid, and D = 2 (den disagree - num valid)"""
    from peba1_amd import identify
    rng = np.random.default_rng(64)
    both = 0
    for trial in range(200):
        num, den = [(8, 25), (1, 3), (3, 10), (1, 2)][trial % 4]
        b, g = rng.integers(0, 2, 64), rng.integers(0, 2, 64)
        if trial % 5 == 0:
            g = b ^ (rng.random(64) < 0.3)                         # near the threshold
        m, n = (rng.random(64) < 0.8).astype(int), (rng.random(64) < 0.7).astype(int)
        valid, disagree = Q.masked_counts(b, g, m, n)
        D = identify.masked_decision(b, g, m, n, num, den)
        assert D == 2 * (den * disagree - num * valid)
        assert (D <= 0) == (den * disagree <= num * valid), (trial, D, valid, disagree)
        both |= 1 << (D <= 0)
    assert both == 3
    assert identify.masked_decision([0], [1], [1], [0], 8, 25) == 0      # nothing valid: 0 / 0 counts as a match (D = 0)


def test_decision_band_and_amplitudes():
    from peba1_amd import api, identify
    pp = api.ParameterSet(128)
    assert identify.clear_decision_band(pp, identify.inner_delta(128)) == identify.inner_decision_band(pp, 128) == 12
    assert identify.clear_decision_band(pp, identify.inner_delta(16)) == identify.inner_decision_band(pp, 16)
    sigma = identify.inner_decision_sigma(pp)
    for delta in (identify.inner_delta(2048), identify.masked_delta(25, 2048)):
        g = identify.clear_decision_band(pp, delta)
        assert (g - 0.5) * delta / 2.0 ** 32 >= 6 * sigma > (g - 1.5) * delta / 2.0 ** 32
    # the figures the header states, computed
    assert identify.inner_delta(2048) == 1 << 19 and identify.clear_decision_band(pp, 1 << 19) == 184
    assert identify.masked_delta(25, 2048) == 1 << 14 and identify.clear_decision_band(pp, 1 << 14) == 5869
    assert -(-5869 // 50) == 118
    # |D| Delta stays below 1/2: D runs from -2 num L to 2 (den - num) L
    for num, den, length in ((8, 25, 2048), (1, 3, 64), (1, 2, 1024)):
        delta = identify.masked_delta(den, length)
        assert 2 * max(num, den - num) * length * delta + delta // 2 < 2 ** 31
    assert abs(identify.masked_product_sigma(8, 25, 2048, 2.0 ** -25) - 3.6e-5) < 1e-6
    assert abs(identify.masked_weight_gain(8, 25) - 26.6) < 0.05 and abs(26.57 * 2.8e-3 - 7.4e-2) < 1e-3
    with pytest.raises(ValueError):
        identify.clear_decision_band(pp, 0)


def test_refusals_leave_outputs_and_slots_untouched(small, L):
    """every refusal of the new entries that is decided before the device is looked at (this test runs without one): -1, a
    message, results with their values and without slots, raw outputs untouched"""
    from peba1_amd import api
    pp, ks = small
    T = K.max_coef(N)
    cts = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    held = cts.words().copy()
    other_pp = api.ParameterSet(custom=K.custom_tuple(N_LWE + 2))
    other_cts = api.CiphertextArray(other_pp, 4)
    pp2048 = api.ParameterSet(custom=K.custom_tuple(N_LWE, N=2048, gadget=(3, 6)))
    ring = K.random_ring(np.random.default_rng(4), 8, N).reshape(-1)
    polys = np.ones((6, N), dtype=np.int32)
    polys[4, 7], polys[5, 9] = T, -1                              # group 2 of terms = 2: maxima T + 1; of terms = 3, group 1
    g = api.PublicGallery(pp, polys)
    g2048 = api.PublicGallery(pp2048, np.ones((2, 2048), dtype=np.int32))
    dead = api.PublicGallery(pp, np.ones((2, N), dtype=np.int32))
    dead_ptr = dead.ptr
    dead.close()
    raw_out = np.full((3, 2 * N), 7, dtype=np.int32)

    def refused(rc, needle):
        assert rc == -1 and needle in api.last_error(), (rc, needle, api.last_error())
        assert [cts.at(j).contents.slot for j in range(4)] == [-1] * 4 and np.array_equal(cts.words(), held)
        assert (raw_out == 7).all()
        L.tfhe_hip_clear_error()

    for entry in (L.tfhe_hip_ring_inner_public_sum, L.tfhe_hip_ring_inner_public_sum_device):
        src = _i32p(ring) if entry is L.tfhe_hip_ring_inner_public_sum else C.c_void_p(ring.ctypes.data)
        refused(entry(g.ptr, ks.cloud, None, 2, 2, N, cts.ptr), "null ring words or result")
        refused(entry(g.ptr, ks.cloud, src, 2, 2, N, None), "null ring words or result")
        refused(entry(g.ptr, None, src, 2, 2, N, cts.ptr), "null cloud key")
        refused(entry(None, ks.cloud, src, 2, 2, N, cts.ptr), "null or deleted gallery")
        refused(entry(dead_ptr, ks.cloud, src, 2, 2, N, cts.ptr), "null or deleted gallery")
        refused(entry(g2048.ptr, ks.cloud, src, 2, 1, N, cts.ptr), "different rings")
        for terms in (0, -1, Q.MAX_TERMS + 1, 16):
            refused(entry(g.ptr, ks.cloud, src, terms, 2, N, cts.ptr), "terms must be in 1..8")
        for terms in (4, 5):
            refused(entry(g.ptr, ks.cloud, src, terms, 1, N, cts.ptr), "6 polynomials are not a multiple of terms = %d" % terms)
        for width in (0, 3, 96, 2 * N, -4):
            refused(entry(g.ptr, ks.cloud, src, 2, 2, width, cts.ptr), "width must be a power of two in 1..1024")
        refused(entry(g.ptr, ks.cloud, src, 2, 0, N, cts.ptr), "M must be at least 1")
        refused(entry(g.ptr, ks.cloud, src, 2, 4, N, cts.ptr), "need more than the 3 groups of the gallery")
        refused(entry(g.ptr, ks.cloud, src, 3, 5, 512, cts.ptr), "need more than the 2 groups of the gallery")
        refused(entry(g.ptr, ks.cloud, src, 2, 3, N, cts.ptr), "group 2 (polynomials 4..5): its terms' largest coefficients sum to %d, past %d" % (T + 1, T))
        refused(entry(g.ptr, ks.cloud, src, 3, 2, N, cts.ptr), "group 1 (polynomials 3..5)")
        refused(entry(g.ptr, ks.cloud, src, 2, 2, N, cts.at(3)), "past the end of the result array")
        refused(entry(g.ptr, ks.cloud, src, 2, 2, N, other_cts.ptr), "LWE dimension")
    refused(L.tfhe_hip_ring_inner_public_sum_device(g.ptr, ks.cloud, C.c_void_p(ring.ctypes.data + 4), 2, 2, N, cts.ptr), "16-byte aligned")
    out = _i32p(raw_out)
    for entry in (L.tfhe_hip_ring_mul_public_sum, L.tfhe_hip_kernel_ring_public_sum_product, L.tfhe_hip_ring_mul_public_sum_device):
        dev = entry is L.tfhe_hip_ring_mul_public_sum_device
        src, dst = (C.c_void_p(ring.ctypes.data), C.c_void_p(raw_out.ctypes.data)) if dev else (_i32p(ring), out)
        refused(entry(None, 0, 2, 1, src, dst), "null or deleted gallery")
        refused(entry(dead_ptr, 0, 2, 1, src, dst), "null or deleted gallery")
        refused(entry(g.ptr, 0, 2, 1, None, dst), "null ring words or destination")
        refused(entry(g.ptr, 0, 2, 1, src, None), "null ring words or destination")
        refused(entry(g.ptr, 0, 0, 1, src, dst), "terms must be in 1..8")
        refused(entry(g.ptr, 0, 9, 1, src, dst), "terms must be in 1..8")
        refused(entry(g.ptr, 0, 4, 1, src, dst), "not a multiple of terms = 4")
        refused(entry(g.ptr, 0, 2, 0, src, dst), "ngroups must be in 1..65536")
        refused(entry(g.ptr, 0, 2, 65537, src, dst), "ngroups must be in 1..65536")
        refused(entry(g.ptr, -1, 2, 1, src, dst), "must lie in 0..5")
        refused(entry(g.ptr, 2, 2, 3, src, dst), "must lie in 0..5")
        refused(entry(g.ptr, 6, 1, 1, src, dst), "must lie in 0..5")
        refused(entry(g.ptr, 0, 2, 3, src, dst), "group 2 (polynomials 4..5)")
        refused(entry(g.ptr, 4, 2, 1, src, dst), "group 0 (polynomials 4..5)")
    mul_dev = L.tfhe_hip_ring_mul_public_sum_device
    refused(mul_dev(g.ptr, 0, 2, 1, C.c_void_p(ring.ctypes.data + 4), C.c_void_p(raw_out.ctypes.data)), "16-byte aligned")
    refused(mul_dev(g.ptr, 0, 2, 1, C.c_void_p(ring.ctypes.data), C.c_void_p(raw_out.ctypes.data + 8)), "16-byte aligned")
    refused(mul_dev(g.ptr, 0, 2, 1, C.c_void_p(ring.ctypes.data), C.c_void_p(ring.ctypes.data + 8 * N)), "overlaps the ring words")
    refused(mul_dev(g.ptr, 0, 1, 2, C.c_void_p(ring.ctypes.data + 8 * N), C.c_void_p(ring.ctypes.data)), "overlaps the ring words")
    rows = L.tfhe_hip_kernel_ring_public_sum_rows
    refused(rows(None, _i32p(ring), 2, 2, N, out), "null or deleted gallery")
    refused(rows(g.ptr, None, 2, 2, N, out), "null argument")
    refused(rows(g.ptr, _i32p(ring), 2, 2, N, None), "null argument")
    refused(rows(g.ptr, _i32p(ring), 0, 2, N, out), "terms must be in 1..8")
    refused(rows(g.ptr, _i32p(ring), 4, 1, N, out), "not a multiple of terms = 4")
    refused(rows(g.ptr, _i32p(ring), 2, 2, 48, out), "width must be a power of two")
    refused(rows(g.ptr, _i32p(ring), 2, 0, 128, out), "M must be at least 1")
    refused(rows(g.ptr, _i32p(ring), 2, 25, 128, out), "need more than the 3 groups of the gallery")
    refused(rows(g.ptr, _i32p(ring), 2, 17, 128, out), "group 2 (polynomials 4..5)")
    # the wrappers check the probe's sample count before the library is called
    with pytest.raises(ValueError):
        api.ring_mul_public_sum(g, ring.reshape(8, 2 * N), 2)
    with pytest.raises(ValueError):
        api.ring_inner_public_sum(g, ring.reshape(8, 2 * N)[:3], 2, 2, N, ks, cts)
    for o in (g, g2048, cts, other_cts):
        o.close()
