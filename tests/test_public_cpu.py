"""A ring sample times public polynomials without a GPU: the definitions of include/tfhe_hip.h restated in numpy and Python
integers (tests/public_common.py) -- coefficient e w of gallery polynomial times probe polynomial is the entry's inner
product and no other entry enters it, the product of a real ring encryption decrypts to q mu --, the CRT bound against
Python big integers, every refusal of the new constructor and entries, and the computed variance against the header's
figures, on host-only keysets."""
import ctypes as C

import numpy as np
import pytest

import public_common as K

N = 1024
N_LWE = 11
BK_STDEV = K.STDEVS[1]


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def small():
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, 0x9B1C, device=False)
    yield pp, ks
    ks.close()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.mark.parametrize("w", [1, 2, 128, N])
def test_probe_layout_identity_against_plain_inner_products(w):
    """gallery polynomial q (entries of w bits in the lookup's layout) times probe polynomial p = sum_i s_i X^(-i), term by
    term in Python integers: coefficient e w is sum_i s_i q[e w + i] for every entry e; zeroing one entry changes that
    entry's coefficient among the coefficients e w and no other.  The argument is symmetric: either factor first."""
    from peba1_amd import identify
    rng = np.random.default_rng(700 + w)
    per = N // w
    s = 1 - 2 * rng.integers(0, 2, w)
    entries = rng.integers(0, 2, (per, w))
    entries[:, 0] = 1                                            # (every entry has weight: zeroing it must show)
    q = identify.clear_gallery_polys(entries, w, N)
    assert q.shape == (1, N) and np.array_equal(q[0], entries.reshape(-1))
    p = K.probe_poly(s, N)
    assert np.array_equal(p, identify.hamming_probe_poly((1 - s) // 2, N))
    pq = K.negacyclic_python(p, q[0])
    for e in range(per):
        assert pq[e * w] == sum(int(s[i]) * int(q[0][e * w + i]) for i in range(w)), e
    if w <= 128:
        assert pq == K.negacyclic_python(q[0], p)
    z = per // 2
    q0 = q[0].copy()
    q0[z * w:(z + 1) * w] = 0
    pq0 = K.negacyclic_python(p, q0)
    assert [e for e in range(per) if pq0[e * w] != pq[e * w]] == [z] and pq0[z * w] == 0


def test_restatements_agree_and_monomials_follow_the_lookups_convention():
    """the dense int64 form equals the term-by-term Python integers mod 2^32 on full-range words; q = 1 is the identity;
    q = X^r is the lookup's X^(-r) with the sign of the exponent flipped: X^r (X^(-r) c) = c"""
    rng = np.random.default_rng(3)
    T = K.max_coef(N)
    q = rng.integers(-T, T + 1, N)
    c = K.random_ring(rng, 1, N)[0]
    got = K.product(q, c)
    for u in range(2):
        want = K.negacyclic_python(q, c[u])
        assert np.array_equal(got[u], K.to_i32(np.array([v % 2 ** 32 for v in want], dtype=np.int64)))
    one = np.zeros(N, dtype=np.int64)
    one[0] = 1
    assert np.array_equal(K.product(one, c), c)
    for r in (1, 129, N - 1):
        x = np.zeros(N, dtype=np.int64)
        x[r] = 1
        assert np.array_equal(K.product(x, c), K.monomial(c, r))
        assert np.array_equal(K.monomial(K.inverse_monomial(c, r), r), c)


@pytest.mark.parametrize("n_ring", [1024, 2048])
def test_bound_function_accepts_T_and_refuses_2T(L, n_ring):
    """T = 2^11 at N = 1024 and 2^10 at N = 2048 by Python big integers; the stated worst case -- all q[j] = -T against
    words 0x80000000 -- reaches N T 2^31 exactly, at coefficient N - 1, below CRT_EXACT_LIMIT; with 2 T it is past it"""
    from peba1_amd import api
    T = K.max_coef(n_ring)
    assert T == {1024: 2 ** 11, 2048: 2 ** 10}[n_ring] == api.public_max_coef(n_ring)
    coef, most = K.worst_case(n_ring)
    assert most == coef[n_ring - 1] == n_ring * T * 2 ** 31 < K.CRT_EXACT_LIMIT <= n_ring * 2 * T * 2 ** 31
    assert L.tfhe_hip_test_public_bounds(n_ring, T) == 0 and L.tfhe_hip_test_public_bounds(n_ring, 2 * T) == 1
    # the function is the inequality itself (T is its largest POWER OF TWO): exact at the last integer that passes
    last = (K.CRT_EXACT_LIMIT - 1) // (n_ring * 2 ** 31)
    assert T <= last < 2 * T and n_ring * last * 2 ** 31 < K.CRT_EXACT_LIMIT <= n_ring * (last + 1) * 2 ** 31
    assert L.tfhe_hip_test_public_bounds(n_ring, last) == 0 and L.tfhe_hip_test_public_bounds(n_ring, last + 1) == 1
    assert L.tfhe_hip_test_public_bounds(n_ring, 1) == 0 and L.tfhe_hip_test_public_bounds(n_ring, 2 ** 31 - 1) == 1
    assert api.last_error() == ""
    for args in ((512, 4), (n_ring, 0), (n_ring, -1), (4096, 1)):
        assert L.tfhe_hip_test_public_bounds(*args) == -1 and "bad arguments" in api.last_error()
        L.tfhe_hip_clear_error()
    # the forward bound the kernel relies on: reduced words (|x| < P) stay inside int32, unreduced ones (2^31) do not
    logn = 10 if n_ring == 1024 else 11
    assert K.forward_bound(logn, float(K.P1)) < 8.2 and K.forward_bound(logn, float(K.P1)) * K.P1 < 2 ** 31
    assert K.forward_bound(logn, 2.0 ** 31) * K.P1 > 2 ** 31
    assert K.forward_bound(logn, float(K.P1)) * K.P1 / 2.0 ** 32 + 0.5 < 4.0


def test_the_product_of_a_ring_encryption_decrypts_to_q_mu(small):
    """w = 128 at N = 1024: a seeded and a seed-compressed probe sample (hamming_probe_ring) times a 0/1 gallery polynomial
    through the restatement: every coefficient of the phase is that of q mu within 7 sigma of the header's variance
    (|q|_2^2 bk_stdev^2 and nothing else), and the extracted row of entry e has the phase of coefficient e w"""
    from peba1_amd import api, identify
    pp, ks = small
    w, per = 128, N // 128
    rng = np.random.default_rng(21)
    bits = rng.integers(0, 2, w)
    entries = rng.integers(0, 2, (per, w))
    q = identify.clear_gallery_polys(entries, w, N)
    delta = identify.inner_delta(w)
    mu = K.probe_poly(1 - 2 * bits, N) * delta
    want = K.negacyclic_python(q[0], mu)
    for e in range(per):
        assert want[e * w] == (int(entries[e].sum()) - 2 * int((entries[e] & bits).sum())) * delta
    sigma = K.variance(float((q[0] ** 2).sum()), BK_STDEV ** 2) ** 0.5
    plain, addend = identify.hamming_probe_ring(bits, w, ks, seed=0x31)
    packed, addend2 = identify.hamming_probe_ring(bits, w, ks, compressed=True, seed=0x32)
    assert plain.shape == (2 * N,) and packed.shape == (10 + N,)
    assert np.array_equal(plain, api.ring_encrypt(mu, ks, seed=0x31))
    for words in (plain.reshape(2, N), api.ring_expand(packed, N).reshape(2, N)):
        out = K.product(q[0], words)
        ph = K.ring_phases(out, ks.tlwe_key()).astype(np.int64)
        err = (ph - np.array([v % 2 ** 32 for v in want], dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31
        assert np.abs(err).max() < 7 * sigma * 2 ** 32, (np.abs(err).max() / 2.0 ** 32, sigma)
        rows = K.rows(q, words, per, w)
        assert np.array_equal(K.U.extracted_phases(rows, ks.tlwe_key()), K.to_i32(ph[np.arange(per) * w]))
    with pytest.raises(ValueError):
        identify.hamming_probe_ring([0, 1, 1], 128, ks)
    with pytest.raises(ValueError):
        identify.clear_gallery_polys([[0, 1, 1]], 128, N)
    for o in (addend, addend2):
        o.close()


def test_computed_variance_equals_the_headers_figures():
    """|q|_2^2 <= N for a 0/1 polynomial: P128 2^-40 = 9.1e-13 (sigma 9.5e-7), the l = 2 set 5.3e-14 (2.3e-7), P2048 2^-39 =
    1.8e-12 (1.3e-6); about 170 times below the TGSW route's 1.6e-4 at P128"""
    v128, vl2, v2048 = (K.variance(1024.0, K.BK_STDEVS["P128"] ** 2), K.variance(1024.0, K.BK_STDEVS["l2"] ** 2),
                        K.variance(2048.0, K.BK_STDEVS["P2048"] ** 2))
    assert v128 == 2.0 ** -40 and abs(v128 - 9.1e-13) < 1e-14 and abs(v128 ** 0.5 - 9.5e-7) < 1e-8
    assert abs(vl2 - 5.3e-14) < 1e-15 and abs(vl2 ** 0.5 - 2.3e-7) < 1e-8
    assert v2048 == 2.0 ** -39 and abs(v2048 - 1.8e-12) < 2e-14 and abs(v2048 ** 0.5 - 1.3e-6) < 5e-8
    assert 160 < 1.6e-4 / v128 ** 0.5 < 180
    assert abs(32 * K.BK_STDEVS["P128"] - 9.5e-7) < 1e-8         # "at most 32 bk_stdev"


def test_constructor_refusals_have_no_effect(small, L):
    from peba1_amd import api
    pp, ks = small
    T = K.max_coef(N)
    polys = np.zeros((2, N), dtype=np.int32)
    polys[1, 5] = T
    polys[0, 9] = -T
    g = api.PublicGallery(pp, polys)                             # +-T itself is taken
    assert L.tfhe_hip_public_gallery_polys(g.ptr) == 2 and api.last_error() == ""
    g.close()

    def refused(ptr, needle):
        assert not ptr and needle in api.last_error(), (needle, api.last_error())
        L.tfhe_hip_clear_error()

    new = L.tfhe_hip_new_public_gallery
    refused(new(None, _i32p(polys), 2), "null parameter set")
    refused(new(pp.ptr, None, 2), "null polynomials")
    refused(new(pp.ptr, _i32p(polys), 0), "R must be in 1..1048576")
    refused(new(pp.ptr, _i32p(polys), -3), "R must be in 1..1048576")
    refused(new(pp.ptr, _i32p(polys), 2 ** 20 + 1), "R must be in 1..1048576")
    bad = polys.copy()
    bad[1, 7] = T + 1
    bad[1, 8] = -5 * T
    refused(new(pp.ptr, _i32p(bad), 2), "coefficient %d at index %d (polynomial 1, coefficient 7) is outside -%d..%d" % (T + 1, N + 7, T, T))
    first = L.tfhe_hip_new_public_gallery(pp.ptr, _i32p(bad), 1)  # (the first polynomial alone is fine)
    assert first and L.tfhe_hip_public_gallery_polys(first) == 1
    L.tfhe_hip_delete_public_gallery(first)
    bad[0, 0] = -T - 1
    refused(new(pp.ptr, _i32p(bad), 2), "coefficient %d at index 0 " % (-T - 1))
    # N = 2048 has the smaller T; another ring or k is refused outright
    pp2048 = api.ParameterSet(custom=K.custom_tuple(N_LWE, N=2048, gadget=(3, 6)))
    wide = np.zeros((1, 2048), dtype=np.int32)
    wide[0, 2047] = 1024
    api.PublicGallery(pp2048, wide).close()
    wide[0, 2047] = 1025
    refused(new(pp2048.ptr, _i32p(wide), 1), "at index 2047 (polynomial 0, coefficient 2047) is outside -1024..1024")
    for tup in (K.custom_tuple(N_LWE, N=512), (N_LWE, 1024, 2) + K.custom_tuple(N_LWE)[3:], K.custom_tuple(N_LWE, N=4096)):
        refused(new(api.ParameterSet(custom=tup).ptr, _i32p(wide), 1), "N = 1024 or 2048 and k = 1")
    assert L.tfhe_hip_public_gallery_polys(None) == -1 and "null or deleted gallery" in api.last_error()
    L.tfhe_hip_clear_error()
    L.tfhe_hip_delete_public_gallery(None)
    assert api.last_error() == ""
    with pytest.raises(ValueError, match="public gallery rejected"):
        api.PublicGallery(pp, bad)
    L.tfhe_hip_clear_error()


def test_entry_refusals_leave_outputs_untouched(small, L):
    """every refusal of tfhe_hip_ring_mul_public, tfhe_hip_ring_inner_public and the two raw entries that is decided before
    the device is looked at (this test runs without one): -1, a message, results with their values and without slots, raw
    outputs untouched"""
    from peba1_amd import api
    pp, ks = small
    cts = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    held = cts.words().copy()
    other_pp = api.ParameterSet(custom=K.custom_tuple(N_LWE + 2))
    other_cts = api.CiphertextArray(other_pp, 4)
    pp2048 = api.ParameterSet(custom=K.custom_tuple(N_LWE, N=2048, gadget=(3, 6)))
    ring = K.random_ring(np.random.default_rng(4), 3, N).reshape(-1)
    g = api.PublicGallery(pp, np.ones((2, N), dtype=np.int32))
    g2048 = api.PublicGallery(pp2048, np.ones((1, 2048), dtype=np.int32))
    dead = api.PublicGallery(pp, np.ones((1, N), dtype=np.int32))
    dead_ptr = dead.ptr
    dead.close()
    raw_out = np.full((3, 2 * N), 7, dtype=np.int32)

    def refused(rc, needle):
        assert rc == -1 and needle in api.last_error(), (rc, needle, api.last_error())
        assert [cts.at(j).contents.slot for j in range(4)] == [-1] * 4 and np.array_equal(cts.words(), held)
        assert (raw_out == 7).all()
        L.tfhe_hip_clear_error()

    for entry in (L.tfhe_hip_ring_inner_public, L.tfhe_hip_ring_inner_public_device):
        src = _i32p(ring) if entry is L.tfhe_hip_ring_inner_public else C.c_void_p(ring.ctypes.data)
        refused(entry(g.ptr, ks.cloud, None, 2, N, cts.ptr), "null ring words or result")
        refused(entry(g.ptr, ks.cloud, src, 2, N, None), "null ring words or result")
        refused(entry(g.ptr, None, src, 2, N, cts.ptr), "null cloud key")
        refused(entry(None, ks.cloud, src, 2, N, cts.ptr), "null or deleted gallery")
        refused(entry(dead_ptr, ks.cloud, src, 2, N, cts.ptr), "null or deleted gallery")
        refused(entry(g2048.ptr, ks.cloud, src, 2, N, cts.ptr), "different rings")
        for width in (0, 3, 96, 2 * N, -4):
            refused(entry(g.ptr, ks.cloud, src, 2, width, cts.ptr), "width must be a power of two in 1..1024")
        refused(entry(g.ptr, ks.cloud, src, 0, N, cts.ptr), "M must be at least 1")
        refused(entry(g.ptr, ks.cloud, src, 3, N, cts.ptr), "need more than the 2 polynomials of the gallery")
        refused(entry(g.ptr, ks.cloud, src, 5, 512, cts.ptr), "need more than the 2 polynomials of the gallery")
        refused(entry(g.ptr, ks.cloud, src, 2, N, cts.at(3)), "past the end of the result array")
        refused(entry(g.ptr, ks.cloud, src, 2, N, other_cts.ptr), "LWE dimension")
    refused(L.tfhe_hip_ring_inner_public_device(g.ptr, ks.cloud, C.c_void_p(ring.ctypes.data + 4), 2, N, cts.ptr), "16-byte aligned")
    out = _i32p(raw_out)
    for entry in (L.tfhe_hip_ring_mul_public, L.tfhe_hip_kernel_ring_public_product, L.tfhe_hip_ring_mul_public_device):
        dev = entry is L.tfhe_hip_ring_mul_public_device
        src, dst = (C.c_void_p(ring.ctypes.data), C.c_void_p(raw_out.ctypes.data)) if dev else (_i32p(ring), out)
        refused(entry(None, 0, 1, src, 1, dst), "null or deleted gallery")
        refused(entry(dead_ptr, 0, 1, src, 1, dst), "null or deleted gallery")
        refused(entry(g.ptr, 0, 1, None, 1, dst), "null ring words or destination")
        refused(entry(g.ptr, 0, 1, src, 1, None), "null ring words or destination")
        refused(entry(g.ptr, 0, 0, src, 1, dst), "npolys must be in 1..65536")
        refused(entry(g.ptr, 0, 65537, src, 1, dst), "npolys must be in 1..65536")
        refused(entry(g.ptr, 0, 1, src, 0, dst), "count must be in 1..65536")
        refused(entry(g.ptr, -1, 1, src, 1, dst), "must lie in 0..1")
        refused(entry(g.ptr, 1, 2, src, 2, dst), "must lie in 0..1")
        refused(entry(g.ptr, 2, 1, src, 1, dst), "must lie in 0..1")
        refused(entry(g.ptr, 0, 2, src, 3, dst), "npolys and count must be equal unless one of them is 1")
    mul_dev = L.tfhe_hip_ring_mul_public_device
    refused(mul_dev(g.ptr, 0, 1, C.c_void_p(ring.ctypes.data + 4), 1, C.c_void_p(raw_out.ctypes.data)), "16-byte aligned")
    refused(mul_dev(g.ptr, 0, 1, C.c_void_p(ring.ctypes.data), 1, C.c_void_p(raw_out.ctypes.data + 8)), "16-byte aligned")
    refused(mul_dev(g.ptr, 0, 2, C.c_void_p(ring.ctypes.data), 1, C.c_void_p(ring.ctypes.data + 4 * N)), "overlaps the ring words")
    refused(mul_dev(g.ptr, 0, 1, C.c_void_p(ring.ctypes.data), 2, C.c_void_p(ring.ctypes.data)), "overlaps the ring words")
    rows = L.tfhe_hip_kernel_ring_public_rows
    refused(rows(None, _i32p(ring), 2, N, out), "null or deleted gallery")
    refused(rows(g.ptr, None, 2, N, out), "null argument")
    refused(rows(g.ptr, _i32p(ring), 2, N, None), "null argument")
    refused(rows(g.ptr, _i32p(ring), 2, 48, out), "width must be a power of two")
    refused(rows(g.ptr, _i32p(ring), 0, 128, out), "M must be at least 1")
    refused(rows(g.ptr, _i32p(ring), 17, 128, out), "need more than the 2 polynomials of the gallery")
    with pytest.raises(ValueError):
        api.ring_mul_public(g, ring.reshape(3, 2 * N))
    for o in (g, g2048, cts, other_cts):
        o.close()
