"""The packed lookup without a GPU: the monomial multiple of the numpy restatement (tests/lookup_common.py) against an
explicit negacyclic product in Python integers, the restated lookup at decrypt level under seeded host keys for every
index, its w = N case against the select's tree word for word, and every refusal of the server-side entries -- all of them
checked before the device is looked at; nothing here launches."""
import ctypes as C

import numpy as np
import pytest

import lookup_common as K
import select_common as S

SEED = 0x10C0
N_LWE = 10                    # the LWE side plays no part: a short key is made quickly


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def host_keys():
    """a host-only keyset of the P128 ring and gadget (N = 1,024, l = 3, Bgbit = 7, bk_stdev = 2^-25)"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=S.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, SEED, device=False)
    yield pp, ks
    ks.close()


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def monomial_product(poly, r):
    """poly(X) * X^(-r) in Z[X]/(X^N + 1) mod 2^32 in Python integers: X^(-r) = -X^(N - r), multiplied out term by term"""
    N = len(poly)
    out = [0] * N
    for i, a in enumerate(poly):
        e = i + (N - r)                                    # a X^i * (-X^(N-r)) = -a X^e, and X^N = -1
        sign = -1
        while e >= N:
            e, sign = e - N, -sign
        out[e] = (out[e] + sign * int(a)) % 2 ** 32
    return out


def test_rotate_ref_is_the_negacyclic_product_by_the_monomial():
    N = 64
    c = S.random_ring(np.random.default_rng(1), 1, N)[0]
    for r in (1, N - 1, N // 2):
        got = K.rotate_ref(c, r).astype(np.int64) % 2 ** 32
        for u in range(2):
            assert list(got[u]) == monomial_product(c[u], r), (r, u)
        # X^(-r) X^(-(N-r)) = X^(-N) = -1
        back = K.rotate_ref(K.rotate_ref(c, r), N - r)
        assert np.array_equal(back, S.to_i32(-c.astype(np.int64))), r
    assert np.array_equal(K.rotate_ref(c, 0), c)
    # the extreme words wrap: -0x80000000 = 0x80000000
    e = np.full((2, N), S.I32_MIN, dtype=np.int32)
    assert np.array_equal(K.rotate_ref(e, 3), e)


@pytest.mark.parametrize("r", [1, 63, 64, 65, 128, 512, 1023])
def test_a_sample_is_formed_whose_rotated_difference_is_constant(r):
    """the operands the GPU test builds for the extreme digits: X^(-r) d0 - d0 = E on every coefficient"""
    N, l, Bgbit = 1024, 3, 7
    for which in ("min", "max"):
        E = S.extreme_difference(l, Bgbit, which)
        d0 = S.to_i32(K.sample_with_rotated_difference(N, r, E))
        diff = (K.rotate_ref(d0, r).astype(np.int64) - d0) % 2 ** 32
        assert (diff == E).all(), (r, which)
        digit = -2 ** (Bgbit - 1) if which == "min" else 2 ** (Bgbit - 1) - 1
        assert (S.decompose(S.to_i32(diff), l, Bgbit) == digit).all()


CASES = [(1024, 3), (128, 8), (128, 20), (1, 5), (512, 3)]          # (w, M)


def bits_of(index, d):
    return [(index >> j) & 1 for j in range(d)]


@pytest.mark.parametrize("w,M", CASES)
def test_numpy_lookup_decrypts_to_the_indexed_entry(host_keys, w, M, capsys):
    """every index; entries are bits at +-1/8, the margin 1/8.  The selector has the fewest bits that hold: d = s + the bits
    of the sample index.  The largest |phase error| is printed beside the computed bound of d CMUX terms."""
    from peba1_amd import api, identify
    pp, ks = host_keys
    N = pp.N
    Sn = N // w
    s, R = K.log2_exact(Sn), -(-M // Sn)
    d = s + max(R - 1, 0).bit_length()
    entries = np.random.default_rng(w + M).integers(0, 2, (M, w))
    gallery = identify.pack_gallery(entries, w, ks, seed=0x6A00 + w).reshape(R, 2, N)
    sigma = (S.STDEVS[1] ** 2 + d * S.cmux_variance(N, pp.l, pp.Bgbit, S.STDEVS[1])) ** 0.5
    worst = 0.0
    for index in range(M):
        sel = api.tgsw_encrypt_bits(bits_of(index, d), ks, seed=0x700 + index) if d else np.zeros((0, 2 * pp.l, 2, N), dtype=np.int32)
        out = K.lookup_ref(sel, gallery, M, w, pp.l, pp.Bgbit)
        assert list(api.packed_decrypt(out, w, ks)) == list(entries[index]), (w, M, index)
        ph = api.packed_phases(out, ks).astype(np.float64)[:w] / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(entries[index] == 1, 0.125, -0.125)).max())
    with capsys.disabled():
        print("\nnumpy lookup w = %d, M = %d, d = %d (%d rotations): largest |phase error| %.3e, computed sigma bound %.3e"
              % (w, M, d, s, worst, sigma))
    assert worst < 1.0 / 8


def test_lookup_of_whole_samples_is_the_tree_word_for_word():
    N, l, Bgbit = 256, 3, 7
    rng = np.random.default_rng(9)
    words = S.random_ring(rng, 3 * 2 * l, N).reshape(3, 2 * l, 2, N)
    gallery = S.random_ring(rng, 5, N)
    for M, d in ((1, 0), (3, 2), (5, 3)):
        assert np.array_equal(K.lookup_ref(words[:d], gallery[:M], M, N, l, Bgbit), S.tree(words[:d], gallery[:M], l, Bgbit)), (M, d)


def test_an_index_in_a_sample_past_R_gives_a_phase_near_zero(host_keys):
    from peba1_amd import api, identify
    pp, ks = host_keys
    entries = np.random.default_rng(4).integers(0, 2, (20, 128))            # R = 3 of the 4 samples d = 5 can name
    gallery = identify.pack_gallery(entries, 128, ks, seed=0x6B00).reshape(3, 2, pp.N)
    sel = api.tgsw_encrypt_bits(bits_of(26, 5), ks, seed=0x7F0)             # entry 2 of sample 3
    ph = api.packed_phases(K.lookup_ref(sel, gallery, 20, 128, pp.l, pp.Bgbit), ks).astype(np.float64) / 2.0 ** 32
    assert np.abs(ph).max() < 1.0 / 64


def test_pack_gallery_and_ring_trivial(host_keys):
    from peba1_amd import api, identify
    pp, ks = host_keys
    N = pp.N
    entries = np.random.default_rng(5).integers(0, 2, (11, 128))
    g = identify.pack_gallery(entries, 128, ks, seed=3)
    assert g.shape == (2, 2 * N) and api.lookup_samples(pp, 11, 128) == 2
    assert list(api.packed_decrypt(g[0], N, ks)) == list(entries[:8].reshape(-1))
    assert list(api.packed_decrypt(g[1], 3 * 128, ks)) == list(entries[8:].reshape(-1))
    assert np.abs(api.packed_phases(g[1], ks)[3 * 128:].astype(np.float64)).max() < 2.0 ** 32 / 64      # zero behind the entries
    with pytest.raises(ValueError, match="every entry carries 128 bits"):
        identify.pack_gallery([[1, 0, 1]], 128, ks)
    with pytest.raises(ValueError, match="power of two"):
        identify.pack_gallery(entries, 96, ks)
    gc = identify.pack_gallery(entries, 128, ks, compressed=True)
    assert gc.shape == (2, 10 + N)
    assert list(api.packed_decrypt(api.ring_expand(gc, N)[1], 3 * 128, ks)) == list(entries[8:].reshape(-1))
    # the noiseless sample: a zero mask, the values as the body -- it decrypts to them under any key
    t = api.ring_trivial(pp, [2 ** 29, -2 ** 29, 7])
    assert t.shape == (2 * N,) and not t[:N].any() and list(t[N:N + 4]) == [2 ** 29, -2 ** 29, 7, 0]
    assert list(api.packed_phases(t, ks)[:3]) == [2 ** 29, -2 ** 29, 7]
    with pytest.raises(ValueError):
        api.ring_trivial(pp, np.zeros(N + 1))


# ---- refusals: nothing is touched, the error is set, no device is looked at ----
def test_refusals_have_no_effect(L, host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    N = pp.N
    words = api.tgsw_encrypt_bits([1, 0, 1], ks, seed=1)
    ring = S.random_ring(np.random.default_rng(6), 4, N)
    out = np.full(2 * N, 0x5A5A5A5A, dtype=np.int32)
    vp = lambda a, off=0: C.c_void_p(a.ctypes.data + off)                       # noqa: E731

    def refused(rc, needle):
        assert rc == -1 and needle in api.last_error(), (rc, api.last_error())
        L.tfhe_hip_clear_error()

    sel = api.Selector(pp, words)                                   # d = 3
    # a null pointer, a deleted (here: absent) selector
    refused(L.tfhe_hip_ring_lookup(None, i32p(ring), 4, N, i32p(out)), "null or deleted selector")
    refused(L.tfhe_hip_ring_lookup_device(None, vp(ring), 4, N, vp(out)), "null or deleted selector")
    for call in (lambda: L.tfhe_hip_ring_lookup(sel.ptr, None, 4, N, i32p(out)),
                 lambda: L.tfhe_hip_ring_lookup(sel.ptr, i32p(ring), 4, N, None),
                 lambda: L.tfhe_hip_ring_lookup_device(sel.ptr, None, 4, N, vp(out)),
                 lambda: L.tfhe_hip_ring_lookup_device(sel.ptr, vp(ring), 4, N, None)):
        refused(call(), "null ring words or destination")
    # width: a power of two in 1..N
    for width in (0, -128, 3, 96, 2 * N, 1 << 30):
        refused(L.tfhe_hip_ring_lookup(sel.ptr, i32p(ring), 4, width, i32p(out)), "width must be a power of two in 1..1024")
    # d < s: entries of 64 coefficients need 4 rotation bits, the selector has 3
    for width in (64, 1):
        refused(L.tfhe_hip_ring_lookup(sel.ptr, i32p(ring), 4, width, i32p(out)), "the selector has 3 bits")
    # M < 1, M > 2^d
    for M in (0, -3, 9, 1 << 30):
        refused(L.tfhe_hip_ring_lookup(sel.ptr, i32p(ring), M, 128, i32p(out)), "M must be in 1..2^3")
        refused(L.tfhe_hip_ring_lookup_device(sel.ptr, vp(ring), M, 128, vp(out)), "M must be in 1..2^3")
    # misaligned device words, either side
    refused(L.tfhe_hip_ring_lookup_device(sel.ptr, vp(ring, 4), 8, 128, vp(out)), "16-byte aligned")
    refused(L.tfhe_hip_ring_lookup_device(sel.ptr, vp(ring), 8, 128, vp(out, 8)), "16-byte aligned")
    none = api.Selector(pp)                                         # d = 0 takes whole samples only
    refused(L.tfhe_hip_ring_lookup(none.ptr, i32p(ring), 1, 512, i32p(out)), "the selector has 0 bits")
    refused(L.tfhe_hip_ring_lookup(none.ptr, i32p(ring), 2, N, i32p(out)), "M must be in 1..2^0")
    # the raw entry
    for call, needle in ((lambda: L.tfhe_hip_kernel_ring_cmux_rotate(None, 0, 1, i32p(ring), 1, i32p(out)), "null or deleted selector"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, 1, None, 1, i32p(out)), "null argument"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, 1, i32p(ring), 1, None), "null argument"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 3, 1, i32p(ring), 1, i32p(out)), "bit_index must be in 0..2"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, -1, 1, i32p(ring), 1, i32p(out)), "bit_index must be in 0..2"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, 0, i32p(ring), 1, i32p(out)), "rot must be in 1..1023"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, N, i32p(ring), 1, i32p(out)), "rot must be in 1..1023"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, -5, i32p(ring), 1, i32p(out)), "rot must be in 1..1023"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, 1, i32p(ring), 0, i32p(out)), "count must be in 1.."),
                         (lambda: L.tfhe_hip_kernel_ring_cmux_rotate(sel.ptr, 0, 1, i32p(ring), 65537, i32p(out)), "count must be in 1..")):
        refused(call(), needle)
    assert (out == 0x5A5A5A5A).all()
    # the Python layer counts the gallery's samples before it calls in
    with pytest.raises(ValueError, match="holds 1 ring samples"):
        api.ring_lookup(sel, ring, 8, 128)
    with pytest.raises(ValueError, match="power of two"):
        api.ring_lookup(sel, ring, 4, 100)

    # the select's own entries keep their words after refused lookups: the same refusals, the same texts, a clean error state
    refused(L.tfhe_hip_ring_lookup(sel.ptr, i32p(ring), 4, 3, i32p(out)), "width must be")
    assert api.last_error() == "" and L.tfhe_hip_selector_bits(sel.ptr) == 3
    refused(L.tfhe_hip_ring_select(sel.ptr, i32p(ring), 9, i32p(out)), "tfhe_hip_ring_select: M must be in 1..2^3")
    refused(L.tfhe_hip_ring_select(sel.ptr, None, 4, i32p(out)), "tfhe_hip_ring_select: null ring words or destination")
    refused(L.tfhe_hip_ring_select_device(sel.ptr, vp(ring, 4), 4, vp(out)), "tfhe_hip_ring_select_device: device words must be 16-byte aligned")
    assert (out == 0x5A5A5A5A).all()
    sel.close()
    none.close()
    assert api.last_error() == ""
