"""Seed-compressed selectors and TGSW probes without a GPU (include/tfhe_hip.h "seed-compressed selectors"): the record's
size, the host expansion against the numpy restatement (tests/seeded_select_common.py) word for word, the gadget term of every
row at phase level -- sign, level and key polynomial --, the numpy CMUX tree (tests/select_common.py) under a host-expanded
selector, the one-seed-per-record rule, and every refusal -- all of them checked before the device is looked at."""
import ctypes as C

import numpy as np
import pytest

import seeded_select_common as Z
import select_common as S

SEED = 0x5EED5E1
N_LWE = 10                    # the LWE side plays no part: a short key is made quickly
MARGIN = 1.0 / 8              # the select's decode margin (tests/test_select_cpu.py, test_numpy_tree_decrypts_to_the_indexed_entry)


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


def test_record_size_is_the_formula(L):
    from peba1_amd import api
    for name, (N, l, _) in S.SETS.items():
        pp = Z.params_of(name)
        for count in (0, 1, 3, Z.SELECT_MAX_BITS):
            assert api.tgsw_compressed_words(pp, count) == 10 + count * 2 * l * N == Z.compressed_words(1, l, N, count), (name, count)
    p128 = Z.params_of("P128")
    assert api.tgsw_compressed_words(p128, 1) == 6154 and api.tgsw_words(p128) == 12288
    assert L.tfhe_hip_tgsw_compressed_words(None, 1) == -1 and "null parameter set" in api.last_error()
    assert L.tfhe_hip_tgsw_compressed_words(p128.ptr, -1) == -1 and "negative" in api.last_error()
    L.tfhe_hip_clear_error()


@pytest.mark.parametrize("count", [1, 3, Z.SELECT_MAX_BITS])
def test_host_expansion_of_bits_is_the_restatement_word_for_word(L, host_keys, count):
    from peba1_amd import api
    pp, ks = host_keys
    bits = [(5 * b + 1) % 3 % 2 for b in range(count)]
    rec = api.tgsw_encrypt_bits_compressed(bits, ks, seed=40 + count)
    assert rec.shape == (Z.compressed_words(1, pp.l, pp.N, count),)
    got = api.tgsw_expand(rec, pp)
    assert got.shape == (count, 2 * pp.l, 2, pp.N)
    assert np.array_equal(got, Z.expand(L, rec, 1, pp.l, pp.N))
    # a prefix of the record's samples is a prefix of its stream: what a selector of fewer bits reads
    if count == 3:
        assert np.array_equal(api.tgsw_expand(rec[:10 + 2 * 2 * pp.l * pp.N], pp), got[:2])


def test_host_expansion_of_a_polynomial_sample_is_the_restatement(L, host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    q = np.random.default_rng(8).integers(-1, 2, (1, pp.N))
    rec = api.tgsw_encrypt_polys_compressed(q, ks, seed=9)
    assert np.array_equal(api.tgsw_expand(rec, pp), Z.expand(L, rec, 1, pp.l, pp.N))
    # and the expanded sample is NOT the plain encryptor's: no mask word depends on the message
    assert not np.array_equal(api.tgsw_expand(rec, pp), api.tgsw_encrypt_polys(q, ks, seed=9))
    other = api.tgsw_encrypt_polys_compressed(-q, ks, seed=9)
    assert np.array_equal(api.tgsw_expand(other, pp)[:, :, 0, :], api.tgsw_expand(rec, pp)[:, :, 0, :])


def check_noise(noise, sigma32, what, capsys):
    """the largest |value| below 6 sigma, the sample mean within 6 sigma / sqrt(count) of zero"""
    count = noise.size
    worst, mean = np.abs(noise).max(), float(noise.mean())
    with capsys.disabled():
        print("\n%s: %d phases less their gadget terms: largest %.1f of 6 sigma = %.1f, mean %.3f of 6 sigma / sqrt(count) = %.3f "
              "(torus32 units), sample sigma %.1f of %.1f" % (what, count, worst, 6 * sigma32, mean, 6 * sigma32 / count ** 0.5,
                                                              noise.std(), sigma32))
    assert worst < 6 * sigma32, what
    assert abs(mean) <= 6 * sigma32 / count ** 0.5, what


def test_every_expanded_row_carries_its_gadget_term_on_the_body(L, host_keys, capsys):
    """phase - g_p m on body rows, phase + g_p (m s_u) on mask rows is the row's noise, for bits 0 and 1 and a polynomial
    of coefficients in {-1, 0, 1}.  A term of the wrong sign, level or key polynomial leaves at least g_(l-1) = 2^11 on a
    coefficient, against 6 sigma = 768."""
    from peba1_amd import api
    pp, ks = host_keys
    sigma32 = S.STDEVS[1] * 2.0 ** 32
    key = ks.tlwe_key()
    bits = [0, 1, 1, 0]
    words = api.tgsw_expand(api.tgsw_encrypt_bits_compressed(bits, ks, seed=21), pp)
    check_noise(Z.noise_of(words, Z.constant_polys(bits, pp.N), 1, pp.l, pp.Bgbit, key), sigma32, "bits 0, 1, 1, 0", capsys)
    q = np.random.default_rng(22).integers(-1, 2, (2, pp.N))
    words_q = api.tgsw_expand(api.tgsw_encrypt_polys_compressed(q, ks, seed=23), pp)
    check_noise(Z.noise_of(words_q, q, 1, pp.l, pp.Bgbit, key), sigma32, "two polynomials in {-1, 0, 1}", capsys)
    # the check does tell: the bit-1 sample read as a 0, and the polynomial with its sign turned, leave the gadget term
    assert np.abs(Z.noise_of(words[1:2], Z.constant_polys([0], pp.N), 1, pp.l, pp.Bgbit, key)).max() > 6 * sigma32
    assert np.abs(Z.noise_of(words_q[:1], -q[:1], 1, pp.l, pp.Bgbit, key)).max() > 6 * sigma32
    # a bit is the constant polynomial: under one seed the two encryptors give the same record
    assert np.array_equal(api.tgsw_encrypt_polys_compressed(Z.constant_polys(bits, pp.N), ks, seed=21),
                          api.tgsw_encrypt_bits_compressed(bits, ks, seed=21))


def test_numpy_tree_under_a_host_expanded_selector_selects_every_entry(host_keys, capsys):
    """tests/select_common.py's tree over 8 ring samples of random bits, the 3-bit selector a host-expanded compressed
    record: every index decrypts to its entry, the largest phase error inside the select's margin"""
    from peba1_amd import api
    pp, ks = host_keys
    bits = np.random.default_rng(31).integers(0, 2, (8, pp.N))
    ring = np.stack([api.ring_encrypt_bits(bits[m], ks, seed=700 + m).reshape(2, pp.N) for m in range(8)])
    worst = 0.0
    for index in range(8):
        rec = api.tgsw_encrypt_bits_compressed([(index >> j) & 1 for j in range(3)], ks, seed=800 + index)
        out = S.tree(api.tgsw_expand(rec, pp), ring, pp.l, pp.Bgbit)
        assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[index]), index
        ph = api.packed_phases(out, ks).astype(np.float64) / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(bits[index] == 1, 0.125, -0.125)).max())
    with capsys.disabled():
        print("\nnumpy tree under host-expanded compressed selectors, 8 entries, 3 levels: largest |phase error| %.3e (margin %.3f)"
              % (worst, MARGIN))
    assert worst < MARGIN


def test_seeded_form_is_reproducible_and_unseeded_records_have_seeds_of_their_own(host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    a = api.tgsw_encrypt_bits_compressed([1, 0, 1], ks, seed=7)
    assert np.array_equal(a, api.tgsw_encrypt_bits_compressed([1, 0, 1], ks, seed=7))
    b = api.tgsw_encrypt_bits_compressed([1, 0, 1], ks, seed=8)
    assert not np.array_equal(a[:10], b[:10]) and not np.array_equal(a[10:], b[10:])
    # one generator for the record: the seed words do not depend on the message, the first sample not on those behind it
    c = api.tgsw_encrypt_bits_compressed([1, 1], ks, seed=7)
    per = 2 * pp.l * pp.N
    assert np.array_equal(a[:10 + per], c[:10 + per])
    u, v = api.tgsw_encrypt_bits_compressed([1], ks), api.tgsw_encrypt_bits_compressed([1], ks)
    assert len(set(u[:10].tolist()) | set(v[:10].tolist())) > 10 and not np.array_equal(u[:10], v[:10])
    assert not np.array_equal(u[10:], v[10:])
    q = np.zeros((1, pp.N), dtype=np.int32)
    assert not np.array_equal(api.tgsw_encrypt_polys_compressed(q, ks)[:10], api.tgsw_encrypt_polys_compressed(q, ks)[:10])


def test_refusals_have_no_effect(L, host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    rec = api.tgsw_encrypt_bits_compressed([1, 0], ks, seed=1)

    def refused(rc, needle):
        assert rc in (-1, None) and needle in api.last_error(), (rc, api.last_error())
        L.tfhe_hip_clear_error()

    # the encryptors: null arguments, count 0 and SELECT_MAX_BITS + 1; the output stays as it was
    buf = np.full(api.tgsw_compressed_words(pp, 1), 0x33333333, dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    poly = np.zeros(pp.N, dtype=np.int32)
    for call in (lambda: L.tfhe_hip_tgsw_encrypt_bits_compressed(None, i32p(one), 1, i32p(buf)),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits_compressed(ks.ptr, None, 1, i32p(buf)),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits_compressed(ks.ptr, i32p(one), 1, None),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits_compressed_seeded(ks.ptr, i32p(one), 1, None, 5),
                 lambda: L.tfhe_hip_tgsw_encrypt_polys_compressed(ks.ptr, None, 1, i32p(buf)),
                 lambda: L.tfhe_hip_tgsw_encrypt_polys_compressed_seeded(None, i32p(poly), 1, i32p(buf), 5)):
        refused(call(), "null argument")
    for count in (0, Z.SELECT_MAX_BITS + 1):
        refused(L.tfhe_hip_tgsw_encrypt_bits_compressed_seeded(ks.ptr, i32p(one), count, i32p(buf), 5), "count must be in 1..20")
        refused(L.tfhe_hip_tgsw_encrypt_bits_compressed(ks.ptr, i32p(one), count, i32p(buf)), "count must be in 1..20")
        refused(L.tfhe_hip_tgsw_encrypt_polys_compressed_seeded(ks.ptr, i32p(poly), count, i32p(buf), 5), "count must be in 1..20")
    assert (buf == 0x33333333).all()

    # the host expansion
    out = np.full(2 * api.tgsw_words(pp), 0x5A5A5A5A, dtype=np.int32)
    for call in (lambda: L.tfhe_hip_tgsw_expand_host(None, i32p(rec), 2, i32p(out)),
                 lambda: L.tfhe_hip_tgsw_expand_host(pp.ptr, None, 2, i32p(out)),
                 lambda: L.tfhe_hip_tgsw_expand_host(pp.ptr, i32p(rec), 2, None)):
        refused(call(), "null argument")
    for count in (0, Z.SELECT_MAX_BITS + 1):
        refused(L.tfhe_hip_tgsw_expand_host(pp.ptr, i32p(rec), count, i32p(out)), "count must be in 1..20")
    assert (out == 0x5A5A5A5A).all()
    with pytest.raises(ValueError, match="words per sample"):
        api.tgsw_expand(rec[:-1], pp)

    # the constructor: tfhe_hip_new_selector's refusals in its words, then its own
    new = L.tfhe_hip_new_selector_compressed
    refused(new(None, i32p(rec), 2, 2), "null parameter set")
    refused(new(pp.ptr, None, 2, 2), "null words")
    for count in (0, Z.SELECT_MAX_BITS + 1):
        refused(new(pp.ptr, i32p(rec), count, 1), "count must be in 1..20")
    for nbits in (-1, Z.SELECT_MAX_BITS + 1):
        refused(new(pp.ptr, i32p(rec), 2, nbits), "nbits must be in 0..20")
    refused(new(pp.ptr, i32p(rec), 2, 3), "nbits = 3 is above the 2 samples of the record")
    with pytest.raises(ValueError, match="above the 2 samples"):
        api.Selector.from_compressed(pp, rec, nbits=3)
    L.tfhe_hip_clear_error()
    with pytest.raises(ValueError, match="words per sample"):
        api.Selector.from_compressed(pp, rec[:-1])
    for gadget, why in (((3, 10), "exact range of the two-prime NTT"), ((10, 3), "every blind-rotate kernel form")):
        bad = api.ParameterSet(custom=S.custom_tuple(N_LWE, gadget=gadget))
        flat = np.zeros(api.tgsw_compressed_words(bad, 1), dtype=np.int32)
        assert L.tfhe_hip_new_selector(bad.ptr, i32p(np.zeros(api.tgsw_words(bad), dtype=np.int32)), 1) is None
        plain_says = api.last_error().split(": ", 1)[1]
        refused(None, why)
        assert new(bad.ptr, i32p(flat), 1, 1) is None
        assert api.last_error() == "tfhe_hip_new_selector_compressed: " + plain_says
        refused(None, why)
    k2 = api.ParameterSet(custom=(N_LWE, 1024, 2, 3, 7, 8, 2) + S.STDEVS)
    refused(new(k2.ptr, i32p(np.zeros(api.tgsw_compressed_words(k2, 1), dtype=np.int32)), 1, 1), "k = 1")
    refused(L.tfhe_hip_selector_upload_bytes(None), "null or deleted selector")


def test_a_compressed_selector_is_made_used_for_refusals_and_deleted_without_a_device(L, host_keys):
    """construction, the accessors, the argument checks of the select and deletion: none of them looks at the device (this
    machine may have none)"""
    from peba1_amd import api
    pp, ks = host_keys
    rec = api.tgsw_encrypt_bits_compressed([1, 0, 1], ks, seed=3)
    sel = api.Selector.from_compressed(pp, rec)
    assert sel.nbits == 3 and L.tfhe_hip_selector_bits(sel.ptr) == 3 and sel.upload_bytes() == 0
    two = api.Selector.from_compressed(pp, rec, nbits=2)
    assert two.nbits == 2 and L.tfhe_hip_selector_bits(two.ptr) == 2
    none = api.Selector.from_compressed(pp, rec, nbits=0)
    assert none.nbits == 0 and none.upload_bytes() == 0
    ring = S.random_ring(np.random.default_rng(6), 4, pp.N)
    out = np.full(2 * pp.N, 0x5A5A5A5A, dtype=np.int32)
    assert L.tfhe_hip_ring_select(sel.ptr, i32p(ring), 9, i32p(out)) == -1 and "M must be in 1..2^3" in api.last_error()
    assert L.tfhe_hip_ring_select(sel.ptr, None, 4, i32p(out)) == -1 and "null ring words" in api.last_error()
    assert L.tfhe_hip_ring_lookup(two.ptr, i32p(ring), 4, 64, i32p(out)) == -1 and "rotation bits" in api.last_error()
    assert L.tfhe_hip_kernel_ring_cmux(sel.ptr, 3, i32p(ring), i32p(ring), 1, i32p(out)) == -1 and "bit_index must be in 0..2" in api.last_error()
    L.tfhe_hip_clear_error()
    assert (out == 0x5A5A5A5A).all()
    for s in (sel, two, none):
        s.close()
    assert api.last_error() == ""
