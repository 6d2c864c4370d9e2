"""The private selection without a GPU: the client's TGSW encryptor, the numpy restatement of the CMUX tree
(tests/select_common.py) at decrypt level, every refusal of the server-side entries -- all of them checked before the
device is looked at -- and the two bounds of the CMUX kernel (peba1_amd/csrc/cmux.hpp) over every gadget a cloud key is
accepted with."""
import ctypes as C

import numpy as np
import pytest

import select_common as S

SEED = 0x5E1EC7
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


def test_word_count_and_seeded_encryption_is_reproducible(L, host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    assert api.tgsw_words(pp) == 2 * pp.l * 2 * pp.N
    a = api.tgsw_encrypt_bits([1, 0, 1], ks, seed=7)
    assert a.shape == (3, 2 * pp.l, 2, pp.N)
    assert np.array_equal(a, api.tgsw_encrypt_bits([1, 0, 1], ks, seed=7))
    assert not np.array_equal(a, api.tgsw_encrypt_bits([1, 0, 1], ks, seed=8))
    # one stream for the call: the first bit's words do not depend on the bits behind it, the masks not on the bits at all
    b = api.tgsw_encrypt_bits([1, 1], ks, seed=7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1, :, 0, :][pp.l:], b[1, :, 0, :][pp.l:])
    # the unseeded form draws fresh streams
    assert not np.array_equal(api.tgsw_encrypt_bits([1], ks), api.tgsw_encrypt_bits([1], ks))


def test_every_row_carries_the_bit_times_its_gadget_power_on_its_polynomial(host_keys, capsys):
    """row (u, p) minus bit << (32 - (p+1) Bgbit) at coefficient 0 of polynomial u is an encryption of zero: every phase
    within 6 sigma of bk_stdev.  The body rows show the message directly; the message taken from the other polynomial
    leaves a phase far outside."""
    from peba1_amd import api
    pp, ks = host_keys
    bits = [1, 0, 1, 1]
    words = api.tgsw_encrypt_bits(bits, ks, seed=11)
    six_sigma = 6 * S.STDEVS[1] * 2.0 ** 32
    worst = 0.0
    for b, bit in enumerate(bits):
        for u in range(2):
            for p in range(pp.l):
                g = bit << (32 - (p + 1) * pp.Bgbit)
                row = words[b, u * pp.l + p].astype(np.int64)
                if u == 1:
                    assert abs(int(api.packed_phases(S.to_i32(row), ks)[0]) - g) <= six_sigma
                row[u, 0] -= g
                ph = api.packed_phases(S.to_i32(row), ks).astype(np.float64)
                worst = max(worst, np.abs(ph).max())
                assert np.abs(ph).max() <= six_sigma, (b, u, p)
                if bit:
                    row[u, 0] += g
                    row[1 - u, 0] -= g
                    assert np.abs(api.packed_phases(S.to_i32(row), ks).astype(np.float64)).max() > six_sigma, (b, u, p)
    with capsys.disabled():
        print("\nTGSW rows: largest |phase| of a row less its message %.1f of 6 sigma = %.1f (torus32 units)" % (worst, six_sigma))


@pytest.fixture(scope="module")
def gallery(host_keys):
    """eight ring-encrypted messages of 1,024 bits"""
    from peba1_amd import api
    pp, ks = host_keys
    bits = np.random.default_rng(3).integers(0, 2, (8, pp.N))
    ring = np.stack([api.ring_encrypt_bits(bits[m], ks, seed=100 + m).reshape(2, pp.N) for m in range(8)])
    return bits, ring


@pytest.mark.parametrize("M,d", [(1, 0), (2, 1), (3, 2), (5, 3), (8, 3)])
def test_numpy_tree_decrypts_to_the_indexed_entry(host_keys, gallery, M, d, capsys):
    from peba1_amd import api
    pp, ks = host_keys
    bits, ring = gallery
    sigma = (S.STDEVS[1] ** 2 + d * S.cmux_variance(pp.N, pp.l, pp.Bgbit, S.STDEVS[1])) ** 0.5
    worst = 0.0
    for index in range(M):
        ib = [(index >> j) & 1 for j in range(d)]
        sel = api.tgsw_encrypt_bits(ib, ks, seed=200 + index) if d else np.zeros((0, 2 * pp.l, 2, pp.N), dtype=np.int32)
        out = S.tree(sel, ring[:M], pp.l, pp.Bgbit)
        assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[index]), (M, index)
        ph = api.packed_phases(out, ks).astype(np.float64) / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(bits[index] == 1, 0.125, -0.125)).max())
    with capsys.disabled():
        print("\nnumpy tree M = %d, d = %d: largest |phase error| %.3e, computed sigma bound %.3e" % (M, d, worst, sigma))
    assert worst < 1.0 / 8


def test_an_index_at_or_past_M_gives_a_phase_near_zero(host_keys, gallery):
    from peba1_amd import api
    pp, ks = host_keys
    _, ring = gallery
    for M, d, index in ((3, 2, 3), (5, 3, 5), (5, 3, 7), (1, 2, 2)):
        sel = api.tgsw_encrypt_bits([(index >> j) & 1 for j in range(d)], ks, seed=300 + index)
        ph = api.packed_phases(S.tree(sel, ring[:M], pp.l, pp.Bgbit), ks).astype(np.float64) / 2.0 ** 32
        assert np.abs(ph).max() < 1.0 / 64, (M, index)          # a message stands at 1/8


def test_restatement_against_python_integers_at_the_extremes():
    """the worst-case operands of the GPU tests through the restatement on the CPU: a small ring is enough for the integers"""
    N, l, Bgbit = 64, 3, 7
    d0 = S.random_ring(np.random.default_rng(5), 1, N)[0]
    for word in (S.I32_MIN, S.I32_MAX):
        for which, digit in (("min", -2 ** (Bgbit - 1)), ("max", 2 ** (Bgbit - 1) - 1)):
            G = np.full((2 * l, 2, N), word, dtype=np.int32)
            d1 = S.to_i32(d0.astype(np.int64) + S.extreme_difference(l, Bgbit, which))
            want, most = S.extreme_closed_form(N, l, word, digit, d0)
            assert np.array_equal(S.cmux(G, d1, d0, l, Bgbit), want)
            assert most == 2 * l * N * abs(digit) * abs(word)


# ---- refusals: nothing is touched, the error is set, no device is looked at ----
def test_refusals_have_no_effect(L, host_keys):
    from peba1_amd import api
    pp, ks = host_keys
    N = pp.N
    words = api.tgsw_encrypt_bits([1, 0], ks, seed=1)
    flat = np.ascontiguousarray(words.reshape(-1))
    ring = S.random_ring(np.random.default_rng(6), 4, N)
    out = np.full(2 * N, 0x5A5A5A5A, dtype=np.int32)

    def refused(rc, needle):
        """-1 (or a null object) came back, the error names the reason; cleared for the next case"""
        assert rc in (-1, None) and needle in api.last_error(), (rc, api.last_error())
        L.tfhe_hip_clear_error()

    # the encryptor
    buf = np.full(api.tgsw_words(pp), 0x33333333, dtype=np.int32)
    one = np.array([1], dtype=np.int32)
    for call in (lambda: L.tfhe_hip_tgsw_encrypt_bits(None, i32p(one), 1, i32p(buf)),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits(ks.ptr, None, 1, i32p(buf)),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits(ks.ptr, i32p(one), 1, None),
                 lambda: L.tfhe_hip_tgsw_encrypt_bits_seeded(ks.ptr, i32p(one), 1, None, 5)):
        refused(call(), "null argument")
    for count in (0, 21):
        assert L.tfhe_hip_tgsw_encrypt_bits_seeded(ks.ptr, i32p(one), count, i32p(buf), 5) == -1
        refused(-1, "count must be in 1..20")
    assert (buf == 0x33333333).all()
    assert L.tfhe_hip_tgsw_words(None) == -1
    refused(-1, "null parameter set")

    # the constructor
    assert L.tfhe_hip_new_selector(None, i32p(flat), 2) is None
    refused(None, "null parameter set")
    assert L.tfhe_hip_new_selector(pp.ptr, None, 2) is None
    refused(None, "null words")
    for nbits in (-1, 21):
        assert L.tfhe_hip_new_selector(pp.ptr, i32p(flat), nbits) is None
        refused(None, "nbits must be in 0..20")
    with pytest.raises(ValueError, match="words per bit"):          # wrong word counts
        api.Selector(pp, flat[:-1])
    with pytest.raises(ValueError, match="words per bit"):
        api.Selector(pp, flat[:api.tgsw_words(pp) // 2])
    assert L.tfhe_hip_selector_bits(None) == -1
    refused(-1, "null or deleted selector")

    # a gadget outside the bounds: beyond the CRT range, and beyond every kernel form (l = 10 at Bgbit = 3); k != 1
    for gadget, why in (((3, 10), "exact range of the two-prime NTT"), ((10, 3), "every blind-rotate kernel form")):
        bad = api.ParameterSet(custom=S.custom_tuple(N_LWE, gadget=gadget))
        assert L.tfhe_hip_new_selector(bad.ptr, i32p(flat), 1) is None
        refused(None, why)
    k2 = api.ParameterSet(custom=(N_LWE, 1024, 2, 3, 7, 8, 2) + S.STDEVS)
    assert L.tfhe_hip_new_selector(k2.ptr, i32p(flat), 1) is None
    refused(None, "k = 1")

    # the select: a null argument, M = 0, M > 2^d -- before the device is looked at (this machine has none)
    sel = api.Selector(pp, words)
    assert sel.nbits == 2 and L.tfhe_hip_selector_bits(sel.ptr) == 2
    refused(L.tfhe_hip_ring_select(None, i32p(ring), 4, i32p(out)), "null or deleted selector")
    for call in (lambda: L.tfhe_hip_ring_select(sel.ptr, None, 4, i32p(out)),
                 lambda: L.tfhe_hip_ring_select(sel.ptr, i32p(ring), 4, None),
                 lambda: L.tfhe_hip_ring_select_device(sel.ptr, None, 4, C.c_void_p(out.ctypes.data)),
                 lambda: L.tfhe_hip_ring_select_device(sel.ptr, C.c_void_p(ring.ctypes.data), 4, None)):
        refused(call(), "null ring words or destination")
    for M in (0, -3, 5, 1 << 30):
        assert L.tfhe_hip_ring_select(sel.ptr, i32p(ring), M, i32p(out)) == -1
        refused(-1, "M must be in 1..2^2")
    assert L.tfhe_hip_ring_select_device(sel.ptr, C.c_void_p(ring.ctypes.data + 4), 4, C.c_void_p(out.ctypes.data)) == -1
    refused(-1, "16-byte aligned")
    none = api.Selector(pp)                                         # d = 0 takes a gallery of one only
    assert none.nbits == 0
    assert L.tfhe_hip_ring_select(none.ptr, i32p(ring), 2, i32p(out)) == -1
    refused(-1, "M must be in 1..2^0")
    # the raw entry
    for call, needle in ((lambda: L.tfhe_hip_kernel_ring_cmux(sel.ptr, 0, None, i32p(ring), 1, i32p(out)), "null argument"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux(sel.ptr, 2, i32p(ring), i32p(ring), 1, i32p(out)), "bit_index must be in 0..1"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux(sel.ptr, -1, i32p(ring), i32p(ring), 1, i32p(out)), "bit_index must be in 0..1"),
                         (lambda: L.tfhe_hip_kernel_ring_cmux(sel.ptr, 0, i32p(ring), i32p(ring), 0, i32p(out)), "count must be in 1..")):
        refused(call(), needle)
    assert (out == 0x5A5A5A5A).all()
    sel.close()
    none.close()
    assert api.last_error() == ""
    L.tfhe_hip_delete_selector(None)
    assert api.last_error() == ""


# ---- the two bounds ----
def test_bounds_hold_for_every_gadget_a_cloud_key_is_accepted_with(L):
    """tfhe_hip_test_select_bounds over the whole grid: the library's answer is the restatement's, every gadget that
    tfhe_hip_test_form_admissible and the CRT range admit passes both bounds, and the frontier is where the derivation
    puts it ((k+1) l <= 18 at N = 1,024, <= 16 at N = 2,048)."""
    ok = L.tfhe_hip_test_form_admissible
    accepted = 0
    for N in (1024, 2048):
        for g in S.grid(N):
            _, l, B = g
            got = L.tfhe_hip_test_select_bounds(N, l, B)
            assert got == (0 if S.mac_ok(N, l) else 1) | (0 if S.crt_ok(N, l, B) else 2), g
            if S.cloud_key_accepted(ok, g):
                accepted += 1
                assert got == 0, g
    assert accepted >= 90                     # about 60 gadgets at N = 1,024 and 50 at N = 2,048
    assert S.mac_ok(1024, 9) and not S.mac_ok(1024, 10) and S.mac_ok(2048, 8) and not S.mac_ok(2048, 9)
    assert L.tfhe_hip_test_select_bounds(1024, 10, 3) == 1 and L.tfhe_hip_test_select_bounds(1024, 3, 10) == 2
    assert L.tfhe_hip_test_select_bounds(2048, 9, 3) == 1 and L.tfhe_hip_test_select_bounds(2048, 2, 10) == 2
    for bad in ((512, 3, 7), (1024, 0, 7), (1024, 3, 13), (1024, 5, 7)):
        assert L.tfhe_hip_test_select_bounds(*bad) == -1
    L.tfhe_hip_clear_error()
