"""The packing key switch on the GPU, word for word against the numpy restatement (tests/pack_common.py).

P128 at its real width with inputs that are partly still pending at the call; one non-default decomposition per accepted
digit width on a small odd LWE width, with a tail range of mask indices; N = 2048; crafted keys and samples at the
largest magnitudes every accepted digit width admits; the device form; two keys alive at once; an exhausted device at the
first pack; and 1,024 gate outputs that must all decrypt right.  Every comparison of words is exact."""
import ctypes as C

import numpy as np
import pytest

import pack_common as K

pytestmark = pytest.mark.gpu

N_SMALL = 33                    # odd: with 4 mask indices per workgroup the last range holds one
SEED, PK_SEED = 0x7AC2, 0x0DDB
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def p128(p128_keys):
    """(parameter set, device keyset, packing key of the default decomposition, its rows for the restatement)"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    pk = api.PackingKey(ks, seed=PK_SEED)
    yield pp, ks, pk, K.KeyRows(pk.words())
    pk.close()


def _custom(n_ring, gadget):
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(N_SMALL, N=n_ring, gadget=gadget))
    return pp, api.SecretKeySet(pp, SEED, device=True)


@pytest.fixture(scope="module")
def small1024():
    pp, ks = _custom(1024, K.GADGET)
    yield pp, ks
    ks.close()


@pytest.fixture(scope="module")
def small2048():
    pp, ks = _custom(2048, (3, 6))
    yield pp, ks
    ks.close()


def random_samples(rng, count, n):
    return rng.integers(I32_MIN, I32_MAX + 1, size=(count, n + 1), dtype=np.int64).astype(np.int32)


def assert_words(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("count", [1, 2, 65, 1024])
def test_p128_pack_observes_a_recording(L, p128, count):
    """coefficient 0 alone, a lane boundary, a register boundary, the full ring: fresh encryptions mixed with bootsAND
    results that are still pending when the pack is called -- the pack runs them first"""
    from peba1_amd import api
    pp, ks, pk, rows = p128
    rng = np.random.default_rng(count)
    bits = rng.integers(0, 2, count)
    m = min(count, 3)                                              # the first m samples are gate results
    xa, xb = rng.integers(0, 2, m), rng.integers(0, 2, m)
    L.tfhe_hip_set_encrypt_seed(1000 + count)
    s = api.CiphertextArray(pp, count).encrypt(bits, ks)
    a, b = api.CiphertextArray(pp, m).encrypt(xa, ks), api.CiphertextArray(pp, m).encrypt(xb, ks)
    api.set_deferred(True)
    api.flush()
    before = api.stats()
    for j in range(m):
        L.bootsAND(s.at(j), a.at(j), b.at(j), ks.cloud)
    assert api.stats()["blind_rotates"] == before["blind_rotates"]             # recorded, not run
    got = api.pack(pk, s, count, ks)
    after = api.stats()
    assert after["blind_rotates"] - before["blind_rotates"] == m and after["flushes"] - before["flushes"] == 1
    assert_words(got, K.pack_ref(rows, s.words(), pk.basebit), ("P128", count))
    bits[:m] = xa & xb
    assert list(api.packed_decrypt(got, count, ks)) == list(bits)
    for o in (s, a, b):
        o.close()


def test_p128_1024_gate_outputs_all_decrypt_right(L, p128, capsys):
    """the full ring at the real width: 1,024 bootsAND / bootsXOR outputs of known bits, packed while pending; every word
    is the restatement's and all 1,024 bits decrypt right -- each stands 1/8 from the boundary, the computed sigma of the
    pack is 1.5e-4.  Prints the largest |phase error| against the gate outputs' own phases, beside that sigma."""
    from peba1_amd import api
    pp, ks, pk, rows = p128
    count = pp.N
    rng = np.random.default_rng(5)
    xa, xb = rng.integers(0, 2, count), rng.integers(0, 2, count)
    L.tfhe_hip_set_encrypt_seed(4242)
    a, b = api.CiphertextArray(pp, count).encrypt(xa, ks), api.CiphertextArray(pp, count).encrypt(xb, ks)
    r = api.CiphertextArray(pp, count)
    api.set_deferred(True)
    half = count // 2
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], r.at(0), a.at(0), b.at(0), half, ks.cloud) == 0
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["XOR"], r.at(half), a.at(half), b.at(half), count - half, ks.cloud) == 0
    got = api.pack(pk, r, count, ks)
    want_bits = np.concatenate([(xa & xb)[:half], (xa ^ xb)[half:]])
    assert list(api.packed_decrypt(got, count, ks)) == list(want_bits)
    words = r.words()
    assert_words(got, K.pack_ref(rows, words, pk.basebit), "P128 full ring")
    lwe = ks.lwe_key().astype(np.int64)
    in_phase = K.to_i32(words[:, pp.n].astype(np.int64) - (words[:, :pp.n].astype(np.int64) % 2 ** 32) @ lwe).astype(np.int64)
    err = K.to_i32(api.packed_phases(got, ks).astype(np.int64) - in_phase).astype(np.float64) / 2.0 ** 32
    sigma = K.pack_variance(pp.n, pk.t, pk.basebit, count, K.STDEVS[1]) ** 0.5
    with capsys.disabled():
        print("\npack P128 count 1024: largest |phase error| %.3e, computed sigma %.3e (%.2f sigma)"
              % (np.abs(err).max(), sigma, np.abs(err).max() / sigma))
    assert np.abs(err).max() < 1.0 / 16                             # far inside the margin; the condition is the bits above
    for o in (a, b, r):
        o.close()


@pytest.mark.parametrize("t,bb", [(11, 1), (6, 2), (5, 3), (3, 4)])
def test_every_digit_width_on_a_small_set(small1024, t, bb):
    """one non-default decomposition per accepted digit width, n = 33: the full ring and a count inside a register, with
    one mask index per workgroup and with four (eight full ranges and a tail of one)"""
    from peba1_amd import api
    pp, ks = small1024
    pk = api.PackingKey(ks, t, bb, seed=PK_SEED + bb)
    rows = K.KeyRows(pk.words())
    rng = np.random.default_rng(100 + bb)
    for count in (pp.N, 700):
        sw = random_samples(rng, count, pp.n)
        want = K.pack_ref(rows, sw, bb)
        for ipw in (0, 4):
            assert_words(api.kernel_pack(pk, ks, sw, idx_per_wg=ipw), want, ((t, bb), count, ipw))
    pk.close()


@pytest.mark.parametrize("count", [3, 2048])
def test_n2048(L, small2048, count):
    """LOGN = 11: 32 coefficients per lane; through the slots (count 3, gate-free) and from raw words (the full ring)"""
    from peba1_amd import api
    pp, ks = small2048
    assert pp.N == 2048
    pk = api.PackingKey(ks, seed=PK_SEED)
    rows = K.KeyRows(pk.words())
    rng = np.random.default_rng(count)
    sw = random_samples(rng, count, pp.n)
    want = K.pack_ref(rows, sw, pk.basebit)
    for ipw in (0, 5):
        assert_words(api.kernel_pack(pk, ks, sw, idx_per_wg=ipw), want, ("N2048 raw", count, ipw))
    if count == 3:
        s = api.CiphertextArray(pp, count).set_words(sw)
        assert_words(api.pack(pk, s, count, ks), want, "N2048 slots")
        s.close()
    pk.close()


@pytest.mark.parametrize("n_ring", [1024, 2048])
@pytest.mark.parametrize("bb", [1, 2, 3, 4])
def test_worst_case_magnitudes(small1024, small2048, n_ring, bb):
    """crafted key words at INT32_MIN / INT32_MAX, samples whose every digit is base - 1, count = N, at the largest t the
    bounds admit for the digit width: where an accumulator that takes too many rows, or a chunk too large for the CRT,
    would wrap"""
    from peba1_amd import api
    pp, ks = small1024 if n_ring == 1024 else small2048
    t = K.largest_t(n_ring, bb)
    assert K.accepted(n_ring, t, bb) and not K.accepted(n_ring, t + 1, bb)
    rng = np.random.default_rng(bb)
    top = (2 ** (t * bb) - 1) * 2 ** (32 - t * bb)                  # every digit base - 1, nothing below them
    sw = np.empty((n_ring, pp.n + 1), dtype=np.int32)
    sw[:, :pp.n] = K.to_i32(top)
    sw[:, pp.n] = random_samples(rng, n_ring, 0)[:, 0]
    assert (K.digits_of(sw[:, :pp.n], t, bb) == 2 ** bb - 1).all()
    shape = (pp.n, t, 2, n_ring)
    keys = {"all INT32_MIN": np.full(shape, I32_MIN, dtype=np.int64),
            "all INT32_MAX": np.full(shape, I32_MAX, dtype=np.int64),
            "MIN / MAX by coin": np.where(rng.integers(0, 2, shape) == 1, I32_MIN, I32_MAX)}
    for name, words in keys.items():
        pk = api.PackingKey.from_words(pp, t, bb, words.astype(np.int32))
        want = K.pack_ref(K.KeyRows(pk.words()), sw, bb)
        assert_words(api.kernel_pack(pk, ks, sw), want, (n_ring, (t, bb), name))
        pk.close()


def test_device_form_two_keys_and_an_exhausted_device(L, small1024):
    """two packing keys of different decompositions alive at once, packing in turn; the device form's words are the host
    form's; a device without room for a key's image at its first pack refuses the call, recoverably"""
    import torch
    from peba1_amd import api
    pp, ks = small1024
    rng = np.random.default_rng(9)
    count = 130
    sw = random_samples(rng, count, pp.n)
    s = api.CiphertextArray(pp, count).set_words(sw)
    pa, pb = api.PackingKey(ks, seed=1), api.PackingKey(ks, 5, 3, seed=2)
    want_a, want_b = K.pack_ref(K.KeyRows(pa.words()), sw, 2), K.pack_ref(K.KeyRows(pb.words()), sw, 3)
    # the first pack of key a on a device with no room left: refused, nothing written, and fine once there is room
    out = np.full(2 * pp.N, 7, dtype=np.int32)
    L.tfhe_hip_test_set_alloc_cap(1)
    rc = L.tfhe_hip_pack_samples(pa.ptr, s.ptr, count, ks.cloud, out.ctypes.data_as(C.POINTER(C.c_int32)))
    L.tfhe_hip_test_set_alloc_cap(0)
    assert rc == -1 and "out of device memory" in api.last_error() and "packing key" in api.last_error() and (out == 7).all()
    L.tfhe_hip_clear_error()
    for _ in range(2):
        assert_words(api.pack(pa, s, count, ks), want_a, "key a")
        assert_words(api.pack(pb, s, count, ks), want_b, "key b")
    dev = torch.zeros(2 * pp.N, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    api.pack_device(pb, s, count, ks, dev.data_ptr())
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(dev.cpu().numpy(), want_b, "device form")
    assert api.last_error() == ""
    for o in (pa, pb, s):
        o.close()
