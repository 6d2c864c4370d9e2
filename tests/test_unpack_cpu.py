"""Ring-encrypted inputs without a GPU: the host ring encryption, its streams, host decryption through the packed-sample
entries, the numpy restatement of the sample extract (tests/unpack_common.py), the error channel of the unpack entries and
the two new statistics, on host-only keysets."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import unpack_common as U

N = 1024
N_LWE = 9                       # a small odd LWE width: the ring side is what is under test
SEED, RING_SEED, PK_SEED = 0x9AC4, 0x41C6, 0x51DE
BK_STDEV = U.STDEVS[1]


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def small():
    """(parameter set, host-only keyset) of a small custom set"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=U.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, SEED, device=False)
    yield pp, ks
    ks.close()


def _err(L):
    return L.tfhe_hip_last_error().decode()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_seeded_encryption_reproduces_and_differs_by_seed(small):
    from peba1_amd import api
    pp, ks = small
    mu = np.random.default_rng(1).integers(U.I32_MIN, U.I32_MAX + 1, N)
    a, b = api.ring_encrypt(mu, ks, seed=RING_SEED), api.ring_encrypt(mu, ks, seed=RING_SEED)
    c, d = api.ring_encrypt(mu, ks, seed=RING_SEED + 1), api.ring_encrypt(mu, ks)
    assert a.shape == (2 * N,) and np.array_equal(a, b)
    assert not np.array_equal(a, c) and not np.array_equal(a, d) and not np.array_equal(c, d)
    assert not np.array_equal(a[:N], c[:N])                                # the masks differ, not the noise alone
    bits = np.arange(N) % 2
    assert np.array_equal(api.ring_encrypt_bits(bits, ks, seed=7), api.ring_encrypt_bits(bits, ks, seed=7))
    assert not np.array_equal(api.ring_encrypt_bits(bits, ks, seed=7), api.ring_encrypt_bits(bits, ks, seed=8))
    assert not np.array_equal(api.ring_encrypt_bits(bits, ks), api.ring_encrypt_bits(bits, ks))


def test_ring_encryptions_leave_keyset_and_packing_key_streams_alone(small):
    """a seeded keyset's words and a seeded packing key's words are the same with or without ring encryptions (seeded and
    default) made in between"""
    from peba1_amd import api
    pp, ks = small
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    names = ("lwe_key", "tlwe_key", "bk", "ksk")
    first = api.SecretKeySet(pp, SEED, device=False)
    before = {name: digest(getattr(first, name)()) for name in names}
    pk_before = api.PackingKey(first, seed=PK_SEED)
    mu = np.zeros(N, dtype=np.int64)
    api.ring_encrypt(mu, first, seed=RING_SEED)
    api.ring_encrypt(mu, first)
    api.ring_encrypt_bits([1, 0, 1], first, seed=RING_SEED)
    api.ring_encrypt_bits([1, 0, 1], first)
    assert {name: digest(getattr(first, name)()) for name in names} == before
    pk_after = api.PackingKey(first, seed=PK_SEED)
    assert np.array_equal(pk_before.words(), pk_after.words())
    again = api.SecretKeySet(pp, SEED, device=False)                       # a keyset made after them draws the same words
    assert {name: digest(getattr(again, name)()) for name in names} == before
    assert {name: digest(getattr(ks, name)()) for name in names} == before
    for o in (pk_before, pk_after, first, again):
        o.close()


def test_phases_of_an_encrypted_message_are_the_message(small):
    """every coefficient's phase equals mu within 6 bk_stdev, through tfhe_hip_packed_phase and through the numpy ring
    phases; the seed is fixed, so the outcome is"""
    from peba1_amd import api
    pp, ks = small
    mu = np.random.default_rng(2).integers(U.I32_MIN, U.I32_MAX + 1, N)
    words = api.ring_encrypt(mu, ks, seed=RING_SEED)
    ph_lib = api.packed_phases(words, ks).astype(np.int64)
    ph_np = U.ring_phases(words.reshape(2, N), ks.tlwe_key()).astype(np.int64)
    assert np.array_equal(ph_lib, ph_np)
    err = U.to_i32(ph_lib - mu).astype(np.float64) / 2.0 ** 32
    assert np.abs(err).max() <= 6 * BK_STDEV, np.abs(err).max()
    assert 0.5 * BK_STDEV < err.std() < 1.5 * BK_STDEV                     # and it IS noise of bk_stdev, not zeros


@pytest.mark.parametrize("count", [1, 65, N])
def test_bits_decrypt_and_the_tail_carries_noise_only(small, count):
    from peba1_amd import api
    pp, ks = small
    bits = np.random.default_rng(count).integers(0, 2, count)
    words = api.ring_encrypt_bits(bits, ks, seed=RING_SEED + count)
    assert list(api.packed_decrypt(words, count, ks)) == list(bits)
    ph = api.packed_phases(words, ks).astype(np.float64) / 2.0 ** 32
    want = np.where(bits == 1, 0.125, -0.125)
    assert np.abs(ph[:count] - want).max() <= 6 * BK_STDEV
    if count < N:
        assert np.abs(ph[count:]).max() <= 6 * BK_STDEV and ph[count:].std() > 0.5 * BK_STDEV
    assert np.array_equal(api.ring_encrypt_bits(bits * 5, ks, seed=RING_SEED + count), words)      # any non-zero word is a 1


def test_extract_ref_is_consistent_with_the_ring_phase(small):
    """the phase of Extract_e under the extracted key (the ring key's bits) is coefficient e of the ring phase, for every
    e of two samples -- one mask all INT32_MIN, whose negation wraps to itself"""
    pp, ks = small
    rng = np.random.default_rng(3)
    ring = U.random_ring(rng, 2, N)
    ring[1, 0, :] = U.I32_MIN
    index = rng.permutation(2 * N)
    u = U.extract_ref(ring, index, N)
    assert u.shape == (2 * N, N + 1)
    ph = U.ring_phases(ring, ks.tlwe_key()).reshape(-1)
    assert np.array_equal(U.extracted_phases(u, ks.tlwe_key()), ph[index])
    # the definition at its ends, read off directly
    e0, eN = U.extract_ref(ring, [0, N - 1], N)
    assert e0[0] == ring[0, 0, 0] and np.array_equal(e0[1:N], U.to_i32(-ring[0, 0, :0:-1].astype(np.int64))) and e0[N] == ring[0, 1, 0]
    assert np.array_equal(eN[:N], ring[0, 0, ::-1]) and eN[N] == ring[0, 1, N - 1]
    assert (U.extract_ref(ring, [N + 5], N)[0, :N] == U.I32_MIN).all()


def test_unpack_errors_are_reported_and_leave_the_call_without_effect(small, L):
    """every refusal that can be raised without a device: -1, a message, the results as they were -- all decided before
    the device is looked at (this test runs without one)"""
    from peba1_amd import api, lib
    pp, ks = small
    cts = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    held = cts.words().copy()
    ring = U.random_ring(np.random.default_rng(4), 2, N)
    other_pp = api.ParameterSet(custom=U.custom_tuple(N_LWE + 2))
    other_cts = api.CiphertextArray(other_pp, 4)
    buf = np.zeros(pp.n + 16, dtype=np.int32)
    foreign = lib.LweSample()
    foreign.a = C.cast(buf.ctypes.data + 8 * 4, C.POINTER(C.c_int32))
    foreign.slot = 5
    idx = lambda *v: _i32p(np.array(v, dtype=np.int32))
    u_out = np.full((4, N + 1), 7, dtype=np.int32)

    def refused(rc, needle):
        assert rc == -1 and needle in _err(L), (rc, needle, _err(L))
        assert [cts.at(j).contents.slot for j in range(4)] == [-1] * 4 and np.array_equal(cts.words(), held)
        assert (u_out == 7).all()
        L.tfhe_hip_clear_error()

    for entry in (L.tfhe_hip_unpack_samples, L.tfhe_hip_unpack_samples_device):
        src = _i32p(ring) if entry is L.tfhe_hip_unpack_samples else C.c_void_p(ring.ctypes.data)
        refused(entry(ks.cloud, None, 2, None, 1, cts.ptr), "null ring words or result")
        refused(entry(ks.cloud, src, 2, None, 1, None), "null ring words or result")
        refused(entry(None, src, 2, None, 1, cts.ptr), "null cloud key")
        refused(entry(ks.cloud, src, 2, None, 0, cts.ptr), "at least 1")
        refused(entry(ks.cloud, src, 0, None, 1, cts.ptr), "at least 1")
        refused(entry(ks.cloud, src, 2, idx(0, 2 * N), 2, cts.ptr), "index 2048 at 1 is outside 0..2047")
        refused(entry(ks.cloud, src, 2, idx(-1), 1, cts.ptr), "index -1 at 0")
        refused(entry(ks.cloud, src, 1, None, N + 1, cts.ptr), "past the last coefficient")
        refused(entry(ks.cloud, src, 2, None, 5, cts.ptr), "past the end of the result array")
        refused(entry(ks.cloud, src, 2, None, 1, C.byref(foreign)), "not allocated by new_gate_bootstrapping_ciphertext_array")
        refused(entry(ks.cloud, src, 2, None, 1, other_cts.ptr), "LWE dimension")
    scattered = L.tfhe_hip_unpack_samples_scattered
    ptrs = lambda *s: (lib.LS * len(s))(*s)
    refused(scattered(ks.cloud, _i32p(ring), 2, None, 2, None), "null ring words or result")
    refused(scattered(ks.cloud, _i32p(ring), 2, None, 2, ptrs(cts.at(0), None)), "null result sample at 1")
    refused(scattered(ks.cloud, _i32p(ring), 2, None, 2, ptrs(cts.at(0), C.pointer(foreign))), "not allocated by")
    refused(scattered(ks.cloud, _i32p(ring), 2, None, 2, ptrs(cts.at(3), other_cts.at(0))), "LWE dimension")
    refused(scattered(ks.cloud, _i32p(ring), 2, idx(0, 4096), 2, ptrs(cts.at(0), cts.at(1))), "outside 0..2047")
    assert foreign.slot == 5 and not buf.any()
    raw = L.tfhe_hip_kernel_ring_extract
    refused(raw(ks.cloud, None, 2, None, 1, _i32p(u_out)), "null argument")
    refused(raw(ks.cloud, _i32p(ring), 2, None, 1, None), "null argument")
    refused(raw(None, _i32p(ring), 2, None, 1, _i32p(u_out)), "null cloud key")
    refused(raw(ks.cloud, _i32p(ring), 2, None, 0, _i32p(u_out)), "at least 1")
    refused(raw(ks.cloud, _i32p(ring), 2, idx(2 * N), 1, _i32p(u_out)), "out of range")
    # the ring encryption's own refusals: the destination untouched
    out = np.full(2 * N, 7, dtype=np.int32)
    mu, bits = np.zeros(N, dtype=np.int32), np.ones(N, dtype=np.int32)
    for call in (lambda: L.tfhe_hip_ring_encrypt(None, _i32p(mu), _i32p(out)),
                 lambda: L.tfhe_hip_ring_encrypt(ks.ptr, None, _i32p(out)),
                 lambda: L.tfhe_hip_ring_encrypt_seeded(ks.ptr, _i32p(mu), None, 1),
                 lambda: L.tfhe_hip_ring_encrypt_bits(ks.ptr, None, 3, _i32p(out)),
                 lambda: L.tfhe_hip_ring_encrypt_bits_seeded(None, _i32p(bits), 3, _i32p(out), 1)):
        assert call() == -1 and "null argument" in _err(L) and (out == 7).all()
        L.tfhe_hip_clear_error()
    for count in (0, -1, N + 1):
        assert L.tfhe_hip_ring_encrypt_bits(ks.ptr, _i32p(bits), count, _i32p(out)) == -1 and "count must be in 1..1024" in _err(L)
        assert L.tfhe_hip_ring_encrypt_bits_seeded(ks.ptr, _i32p(bits), count, _i32p(out), 1) == -1 and (out == 7).all()
        L.tfhe_hip_clear_error()
    for o in (cts, other_cts):
        o.close()


def test_the_two_new_statistics_exist_and_read_zero(L):
    """unpacked_samples and unpack_launches stand at the end of TfheHipStats, behind everything the mirror held before"""
    from peba1_amd import api, lib
    L.tfhe_hip_reset_stats()
    assert lib.UNPACK_STATS_FIELDS == ["unpacked_samples", "unpack_launches"]
    assert lib.StatsWhole.unpacked_samples.offset == C.sizeof(lib.StatsAll)
    assert lib.StatsWhole.unpack_launches.offset == C.sizeof(lib.StatsAll) + 8
    assert C.sizeof(lib.StatsWhole) == 8 * (len(lib.STATS_FIELDS) + 2)
    guard = (C.c_uint64 * (len(lib.STATS_FIELDS) + 4))(*([0x5A5A5A5A5A5A5A5A] * (len(lib.STATS_FIELDS) + 4)))
    L.tfhe_hip_get_stats(C.cast(guard, C.POINTER(lib.StatsWhole)))         # writes the whole struct and nothing behind it
    assert list(guard[-2:]) == [0x5A5A5A5A5A5A5A5A] * 2 and list(guard[-4:-2]) == [0, 0]
    assert api.unpack_stats() == {"unpacked_samples": 0, "unpack_launches": 0}
    assert list(api.stats()) == lib.STATS_FIELDS


def test_ring_encrypt_vector_lays_bit_j_of_slot_s_at_coefficient_s_bitsize_plus_j(small):
    from peba1_amd import api, circuits
    pp, ks = small
    values, bitsize = [0xA5, 0x00, 0xFF, 0x3C, 0x81], 8
    words = circuits.ring_encrypt_vector(values, bitsize, ks, seed=RING_SEED)
    bits = api.packed_decrypt(words, len(values) * bitsize, ks)
    assert [sum(int(bits[s * bitsize + j]) << j for j in range(bitsize)) for s in range(len(values))] == values
    with pytest.raises(ValueError):
        circuits.EncryptedVector.from_ring(pp, words, 129, 8, ks)          # 1,032 bits do not fit a ring of 1,024
