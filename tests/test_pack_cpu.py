"""The packing key switch without a GPU: the key object, key generation, host decryption, the error channel and the
bound check, on host-only keysets.  The numpy restatement is tests/pack_common.py."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import pack_common as K

N = 1024
N_LWE = 9                       # a small odd LWE width: the ring side is what is under test
SEED, PK_SEED = 0x9AC4, 0x51DE


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def small():
    """(parameter set, host-only keyset) of a small custom set, ks decomposition (8, 2)"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(N_LWE))
    ks = api.SecretKeySet(pp, SEED, device=False)
    yield pp, ks
    ks.close()


def _err(L):
    return L.tfhe_hip_last_error().decode()


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_key_rows_encrypt_the_stated_constants(small):
    """every row's phase under the ring key is the constant polynomial lwe_key[i] << (32 - (p+1) basebit) within
    6 bk_stdev, for the default decomposition and a non-default one"""
    from peba1_amd import api
    pp, ks = small
    for t, bb in ((0, 0), (5, 3)):
        pk = api.PackingKey(ks, t, bb, seed=PK_SEED)
        assert (pk.t, pk.basebit) == ((t, bb) if t else (pp.ks_t, pp.ks_basebit))
        rows = pk.words()
        assert rows.shape == (pp.n, pk.t, 2, N)
        ph = K.ring_phases(rows, ks.tlwe_key()).astype(np.int64)
        want = np.zeros_like(ph)
        for p in range(pk.t):
            want[:, p, 0] = K.to_i32(ks.lwe_key().astype(np.int64) << (32 - (p + 1) * pk.basebit))
        err = K.to_i32(ph - want).astype(np.float64) / 2.0 ** 32
        assert np.abs(err).max() <= 6 * K.STDEVS[1], np.abs(err).max()
        assert 0.5 * K.STDEVS[1] < err.std() < 1.5 * K.STDEVS[1]          # and it IS noise of bk_stdev, not zeros
        pk.close()


def test_seeded_keys_reproduce_and_leave_the_keyset_digests_alone(small):
    from peba1_amd import api
    pp, ks = small
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    fresh = api.SecretKeySet(pp, SEED, device=False)                       # the same keyset, never asked for a packing key
    before = {name: digest(getattr(fresh, name)()) for name in ("lwe_key", "tlwe_key", "bk", "ksk")}
    a = api.PackingKey(ks, seed=PK_SEED)
    b = api.PackingKey(ks, seed=PK_SEED)
    c = api.PackingKey(ks, seed=PK_SEED + 1)
    d = api.PackingKey(ks)                                                 # the default form: OS-keyed streams
    assert np.array_equal(a.words(), b.words())
    assert not np.array_equal(a.words(), c.words()) and not np.array_equal(a.words(), d.words())
    after = {name: digest(getattr(ks, name)()) for name in before}
    assert after == before
    again = api.SecretKeySet(pp, SEED, device=False)                       # and a keyset made after them draws the same words
    assert {name: digest(getattr(again, name)()) for name in before} == before
    for o in (a, b, c, d, fresh, again):
        o.close()


def test_from_words_reproduces_words(small):
    from peba1_amd import api
    pp, ks = small
    a = api.PackingKey(ks, 4, 4, seed=PK_SEED)
    b = api.PackingKey.from_words(pp, 4, 4, a.words())
    assert (b.t, b.basebit) == (4, 4) and np.array_equal(a.words(), b.words())
    c = api.PackingKey.from_words(pp, 0, 0, np.arange(pp.n * 8 * 2 * N, dtype=np.int32))
    assert (c.t, c.basebit) == (8, 2) and np.array_equal(c.words().reshape(-1), np.arange(pp.n * 8 * 2 * N, dtype=np.int32))
    for o in (a, b, c):
        o.close()


@pytest.mark.parametrize("count", [1, 2, 65, N])
def test_numpy_packed_words_decrypt_through_the_library(small, L, count):
    """pack in numpy from the definition, decrypt with the library's host decryption: the right bits, the phases of the
    inputs within 6 sigma of the computed variance (plus the inputs' own noise), noise only from `count` on"""
    from peba1_amd import api
    pp, ks = small
    pk = api.PackingKey(ks, seed=PK_SEED)
    rng = np.random.default_rng(count)
    bits = rng.integers(0, 2, count)
    L.tfhe_hip_set_encrypt_seed(77 + count)
    cts = api.CiphertextArray(pp, count).encrypt(bits, ks)
    words = cts.words()                                                    # host mirrors: no device involved
    in_phase = np.array([api.phase(cts.at(j), ks) for j in range(count)], dtype=np.int64)
    packed = K.pack_ref(K.KeyRows(pk.words()), words, pk.basebit)
    assert list(api.packed_decrypt(packed, count, ks)) == list(bits)
    ph = api.packed_phases(packed, ks).astype(np.int64)
    sigma = K.pack_variance(pp.n, pk.t, pk.basebit, count, K.STDEVS[1]) ** 0.5
    err = K.to_i32(ph[:count] - in_phase).astype(np.float64) / 2.0 ** 32
    assert np.abs(err).max() <= 6 * sigma, (np.abs(err).max(), sigma)
    if count < N:
        assert np.abs(ph[count:] / 2.0 ** 32).max() <= 6 * sigma
    # the library's phases are B - A S by the numpy restatement too
    assert np.array_equal(ph, K.ring_phases(packed.reshape(2, N), ks.tlwe_key()).astype(np.int64))
    pk.close()
    cts.close()


def test_refused_decompositions_and_the_frontier(small, L):
    """a key constructor takes exactly the decompositions pack_common.accepted takes (restated from the derivation), for
    the secret-side and the cloud-side constructor; a refusal returns NULL and says why"""
    from peba1_amd import api
    pp, ks = small
    assert [K.largest_t(1024, bb) for bb in (1, 2, 3, 4)] == [18, 16, 10, 8]
    assert [K.largest_t(2048, bb) for bb in (1, 2, 3, 4)] == [16, 16, 10, 8]
    words = np.zeros(pp.n * 19 * 2 * N, dtype=np.int32)
    for bb in range(0, 7):
        for t in range(0, 34):
            if t == 0 and bb == 0:
                continue                                                   # 0, 0 names the set's own decomposition
            L.tfhe_hip_clear_error()
            ptr = L.tfhe_hip_new_packing_key_from_words(pp.ptr, t, bb, _i32p(words))       # (read only if accepted: t <= 18)
            assert bool(ptr) == K.accepted(N, t, bb), (t, bb, _err(L))
            if ptr:
                L.tfhe_hip_delete_packing_key(ptr)
            else:
                assert _err(L) != ""
    for bb in (1, 2, 3, 4):                                                # the secret-side constructor at the frontier
        t = K.largest_t(N, bb)
        ptr = L.tfhe_hip_new_packing_key_seeded(ks.ptr, t, bb, 1)
        assert ptr and not L.tfhe_hip_new_packing_key_seeded(ks.ptr, t + 1, bb, 1)
        L.tfhe_hip_delete_packing_key(ptr)
    L.tfhe_hip_clear_error()
    assert not L.tfhe_hip_new_packing_key_from_words(pp.ptr, 19, 1, _i32p(words)) and "MAC bound" in _err(L)
    assert not L.tfhe_hip_new_packing_key_from_words(pp.ptr, 2, 5, _i32p(words)) and "1..4 bits" in _err(L)
    assert not L.tfhe_hip_new_packing_key_from_words(pp.ptr, 9, 4, _i32p(words)) and "t * basebit <= 32" in _err(L)
    assert not L.tfhe_hip_new_packing_key_from_words(None, 8, 2, _i32p(words))
    assert not L.tfhe_hip_new_packing_key_from_words(pp.ptr, 8, 2, None)
    assert not L.tfhe_hip_new_packing_key(None, 8, 2) and "null secret keyset" in _err(L)


def test_bound_check_frontier_matches_an_independent_evaluation(L):
    """tfhe_hip_test_pack_bounds against pack_common.mac_ok / crt_ok over every chunk size near either frontier"""
    for n_ring in (1024, 2048):
        mac_frontier = max(r for r in range(1, 64) if K.mac_ok(n_ring, r))
        assert mac_frontier == {1024: 18, 2048: 16}[n_ring]
        for bb in (1, 2, 3, 4):
            crt_frontier = ((K.P0 * K.P1 // 100) * 36 - 1) // (n_ring * (2 ** bb - 1) * 2 ** 31)
            assert K.crt_ok(n_ring, crt_frontier, bb) and not K.crt_ok(n_ring, crt_frontier + 1, bb)
            rows = sorted(set(list(range(1, 40)) + [crt_frontier + d for d in range(-3, 4)] + [5040, 1 << 20]))
            for r in rows:
                got = L.tfhe_hip_test_pack_bounds(n_ring, r, bb)
                assert got == (0 if K.mac_ok(n_ring, r) else 1) | (0 if K.crt_ok(n_ring, r, bb) else 2), (n_ring, r, bb, got)
            # one mask index always holds; all rows of P128 in one chunk would wrap (2^54.9 at base 4)
            assert all(K.crt_ok(n_ring, t, bb) for t in range(1, 33))
    assert not K.crt_ok(1024, 630 * 8, 2)
    assert L.tfhe_hip_test_pack_bounds(512, 8, 2) == -1 and L.tfhe_hip_test_pack_bounds(1024, 8, 5) == -1
    assert L.tfhe_hip_test_pack_bounds(1024, 0, 2) == -1


def test_pack_errors_are_reported_and_leave_the_call_without_effect(small, L):
    """every refusal of tfhe_hip_pack_samples / _device / tfhe_hip_kernel_pack / the decryptions: -1, a message, the
    destination untouched -- all decided before the device is looked at (this test runs without one)"""
    from peba1_amd import api, lib
    pp, ks = small
    pk = api.PackingKey(ks, seed=PK_SEED)
    cts = api.CiphertextArray(pp, 4)
    out = np.full(2 * N, 7, dtype=np.int32)
    other_pp = api.ParameterSet(custom=K.custom_tuple(N_LWE + 2))
    other_ks = api.SecretKeySet(other_pp, SEED, device=False)
    other_cts = api.CiphertextArray(other_pp, 4)
    buf = np.zeros(pp.n + 16, dtype=np.int32)
    foreign = lib.LweSample()
    foreign.a = C.cast(buf.ctypes.data + 8 * 4, C.POINTER(C.c_int32))
    foreign.slot = 5

    def refused(rc, needle):
        assert rc == -1 and needle in _err(L), (rc, needle, _err(L))
        assert (out == 7).all()
        L.tfhe_hip_clear_error()

    for entry in (L.tfhe_hip_pack_samples, L.tfhe_hip_pack_samples_device):
        dst = _i32p(out) if entry is L.tfhe_hip_pack_samples else C.c_void_p(out.ctypes.data)
        refused(entry(pk.ptr, cts.ptr, 0, ks.cloud, dst), "count must be in 1..1024")
        refused(entry(pk.ptr, cts.ptr, N + 1, ks.cloud, dst), "count must be in 1..1024")
        refused(entry(pk.ptr, cts.ptr, 5, ks.cloud, dst), "past the end")
        refused(entry(None, cts.ptr, 1, ks.cloud, dst), "null or deleted packing key")
        refused(entry(pk.ptr, None, 1, ks.cloud, dst), "null samples")
        refused(entry(pk.ptr, cts.ptr, 1, None, dst), "null cloud key")
        refused(entry(pk.ptr, cts.ptr, 1, ks.cloud, None), "null samples or destination")
        refused(entry(pk.ptr, C.byref(foreign), 1, ks.cloud, dst), "not allocated by new_gate_bootstrapping_ciphertext_array")
        refused(entry(pk.ptr, other_cts.ptr, 1, ks.cloud, dst), "LWE dimension")
        refused(entry(pk.ptr, cts.ptr, 1, other_ks.cloud, dst), "another parameter set")
    assert foreign.slot == 5 and not buf.any()
    sw = np.zeros((2, pp.words), dtype=np.int32)
    refused(L.tfhe_hip_kernel_pack(pk.ptr, ks.cloud, _i32p(sw), 0, 0, _i32p(out)), "count must be in 1..N")
    refused(L.tfhe_hip_kernel_pack(pk.ptr, other_ks.cloud, _i32p(sw), 2, 0, _i32p(out)), "another parameter set")
    refused(L.tfhe_hip_kernel_pack(pk.ptr, ks.cloud, None, 2, 0, _i32p(out)), "null argument")
    refused(L.tfhe_hip_kernel_pack(None, ks.cloud, _i32p(sw), 2, 0, _i32p(out)), "null or deleted packing key")
    bits = np.full(4, 7, dtype=np.int32)
    assert L.tfhe_hip_packed_decrypt_bits(ks.ptr, _i32p(out), 0, _i32p(bits)) == -1 and "count must be in 1..1024" in _err(L)
    assert L.tfhe_hip_packed_decrypt_bits(ks.ptr, _i32p(out), N + 1, _i32p(bits)) == -1 and (bits == 7).all()
    assert L.tfhe_hip_packed_decrypt_bits(None, _i32p(out), 1, _i32p(bits)) == -1
    assert L.tfhe_hip_packed_phase(ks.ptr, None, _i32p(out)) == -1 and (out == 7).all()
    cnt = C.c_int64(5)
    assert not L.tfhe_hip_packing_key_words(None, C.byref(cnt)) and cnt.value == 0
    L.tfhe_hip_clear_error()
    for o in (pk, cts, other_cts, other_ks):
        o.close()


def test_identify_helper_packs_in_ring_sized_pieces(small, monkeypatch):
    """identify.pack_match_bits cuts the match bits into pieces of N and packs each (api.pack stubbed: no device here)"""
    from peba1_amd import api, identify
    pp, ks = small
    calls = []
    monkeypatch.setattr(api, "pack", lambda pkey, samples, count, key, first=0: calls.append((first, count)) or np.zeros(2 * N, np.int32))
    pk = api.PackingKey(ks, seed=PK_SEED)
    bits = api.CiphertextArray(pp, N + 3)
    got = identify.pack_match_bits(pk, bits, ks)
    assert calls == [(0, N), (N, 3)] and [c for _, c in got] == [N, 3]
    pk.close()
    bits.close()
