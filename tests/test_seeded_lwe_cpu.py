"""Seed-compressed LWE sample arrays without a GPU: the fixture encryptors and the host expansion against the numpy
restatement of tests/seeded_lwe_common.py, the default encryptors by what they must mean (fresh seeds, right bits, the set's
noise), every refusal of the host entries and of the seeded import before the device is looked at, and the sizes of the
statistics structs.  Every word comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import seeded_lwe_common as S

GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


_SETS = {}


def host_set(n):
    """one host-only keyset per LWE dimension; 630 is the product's own set"""
    from peba1_amd import api
    if n not in _SETS:
        pp = api.ParameterSet(128) if n == 630 else api.ParameterSet(custom=S.custom_tuple(n))
        _SETS[n] = (pp, api.SecretKeySet(pp, 0x1E5 + n, device=False))
    assert _SETS[n][0].n == n
    return _SETS[n]


@pytest.fixture(scope="module", autouse=True)
def close_sets():
    yield
    for _, sk in _SETS.values():
        sk.close()
    _SETS.clear()


# ---- the fixture form ----
@pytest.mark.parametrize("n", [1, 7, 8, 9, 10, 630])
def test_fixture_form_against_the_restatement(L, oracle, n):
    """seed words verbatim in front; body - <a, s> - mu is the fixture noise exactly, a the stream words j n .. of the
    restatement, the inner product wrapping in uint32; both the torus and the bits form"""
    from peba1_amd import api
    pp, sk = host_set(n)
    rng = np.random.default_rng(n)
    count = 19
    mu = rng.integers(-2 ** 31, 2 ** 31, count, dtype=np.int64).astype(np.int32)
    bits = rng.integers(0, 2, count).astype(np.int32)
    noise = S.fixture_noise(oracle, S.NOISE_SEED, S.KS_STDEV, count)
    assert np.abs(noise).max() > 0
    key = np.array(sk.lwe_key())
    for rec, msg in ((api.encrypt_torus_compressed(mu, sk, seed=S.NOISE_SEED, mask_seed=S.MASK_SEED), mu),
                     (api.encrypt_bits_compressed(bits, sk, seed=S.NOISE_SEED, mask_seed=S.MASK_SEED),
                      np.where(bits == 1, 2 ** 29, -2 ** 29).astype(np.int32))):
        assert rec.shape == (10 + count,) and rec.dtype == np.int32
        S.assert_words(rec[:10].view(np.uint32), S.MASK_SEED, "seed words")
        plain = S.expand_ref(L, rec, n, np.arange(count))
        with np.errstate(over="ignore"):
            got = (S.phases(plain, key).view(np.uint32) - msg.view(np.uint32)).view(np.int32)
        S.assert_words(got, noise, ("fixture noise", n))
    S.assert_words(api.encrypt_bits_compressed(bits, sk, seed=S.NOISE_SEED, mask_seed=S.MASK_SEED), rec, "reproducible")


# ---- the host expansion ----
@pytest.mark.parametrize("n,record_count", [(1, 5), (7, 3), (8, 4), (9, 11), (10, 33), (630, 9)])
def test_expand_host_against_the_restatement(L, n, record_count):
    """the identity (index NULL and given), a reversed index, repeats, the first sample and the last alone: the stream's
    final block is only partly used when record_count n is no multiple of 8"""
    from peba1_amd import api
    rng = np.random.default_rng(100 + n)
    rec = S.random_record(rng, record_count)
    ident = np.arange(record_count)
    want = S.expand_ref(L, rec, n, ident)
    S.assert_words(want[:, n], rec[10:], "bodies")
    S.assert_words(api.lwe_expand(rec, n), want, "index NULL, the whole record")
    S.assert_words(api.lwe_expand(rec, n, count=min(2, record_count)), want[:2], "index NULL, a prefix")
    S.assert_words(api.lwe_expand(rec, n, index=ident), want, "identity")
    S.assert_words(api.lwe_expand(rec, n, index=ident[::-1]), want[::-1], "reversed")
    rep = np.array([record_count - 1, 0, 0, record_count - 1, record_count // 2, 0])
    S.assert_words(api.lwe_expand(rec, n, index=rep), want[rep], "repeats")
    S.assert_words(api.lwe_expand(rec, n, index=[0]), want[:1], "first alone")
    S.assert_words(api.lwe_expand(rec, n, index=[record_count - 1]), want[-1:], "last alone")


def test_expand_host_last_sample_of_the_largest_record(L):
    """2^20 samples at n = 1,024: the last sample alone, stream words 2^30 - 1,024 .. 2^30 - 1"""
    from peba1_amd import api
    rec = np.zeros(10 + S.RECORD_MAX, dtype=np.int32)
    rec[:10] = S.MASK_SEED.view(np.int32)
    rec[-1], rec[-2] = 0x1234567, -5
    got = api.lwe_expand(rec, 1024, index=[S.RECORD_MAX - 1])
    want = S.expand_ref(L, rec, 1024, [S.RECORD_MAX - 1])
    assert want[0, 1024] == 0x1234567
    S.assert_words(got, want, "last sample of 2^20")


# ---- the default encryptors ----
def test_default_encryptors_draw_fresh_seeds_and_the_sets_noise(L):
    """two calls give different seeds; 4,096 bits at P128 all decrypt through lwe_expand and the phase under the secret
    key; the sample deviation of the noise lies within 10 % of ks_stdev (standard error at 4,096 samples: 1.1 %)"""
    from peba1_amd import api
    pp, sk = host_set(630)
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, 4096).astype(np.int32)
    rec, rec2 = api.encrypt_bits_compressed(bits, sk), api.encrypt_bits_compressed(bits, sk)
    assert rec.nbytes == 40 + 4 * 4096
    assert (rec[:10] != rec2[:10]).any() and (rec[10:] != rec2[10:]).any()
    key = np.array(sk.lwe_key())
    ph = S.phases(api.lwe_expand(rec, pp.n), key)
    assert ((ph > 0).astype(np.int32) == bits).all()
    noise = ph.astype(np.int64) - np.where(bits == 1, 2 ** 29, -2 ** 29)
    sigma = S.KS_STDEV * 2.0 ** 32
    dev = float(np.sqrt(np.mean(noise.astype(np.float64) ** 2)))
    print("noise deviation", dev, "of", sigma)
    assert 0.9 * sigma <= dev <= 1.1 * sigma, (dev, sigma)
    assert abs(float(noise.mean())) < 5 * sigma / 64                    # 5 standard errors of the mean
    mu = rng.integers(-2 ** 31, 2 ** 31, 64, dtype=np.int64).astype(np.int32)
    t1, t2 = api.encrypt_torus_compressed(mu, sk), api.encrypt_torus_compressed(mu, sk)
    assert (t1[:10] != t2[:10]).any()
    err = S.centred(S.phases(api.lwe_expand(t1, pp.n), key).astype(np.int64) - mu)
    assert np.abs(err).max() <= 6 * sigma and np.abs(err).max() > 0


# ---- refusals ----
def _refused(L, rc, needle):
    from peba1_amd import api
    msg = api.last_error()
    assert rc == -1 and needle in msg, (rc, msg, needle)
    L.tfhe_hip_clear_error()


def test_host_entries_refuse_without_effect(L):
    from peba1_amd import lib
    pp, sk = host_set(10)
    I, U = lib.I32P, lib.U32P
    bits = np.ones(4, dtype=np.int32)
    out = np.full(10 + 4, 77, dtype=np.int32)
    seed = S.MASK_SEED.ctypes.data_as(U)
    bp, op = bits.ctypes.data_as(I), out.ctypes.data_as(I)
    L.tfhe_hip_clear_error()
    for plain, fixture in ((L.tfhe_hip_sym_encrypt_bits_compressed, L.tfhe_hip_sym_encrypt_bits_compressed_seeded),
                           (L.tfhe_hip_sym_encrypt_torus_compressed, L.tfhe_hip_sym_encrypt_torus_compressed_seeded)):
        _refused(L, plain(None, bp, 4, op), "null")
        _refused(L, plain(sk.ptr, None, 4, op), "null")
        _refused(L, plain(sk.ptr, bp, 4, None), "null")
        _refused(L, plain(sk.ptr, bp, 0, op), "1..1048576")
        _refused(L, plain(sk.ptr, bp, -3, op), "1..1048576")
        _refused(L, plain(sk.ptr, bp, S.RECORD_MAX + 1, op), "1..1048576")
        _refused(L, fixture(sk.ptr, bp, 4, op, None, 1), "null")
        _refused(L, fixture(sk.ptr, None, 4, op, seed, 1), "null")
        _refused(L, fixture(sk.ptr, bp, 0, op, seed, 1), "1..1048576")
        assert (out == 77).all()
    rec = S.random_record(np.random.default_rng(1), 6)
    rp = rec.ctypes.data_as(I)
    rows = np.full((3, 11), 77, dtype=np.int32)
    wp = rows.ctypes.data_as(I)

    def idx(*v):
        return np.array(v, dtype=np.int32).ctypes.data_as(I)

    ex = L.tfhe_hip_lwe_expand_host
    _refused(L, ex(None, 10, 6, None, 3, wp), "null")
    _refused(L, ex(rp, 10, 6, None, 3, None), "null")
    _refused(L, ex(rp, 10, 6, None, 0, wp), "count must be at least 1")
    _refused(L, ex(rp, 10, 0, None, 3, wp), "1..1048576")
    _refused(L, ex(rp, 10, S.RECORD_MAX + 1, None, 3, wp), "1..1048576")
    _refused(L, ex(rp, 10, 2, None, 3, wp), "past the last sample")
    _refused(L, ex(rp, 10, 6, idx(0, 6, 1), 3, wp), "index 6 at 1 is outside 0..5")
    _refused(L, ex(rp, 10, 6, idx(0, 1, -1), 3, wp), "index -1 at 2")
    _refused(L, ex(rp, 0, 6, None, 3, wp), "LWE dimension")
    _refused(L, ex(rp, 1025, 6, None, 3, wp), "LWE dimension")
    assert (rows == 77).all()
    assert ex(rp, 10, 6, idx(5, 0, 5), 3, wp) == 0 and not (rows == 77).all()


def test_seeded_import_refuses_before_the_device_is_looked_at(L):
    """every refusal of the import entries happens on a machine without a GPU: the results keep their words, nothing is
    counted, and the raw kernel entry refuses the same arguments"""
    from peba1_amd import api, lib
    pp, sk = host_set(10)
    other, _ = host_set(7)
    I = lib.I32P
    rec = S.random_record(np.random.default_rng(2), 6)
    rp = rec.ctypes.data_as(I)
    arr, small = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], sk), api.CiphertextArray(other, 4)
    held = arr.words().copy()

    def idx(*v):
        return np.array(v, dtype=np.int32).ctypes.data_as(I)

    ptrs = (lib.LS * 4)(*[arr.at(j) for j in range(4)])
    holes = (lib.LS * 4)(arr.at(0), None, arr.at(2), arr.at(3))
    foreign = (lib.LweSample * 1)()
    imp, sca, dev = L.tfhe_hip_import_samples_seeded, L.tfhe_hip_import_samples_seeded_scattered, L.tfhe_hip_import_samples_seeded_device
    L.tfhe_hip_clear_error()
    _refused(L, imp(pp.ptr, None, 6, None, 4, arr.ptr), "null")
    _refused(L, imp(pp.ptr, rp, 6, None, 4, None), "null")
    _refused(L, imp(None, rp, 6, None, 4, arr.ptr), "null parameter set")
    _refused(L, imp(pp.ptr, rp, 6, None, 0, arr.ptr), "count must be at least 1")
    _refused(L, imp(pp.ptr, rp, 0, None, 4, arr.ptr), "1..1048576")
    _refused(L, imp(pp.ptr, rp, S.RECORD_MAX + 1, None, 4, arr.ptr), "1..1048576")
    _refused(L, imp(pp.ptr, rp, 3, None, 4, arr.ptr), "past the last sample")
    _refused(L, imp(pp.ptr, rp, 6, idx(0, 1, 6, 2), 4, arr.ptr), "index 6 at 2 is outside 0..5")
    _refused(L, imp(pp.ptr, rp, 6, idx(0, 1, 2, 3, 4), 5, arr.ptr), "past the end of the result array")
    _refused(L, imp(pp.ptr, rp, 6, None, 4, small.ptr), "LWE dimension 7")
    _refused(L, imp(pp.ptr, rp, 6, None, 1, C.cast(foreign, lib.LS)), "not allocated")
    _refused(L, sca(pp.ptr, rp, 6, None, 4, None), "null")
    _refused(L, sca(pp.ptr, rp, 6, None, 4, holes), "null result sample at 1")
    _refused(L, sca(pp.ptr, rp, 6, idx(0, 0, 0, -1), 4, ptrs), "index -1 at 3")
    _refused(L, dev(pp.ptr, None, 6, None, 4, arr.ptr), "null")
    _refused(L, dev(pp.ptr, C.c_void_p(0x1000), 6, idx(9), 1, arr.ptr), "index 9 at 0")
    out = np.full((4, 11), 77, dtype=np.int32)
    ker = L.tfhe_hip_kernel_lwe_expand
    _refused(L, ker(pp.ptr, None, 6, None, 4, out.ctypes.data_as(I)), "null")
    _refused(L, ker(pp.ptr, rp, 6, None, 7, out.ctypes.data_as(I)), "past the last sample")
    _refused(L, ker(None, rp, 6, None, 4, out.ctypes.data_as(I)), "null parameter set")
    assert L.tfhe_hip_test_expand_slots(None, -1) == -1
    L.tfhe_hip_clear_error()
    assert L.tfhe_hip_test_expand_slots(None, 0) == 0                   # nothing was ever launched
    assert (out == 77).all()
    S.assert_words(arr.words(), held, "results after the refusals")
    assert arr.decrypt(sk).tolist() == [1, 0, 1, 1]
    assert api.seeded_lwe_stats() == {"seeded_imported_samples": 0, "seeded_import_launches": 0}
    arr.close()
    small.close()


def test_statistics_structs_keep_their_sizes(L):
    """the counters are a struct of their own: TfheHipStats, TfheHipExpandStats and TfheHipSeededStats are filled whole by
    their entries and have not grown; the new entry writes its two words and nothing behind them"""
    from peba1_amd import lib
    assert C.sizeof(lib.StatsWhole) == 8 * (len(lib.STATS_FIELDS) + 2) == 8 * 35
    assert C.sizeof(lib.ExpandStats) == 16 and C.sizeof(lib.SeededStats) == 32 and C.sizeof(lib.SeededLweStats) == 16
    assert lib.SEEDED_LWE_STATS_FIELDS == ["seeded_imported_samples", "seeded_import_launches"]
    L.tfhe_hip_reset_stats()
    for entry, struct in ((L.tfhe_hip_get_stats, lib.StatsWhole), (L.tfhe_hip_get_expand_stats, lib.ExpandStats),
                          (L.tfhe_hip_get_seeded_stats, lib.SeededStats), (L.tfhe_hip_get_seeded_lwe_stats, lib.SeededLweStats)):
        words = C.sizeof(struct) // 8
        guard = (C.c_uint64 * (words + 2))(*([GUARD] * (words + 2)))
        entry(C.cast(guard, C.POINTER(struct)))
        assert list(guard[words:]) == [GUARD] * 2, struct.__name__
        assert list(guard[:words]) == [0] * words, struct.__name__
    L.tfhe_hip_get_seeded_lwe_stats(None)                               # a no-op
