"""Seed-compressed cloud keys on the host (include/tfhe_hip.h): the mask stream against the definition, the rule that a
mask carries nothing but stream words, what the rows mean (restated in numpy), the word-level contracts, the file form and
the CPU oracle under a host-expanded key.  Every comparison is exact; the only bound is the noise bound of the independent
key test of tests/test_host_cpu.py for the same deviations."""
import ctypes as C
import resource
import struct
import time

import numpy as np
import pytest

import compressed_common as K


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


def _params(n, ks=(8, 2), gadget=(2, 10), N=1024):
    from peba1_amd import api
    return api.ParameterSet(custom=K.custom_tuple(n, N=N, ks=ks, gadget=gadget))


def _compressed(pp, key_seed=21, noise_seed=K.NOISE_SEED, mask_seed=K.MASK_SEED):
    from peba1_amd import api
    sk = api.SecretKeySet(pp, key_seed, device=False)
    return sk, api.CompressedCloudKey.generate_seeded(sk, noise_seed, mask_seed)


@pytest.fixture(scope="module")
def small16():
    """n = 16, N = 1,024, l = 2, (8, 2): secret keyset, compressed key, host-expanded keyset"""
    pp = _params(16)
    sk, ck = _compressed(pp)
    host = ck.expand_host()
    yield pp, sk, ck, host
    host.close()
    ck.close()
    sk.close()


# ---- the stream ----
@pytest.mark.parametrize("ks", [(8, 2), (2, 4)])
def test_host_expanded_masks_are_the_stream_words(L, ks):
    """n = 10, N = 1,024: EVERY mask word of the expanded key is word 2 (m mod 8) + 1 of block floor(m / 8), the BK's masks
    first, then the KSK's -- the first and last word of each, and every KSK row (10 words, so four rows in five straddle
    a block) among them; the bodies are the transmitted words and the digit-0 rows are zero"""
    pp = _params(10, ks=ks)
    sk, ck = _compressed(pp)
    host = ck.expand_host()
    try:
        sh = K.Shape(pp)
        bk, ksk = host.bk().view(np.uint32), host.ksk().view(np.uint32)
        assert bk.size == sh.bk_words and ksk.size == sh.ksk_words
        stream = K.stream_words(L, K.MASK_SEED, 0, sh.bk_masks + sh.ksk_masks)
        m = np.arange(sh.bk_masks)
        poly, j = np.divmod(m, sh.N)
        row, u = np.divmod(poly, sh.k)
        assert np.array_equal(bk[(row * (sh.k + 1) + u) * sh.N + j], stream[:sh.bk_masks])
        assert bk[sh.bk_mask_index(0)] == stream[0] and bk[sh.bk_mask_index(sh.bk_masks - 1)] == stream[sh.bk_masks - 1]
        m = np.arange(sh.ksk_masks)
        crow, q = np.divmod(m, sh.n)
        r, v1 = np.divmod(crow, sh.base - 1)
        assert np.array_equal(ksk[(r * sh.base + v1 + 1) * (sh.n + 1) + q], stream[sh.bk_masks:])
        assert ksk[sh.ksk_mask_index(0)] == stream[sh.bk_masks] and ksk[sh.ksk_mask_index(sh.ksk_masks - 1)] == stream[-1]
        B = host.bk().reshape(sh.n * sh.kpl, sh.k + 1, sh.N)
        assert np.array_equal(B[:, sh.k, :].reshape(-1), ck.bk_body())
        Kk = host.ksk().reshape(-1, sh.base, sh.n + 1)
        assert np.array_equal(Kk[:, 1:, sh.n].reshape(-1), ck.ksk_body()) and not Kk[:, 0, :].any()
    finally:
        host.close()
        ck.close()
        sk.close()


# ---- the trap ----
def test_two_secrets_under_one_seed_share_every_mask_word(small16):
    """a mask that comes from a public seed is the stream and nothing else: under another secret the expanded key has the
    same mask words everywhere, the rows with bloc < k included, and only bodies differ"""
    pp, sk, ck, host = small16
    sh = K.Shape(pp)
    sk2, ck2 = _compressed(pp, key_seed=22)
    host2 = ck2.expand_host()
    try:
        assert not np.array_equal(sk.lwe_key(), sk2.lwe_key())
        a = host.bk().reshape(sh.n * sh.kpl, sh.k + 1, sh.N)
        b = host2.bk().reshape(sh.n * sh.kpl, sh.k + 1, sh.N)
        assert np.array_equal(a[:, :sh.k, :], b[:, :sh.k, :])
        assert (a[:, sh.k, :] != b[:, sh.k, :]).any(axis=1).all()          # every body polynomial differs
        ka, kb = host.ksk().reshape(-1, sh.n + 1), host2.ksk().reshape(-1, sh.n + 1)
        assert np.array_equal(ka[:, :sh.n], kb[:, :sh.n]) and not np.array_equal(ka[:, sh.n], kb[:, sh.n])
    finally:
        host2.close()
        ck2.close()
        sk2.close()


# ---- what the rows mean ----
def test_rows_are_tgsw_and_lwe_samples_under_the_secret(small16):
    """every BK row's phase body - sum_u mask_u S_u is noise plus the gadget term -- on body coefficient 0 for bloc = k, as
    -mu S_bloc(X) otherwise; every KSK row is an LWE sample of v S_i / base^(j+1).  Bounds: 8 sigma of bk_stdev = 2^-25 and
    8 * 2^17 for ks_stdev = 2^-15, as the independent key test uses for these deviations"""
    pp, sk, ck, host = small16
    sh = K.Shape(pp)
    s = np.asarray(sk.lwe_key(), dtype=np.int64)
    S = np.asarray(sk.tlwe_key(), dtype=np.int64).reshape(sh.k, sh.N)
    rows = host.bk().astype(np.int64).reshape(sh.n, sh.kpl, sh.k + 1, sh.N) % (1 << 32)
    worst = 0
    for i in range(sh.n):
        for row in range(sh.kpl):
            bloc, j = divmod(row, sh.l)
            phase = rows[i, row, sh.k].copy()
            for u in range(sh.k):
                phase -= K.negacyclic_by_bits(rows[i, row, u], S[u])
            g = int(s[i]) << (32 - (j + 1) * pp.Bgbit)
            if bloc == sh.k:
                phase[0] -= g
            else:
                phase += g * S[bloc]
            worst = max(worst, int(np.abs(K.centred(phase)).max()))
    assert 0 < worst < 8 * 2.0 ** 7, worst
    Kk = host.ksk().astype(np.int64).reshape(sh.k * sh.N, sh.t, sh.base, sh.n + 1) % (1 << 32)
    ph = Kk[:, :, 1:, sh.n] - (Kk[:, :, 1:, :sh.n] * s).sum(axis=-1)
    jj = np.arange(sh.t).reshape(1, sh.t, 1)
    vv = np.arange(1, sh.base).reshape(1, 1, sh.base - 1)
    want = (S.reshape(-1, 1, 1) * vv) << (32 - (jj + 1) * sh.bb)
    err = np.abs(K.centred(ph - want))
    assert err.max() < 8 * 2.0 ** 17 and err.std() > 2.0 ** 14, (int(err.max()), float(err.std()))


# ---- word-level contracts ----
def test_seeded_generation_from_words_and_sizes(small16):
    from peba1_amd import api
    pp, sk, ck, host = small16
    sh = K.Shape(pp)
    again = api.CompressedCloudKey.generate_seeded(sk, K.NOISE_SEED, K.MASK_SEED)
    other = api.CompressedCloudKey.generate_seeded(sk, K.NOISE_SEED + 1, K.MASK_SEED)
    copy = api.CompressedCloudKey.from_words(pp, ck.seed(), ck.bk_body(), ck.ksk_body())
    fresh = api.CompressedCloudKey.generate(sk)
    try:
        assert np.array_equal(again.bk_body(), ck.bk_body()) and np.array_equal(again.ksk_body(), ck.ksk_body())
        assert not np.array_equal(other.bk_body(), ck.bk_body())
        assert np.array_equal(copy.seed(), K.MASK_SEED) and np.array_equal(copy.bk_body(), ck.bk_body())
        assert np.array_equal(copy.ksk_body(), ck.ksk_body())
        assert ck.bk_body().size == sh.bk_body_words == sh.n * (sh.k + 1) * sh.l * sh.N
        assert ck.ksk_body().size == sh.ksk_body_words == sh.k * sh.N * sh.t * (sh.base - 1)
        assert ck.nbytes == 40 + 4 * (sh.bk_body_words + sh.ksk_body_words) == copy.nbytes == fresh.nbytes
        assert not np.array_equal(fresh.seed(), K.MASK_SEED) and fresh.seed().any()
    finally:
        for k in (again, other, copy, fresh):
            k.close()


def test_p128_sizes(tmp_path):
    """the product's set: n (k+1) l N + kN t (base-1) body words and 40 bytes of seed travel; the file adds the 24-byte
    header and the 56-byte parameter record"""
    from peba1_amd import api
    pp = api.ParameterSet(128)
    sk, ck = _compressed(pp)
    try:
        sh = K.Shape(pp)
        assert (sh.bk_body_words, sh.ksk_body_words) == (630 * 2 * pp.l * 1024, 24576)
        assert ck.nbytes == 40 + 4 * (sh.bk_body_words + sh.ksk_body_words)
        assert 4 * (sh.bk_words + sh.ksk_words) > 7 * ck.nbytes
        ck.save(tmp_path / "c.key")
        assert (tmp_path / "c.key").stat().st_size == 24 + 56 + ck.nbytes
    finally:
        ck.close()
        sk.close()


def test_expand_host_survives_the_cloud_file(small16, tmp_path):
    """expand_host, the existing cloud-key export and load: the same words; a device-expanded keyset exports them too
    (its host words are made on demand, no GPU involved)"""
    from peba1_amd import api
    pp, sk, ck, host = small16
    host.save(tmp_path / "host.key")
    lazy = ck.expand()
    lazy.save(tmp_path / "lazy.key")
    back = api.CloudKeySet.load(tmp_path / "host.key")
    try:
        assert np.array_equal(back.bk(), host.bk()) and np.array_equal(back.ksk(), host.ksk())
        assert (tmp_path / "lazy.key").read_bytes() == (tmp_path / "host.key").read_bytes()
        assert np.array_equal(lazy.bk(), host.bk()) and np.array_equal(lazy.ksk(), host.ksk())
    finally:
        back.close()
        lazy.close()


# ---- files ----
def test_file_round_trip_and_hostile_files(small16, tmp_path):
    from peba1_amd import api
    pp, sk, ck, host = small16
    ck.save(tmp_path / "c.key")
    blob = (tmp_path / "c.key").read_bytes()
    assert len(blob) == 24 + 56 + ck.nbytes and blob[:4] == b"TFHP"
    back = api.CompressedCloudKey.load(tmp_path / "c.key")
    assert np.array_equal(back.seed(), ck.seed()) and np.array_equal(back.bk_body(), ck.bk_body())
    assert np.array_equal(back.ksk_body(), ck.ksk_body())
    again = back.expand_host()
    assert np.array_equal(again.bk(), host.bk()) and again.params.n == pp.n
    again.close()
    back.close()
    hdr, rec = blob[:24], blob[24:80]
    fields = list(struct.unpack("<8i", rec[:32]))

    def record(**kw):
        v = dict(zip(("n", "N", "k", "l", "Bgbit", "ks_t", "ks_basebit", "pad"), fields))
        v.update(kw)
        return struct.pack("<8i", *v.values()) + rec[32:]

    big = 56 + 40 + 4 * (1024 * 8 * 2048 + 2048 * 8 * 3)                  # n = 1,024, N = 2,048, l = 4: 64 MiB of bodies
    host.save(tmp_path / "plain.key")
    cases = {
        "magic": (b"XFHP" + blob[4:], "not a libtfhe-hip file"),
        "version": (blob[:4] + struct.pack("<I", 2) + blob[8:], "unsupported file version"),
        "kind": ((tmp_path / "plain.key").read_bytes(), "expected 5"),
        "size": (hdr + record(n=1024, N=2048, l=4, Bgbit=8) + blob[80:200], "payload size does not match"),
        "forged": (hdr[:16] + struct.pack("<Q", big) + record(n=1024, N=2048, l=4, Bgbit=8) + blob[80:200], "short read"),
        "truncated": (blob[:len(blob) // 2], "short read"),
        "shape": (hdr + record(N=4096) + blob[80:200], "unsupported parameter set in file"),
    }
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for name, (data, needle) in cases.items():
        (tmp_path / name).write_bytes(data)
        t = time.time()
        with pytest.raises(ValueError, match=needle):
            api.CompressedCloudKey.load(tmp_path / name)
        assert time.time() - t < 5.0, name
    # nothing of the declared 64 MiB was allocated: reads go in 16 MiB chunks and stop at the file's real end
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - peak < 40 * 1024
    with pytest.raises(ValueError, match="expected 2"):
        api.CloudKeySet.load(tmp_path / "c.key")
    ok = api.CompressedCloudKey.load(tmp_path / "c.key")                   # still alive and working
    ok.close()


def test_refused_parameter_sets_and_null_arguments(L):
    """a set the kernels cannot run is refused with the message of a refused keyset"""
    from peba1_amd import api, lib
    pp = api.ParameterSet(custom=K.custom_tuple(16, gadget=(8, 4), N=2048))
    sk = api.SecretKeySet(pp, 3, device=False)
    with pytest.raises(RuntimeError, match="every blind-rotate kernel form"):
        api.CompressedCloudKey.generate_seeded(sk, 1, K.MASK_SEED)
    with pytest.raises(RuntimeError, match="every blind-rotate kernel form"):
        api.CompressedCloudKey.generate(sk)
    sk.close()
    assert not L.tfhe_hip_new_compressed_cloud_key(None) and b"null secret keyset" in L.tfhe_hip_last_error()
    assert not L.tfhe_hip_expand_cloud_key(None) and not L.tfhe_hip_expand_cloud_key_host(None)
    assert L.tfhe_hip_compressed_key_bytes(None) == -1


def test_expand_counters_read_zero_without_a_device(L):
    from peba1_amd import api, lib
    L.tfhe_hip_reset_stats()
    assert lib.EXPAND_STATS_FIELDS == ["expanded_keys", "expand_launches"]
    assert api.expand_stats() == {"expanded_keys": 0, "expand_launches": 0}
    assert "expanded_keys" not in lib.STATS_FIELDS and list(api.stats()) == lib.STATS_FIELDS


# ---- the oracle under a host-expanded key ----
def test_oracle_decrypts_gates_under_the_expanded_words(small16, oracle):
    """the CPU oracle, its key words replaced by the host-expanded ones and its secret by the product's (schoolbook
    evaluator: the oracle's transformed images belong to the key it generated), decrypts the truth tables of AND and MUX"""
    pp, sk, ck, host = small16
    oks = oracle.KeySet(oracle.custom_params(n=pp.n, N=pp.N, l=pp.l, Bgbit=pp.Bgbit, ks_t=pp.ks_t, ks_basebit=pp.ks_basebit), 1)
    oks.bk()[:] = host.bk()
    oks.ksk()[:] = host.ksk()
    oks.lwe_key()[:] = sk.lwe_key()
    oks.tlwe_key()[:] = sk.tlwe_key()
    rng = oracle.Rng(5)
    enc = {b: oks.encrypt(rng, [b])[0] for b in (0, 1)}
    for a in (0, 1):
        for b in (0, 1):
            assert oks.decrypt(oks.gate("AND", enc[a], enc[b], use_ntt=False))[0] == (a & b)
            for c in (0, 1):
                assert oks.decrypt(oks.mux(enc[a], enc[b], enc[c], use_ntt=False))[0] == (b if a else c)
