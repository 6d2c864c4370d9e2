"""Seed-compressed cloud keys on the GPU: the device kernels' stream against the host blocks, the device images of a
device-expanded keyset against those of a host-expanded one word for word (padding and zero row included), the product's
paths under a device-expanded P128 key, an exhausted device and the counters.  Every comparison is exact and every device
step runs once.

What stands in for "the oracle's words from tfhe_hip_key_bk / _ksk" at P128: the oracle's fast evaluators read transformed
images of the key it generated itself, and its schoolbook evaluator takes about ten seconds per rotation at n = 630.  So
the 64 rotations are compared with the same launch under the HOST-expanded keyset -- the untouched plain path, which the
existing suites pin to the oracle -- and with the oracle's schoolbook words on a small set; the 64 key switches with the
numpy restatement of tests/ks_common.py fed tfhe_hip_key_ksk of the device-expanded keyset."""
import re

import numpy as np
import pytest

import compressed_common as K
import unpack_common as U
import pack_common as P

pytestmark = pytest.mark.gpu

GATES = ["NAND", "OR", "AND", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
TRUTH = {"NAND": lambda a, b: 1 - (a & b), "OR": lambda a, b: a | b, "AND": lambda a, b: a & b, "NOR": lambda a, b: 1 - (a | b),
         "XOR": lambda a, b: a ^ b, "XNOR": lambda a, b: 1 - (a ^ b), "ANDNY": lambda a, b: (1 - a) & b,
         "ANDYN": lambda a, b: a & (1 - b), "ORNY": lambda a, b: (1 - a) | b, "ORYN": lambda a, b: a | (1 - b)}


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module", autouse=True)
def deferred():
    from peba1_amd import api
    was = api.get_deferred()
    api.set_deferred(True)
    yield
    api.set_deferred(was)


def assert_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got[bad[:3]], want[bad[:3]])


# ---- the raw stream ----
@pytest.mark.parametrize("first,count", [(0, 1), (0, 7), (0, 8), (0, 9), (0, 64), (0, 4099), (5, 30), (8 * 2 ** 32 - 12, 24)])
def test_device_stream_against_the_host_blocks(L, first, count):
    """counts around a block and past a workgroup, an unaligned start, and a range straddling block counter 2^32: the carry
    into the high counter word"""
    from peba1_amd import api
    before = api.expand_stats()
    assert_words(api.kernel_expand_masks(K.MASK_SEED, first, count), K.stream_words(L, K.MASK_SEED, first, count), (first, count))
    after = api.expand_stats()
    assert after["expand_launches"] - before["expand_launches"] == 1 and after["expanded_keys"] == before["expanded_keys"]


# ---- the images ----
IMAGE_CASES = [(n, (8, 2), 1024, (2, 10)) for n in (1, 7, 8, 9, 10)] + [
    (630, (8, 2), 1024, (2, 10)), (10, (2, 4), 1024, (2, 10)), (10, (1, 8), 1024, (2, 10)), (10, (8, 2), 1024, (3, 7)),
    (10, (8, 2), 2048, (2, 8)), (1023, (8, 2), 1024, (2, 10))]


@pytest.mark.parametrize("n,ks,N,gadget", IMAGE_CASES)
def test_device_images_equal_the_host_expanded_ones(n, ks, N, gadget):
    """rows shorter than, equal to and one past a block; the product's row width; 15 and 255 rows per digit; l = 3;
    N = 2,048; n = 1,023 (and 7), whose rows leave no padding word behind the body.  Both keysets are used once (their image is
    made); BK images and compact KSKs are identical, and the compact KSK is the numpy restatement of the host words"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(n, N=N, ks=ks, gadget=gadget))
    sh = K.Shape(pp)
    assert (sh.stride == n + 1) == (n in (7, 1023))                          # rows without a padding word
    sk = api.SecretKeySet(pp, 100 + n, device=False)
    ck = api.CompressedCloudKey.generate_seeded(sk, K.NOISE_SEED, K.MASK_SEED)
    dev, host = ck.expand(), ck.expand_host()
    try:
        before = api.expand_stats()
        ksk_d, ksk_h = api.key_image(dev, 1), api.key_image(host, 1)
        after = api.expand_stats()
        assert after["expanded_keys"] - before["expanded_keys"] == 1 and after["expand_launches"] - before["expand_launches"] == 2
        assert ksk_d.size == (sh.ksk_body_words + 1) * sh.stride
        assert_words(ksk_d, ksk_h, "compact KSK, device against host expansion")
        assert_words(ksk_h, K.compact_ksk(host.ksk(), sh), "compact KSK against its restatement")
        bk_d, bk_h = api.key_image(dev, 0), api.key_image(host, 0)
        assert bk_d.size == 2 * sh.bk_words
        assert_words(bk_d, bk_h, "BK image")
        assert api.expand_stats() == after                                    # the images are made once
    finally:
        dev.close()
        host.close()
        ck.close()
        sk.close()


# ---- use at P128 ----
@pytest.fixture(scope="module")
def p128x():
    """(parameter set, secret keyset on the host, device-expanded keyset, host-expanded keyset) of the product's set"""
    from peba1_amd import api
    pp = api.ParameterSet(128)
    sk = api.SecretKeySet(pp, 0xC0FFEE, device=False)
    ck = api.CompressedCloudKey.generate_seeded(sk, K.NOISE_SEED, K.MASK_SEED)
    dev, host = ck.expand(), ck.expand_host()
    ck.close()                                           # the keysets hold what they need
    yield pp, sk, dev, host
    dev.close()
    host.close()
    sk.close()


def test_p128_rotations_and_key_switches(p128x):
    """64 random rotations and 64 key switches through the raw entries; tfhe_hip_key_bk / _ksk of the device-expanded
    keyset (made on demand) are the host-expanded words"""
    from peba1_amd import api
    pp, sk, dev, host = p128x
    rng = np.random.default_rng(3)
    lin = rng.integers(U.I32_MIN, U.I32_MAX + 1, size=(64, pp.n + 1), dtype=np.int64).astype(np.int32)
    before = api.expand_stats()
    u_dev = api.kernel_bootstrap_woks(dev, lin)
    after = api.expand_stats()
    assert after["expanded_keys"] - before["expanded_keys"] == 1 and after["expand_launches"] - before["expand_launches"] == 2
    assert_words(u_dev, api.kernel_bootstrap_woks(host, lin), "64 rotations, device- against host-expanded key")
    assert api.expand_stats() == after                                        # a host-expanded key counts nothing
    assert_words(dev.bk(), host.bk(), "tfhe_hip_key_bk of the device-expanded keyset")
    assert_words(dev.ksk(), host.ksk(), "tfhe_hip_key_ksk of the device-expanded keyset")
    u = rng.integers(U.I32_MIN, U.I32_MAX + 1, size=(64, pp.N + 1), dtype=np.int64).astype(np.int32)
    want = U.keyswitch_ref(dev.ksk(), u, pp.n, pp.N, pp.ks_t, pp.ks_basebit)
    assert_words(api.kernel_keyswitch(dev, u), want, "64 key switches against the restatement")


def test_small_set_rotations_against_the_oracle(oracle):
    """n = 16: the oracle's schoolbook evaluator over tfhe_hip_key_bk / _ksk of a device-expanded keyset"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=K.custom_tuple(16, gadget=(2, 10)))
    sk = api.SecretKeySet(pp, 77, device=False)
    ck = api.CompressedCloudKey.generate_seeded(sk, K.NOISE_SEED, K.MASK_SEED)
    dev = ck.expand()
    try:
        rng = np.random.default_rng(4)
        lin = rng.integers(U.I32_MIN, U.I32_MAX + 1, size=(8, pp.n + 1), dtype=np.int64).astype(np.int32)
        got = api.kernel_bootstrap_woks(dev, lin)
        oks = oracle.KeySet(oracle.custom_params(n=16, N=1024, l=2, Bgbit=10), 1)
        oks.bk()[:] = dev.bk()
        oks.ksk()[:] = dev.ksk()
        for c in range(len(lin)):
            u = oks.bootstrap_woks(lin[c], use_ntt=False)
            assert_words(got[c], u, ("rotation", c))
        assert_words(api.kernel_keyswitch(dev, got), np.stack([oks.keyswitch(u) for u in got]), "key switches")
    finally:
        dev.close()
        ck.close()
        sk.close()


def test_p128_recorded_gates_decrypt_right(L, p128x):
    """256 recorded gates of mixed kinds, one flush, under the device-expanded key"""
    from peba1_amd import api
    pp, sk, dev, host = p128x
    rng = np.random.default_rng(5)
    xa, xb = rng.integers(0, 2, 256), rng.integers(0, 2, 256)
    a, b = api.CiphertextArray(pp, 256).encrypt(xa, sk), api.CiphertextArray(pp, 256).encrypt(xb, sk)
    r = api.CiphertextArray(pp, 256)
    api.flush()
    before = api.stats()
    for i in range(256):
        getattr(L, "boots" + GATES[i % 10])(r.at(i), a.at(i), b.at(i), dev.cloud)
    api.flush()
    after = api.stats()
    assert after["blind_rotates"] - before["blind_rotates"] == 256 and after["flushes"] - before["flushes"] == 1
    want = [TRUTH[GATES[i % 10]](int(xa[i]), int(xb[i])) for i in range(256)]
    assert r.decrypt(sk).tolist() == want
    for x in (a, b, r):
        x.close()


def test_p128_multi_key_flush_with_a_plain_key(L, p128x, p128_keys):
    """one flush ("batch_keys") over a plain key and a device-expanded key of the same set: the plain key's results are the
    oracle's words, the expanded key's those of the same gates run alone under the host-expanded keyset"""
    from peba1_amd import api
    pp, sk, dev, host = p128x
    ppa, ksa, oks = p128_keys
    rng = np.random.default_rng(6)
    xa, xb = rng.integers(0, 2, 8), rng.integers(0, 2, 8)
    L.tfhe_hip_set_encrypt_seed(606)
    a1, b1 = api.CiphertextArray(ppa, 8).encrypt(xa, ksa), api.CiphertextArray(ppa, 8).encrypt(xb, ksa)
    a2, b2 = api.CiphertextArray(pp, 8).encrypt(xa, sk), api.CiphertextArray(pp, 8).encrypt(xb, sk)
    r1, r2, alone = api.CiphertextArray(ppa, 8), api.CiphertextArray(pp, 8), api.CiphertextArray(pp, 8)
    api.flush()
    had = L.tfhe_hip_set_batch_keys(1)
    try:
        for i in range(8):
            L.bootsXOR(r1.at(i), a1.at(i), b1.at(i), ksa.cloud)
            L.bootsNAND(r2.at(i), a2.at(i), b2.at(i), dev.cloud)
        api.flush()
        assert api.last_flush_keys() == 2
    finally:
        L.tfhe_hip_set_batch_keys(had)
    for i in range(8):
        L.bootsNAND(alone.at(i), a2.at(i), b2.at(i), host.cloud)
    api.flush()
    w1a, w1b, got1 = a1.words(), b1.words(), r1.words()
    for i in range(8):
        assert_words(got1[i], oks.gate("XOR", w1a[i], w1b[i]), ("plain key against the oracle", i))
    assert_words(r2.words(), alone.words(), "expanded key against the same gates alone")
    assert r2.decrypt(sk).tolist() == [1 - (int(x) & int(y)) for x, y in zip(xa, xb)]
    for x in (a1, b1, a2, b2, r1, r2, alone):
        x.close()


def test_p128_pack_and_unpack_under_the_expanded_key(L, p128x):
    from peba1_amd import api
    pp, sk, dev, host = p128x
    rng = np.random.default_rng(7)
    ring = U.random_ring(rng, 1, pp.N)
    index = rng.integers(0, pp.N, 40)
    r = api.CiphertextArray(pp, 40)
    api.unpack(ring, dev, r, index=index)
    assert_words(r.words(), U.unpack_ref(dev.ksk(), pp, ring, index), "unpack")
    pk = api.PackingKey(sk, seed=9)
    rows = P.KeyRows(np.asarray(pk.words()).reshape(pp.n, pk.t, 2, pp.N))
    assert_words(api.pack(pk, r, 40, dev), P.pack_ref(rows, r.words(), pk.basebit), "pack")
    pk.close()
    r.close()


# ---- an exhausted device ----
def test_exhausted_device_at_first_use(L, p128x):
    """with the cap below the staging need the first use fails with a message and nothing is held; after the cap is lifted
    the same keyset works.  What is held shows in the message of a refusal under a cap of one byte, before and after"""
    from peba1_amd import api
    pp, sk, dev0, host = p128x
    ck = api.CompressedCloudKey.generate_seeded(sk, 11, K.MASK_SEED)
    dev = ck.expand()
    ck.close()
    a, b = api.CiphertextArray(pp, 1).encrypt([1], sk), api.CiphertextArray(pp, 1).encrypt([1], sk)
    r = api.CiphertextArray(pp, 1)
    api.flush()

    def refused(cap):
        L.tfhe_hip_test_set_alloc_cap(cap)
        L.tfhe_hip_clear_error()
        before = api.expand_stats()
        rc = L.tfhe_hip_gate_batch(2, r.ptr, a.ptr, b.ptr, 1, dev.cloud)
        L.tfhe_hip_test_set_alloc_cap(0)
        msg = api.last_error()
        assert rc == -1 and "out of device memory" in msg and api.expand_stats() == before, (rc, msg)
        return msg, int(re.search(r"\((\d+) MiB held", msg).group(1))

    try:
        _, held = refused(1)
        # twiddles, BK image (59 MiB) and compact KSK (59 MiB) fit, the staging copy of the BK (30 MiB) does not
        msg, _ = refused((held + 140) << 20)
        assert "staging copy" in msg or "bodies" in msg, msg
        assert refused(1)[1] == held
        assert L.tfhe_hip_gate_batch(2, r.ptr, a.ptr, b.ptr, 1, dev.cloud) == 0
        assert r.decrypt(sk).tolist() == [1]
    finally:
        L.tfhe_hip_test_set_alloc_cap(0)
        for x in (a, b, r):
            x.close()
        dev.close()
