"""Seed-compressed packing keys and ring samples on the GPU.  The seeded extract kernel is compared word for word with numpy
(the header's Extract_e on the numpy stream), the seeded unpack with the plain unpack of the host-expanded samples, the
device-expanded packing key's image and packs with the host-expanded key's; decryption, an exhausted device, the counters
and the protocol flag are checked by what they mean.  Every comparison is exact and every device step runs once."""
import re

import numpy as np
import pytest

import seeded_wire_common as W
import unpack_common as U

pytestmark = pytest.mark.gpu

SEED = 0x5EED


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


_SETS = {}


def keyset(n, N, gadget):
    """one device keyset per (n, N), shared by the tests of this file"""
    from peba1_amd import api
    if (n, N) not in _SETS:
        pp = api.ParameterSet(custom=W.custom_tuple(n, N=N, gadget=gadget))
        _SETS[(n, N)] = (pp, api.SecretKeySet(pp, SEED + n, device=True))
    return _SETS[(n, N)]


@pytest.fixture(scope="module", autouse=True)
def close_sets():
    yield
    for _, ks in _SETS.values():
        ks.close()
    _SETS.clear()


@pytest.fixture(scope="module")
def small():
    return keyset(10, 1024, (3, 7))


# ---- the extract kernel alone ----
@pytest.mark.parametrize("N,gadget", [(1024, (3, 7)), (2048, (2, 8))])
def test_seeded_extract_against_numpy(L, N, gadget):
    """three samples under three seeds; e around the wrap, both 16-byte phases and both block phases, of sample 0 and of
    sample 2; a repeat, a descending run; one row, and 257 rows; the padding behind the body is zero"""
    from peba1_amd import api
    pp, ks = keyset(10, N, gadget)
    rng = np.random.default_rng(N)
    comp = W.random_compressed(rng, 3, N)
    ring = W.ring_expand_ref(L, comp, N)
    es = np.array([0, 1, 3, 4, 5, 7, 8, 9, N // 2, N - 9, N - 8, N - 1])
    index = np.concatenate([es, 2 * N + es, [N + 5, N + 5], np.arange(2 * N + 40, 2 * N + 20, -1)])
    index = np.concatenate([index, rng.integers(0, 3 * N, 257 - len(index))])
    assert len(index) == 257
    before, ubefore = api.seeded_stats(), api.unpack_stats()
    got = api.kernel_ring_extract_seeded(ks, comp, index)
    rows = api.extract_rows(N + 4)
    one = api.kernel_ring_extract_seeded(ks, comp, [2 * N + N - 1])
    after, uafter = api.seeded_stats(), api.unpack_stats()
    W.assert_words(got, U.extract_ref(ring, index, N), "257 rows")
    W.assert_words(one, U.extract_ref(ring, [3 * N - 1], N), "one row")
    assert rows.shape == (257, N + 4)
    W.assert_words(rows[:, :N + 1], got, "the rows as stored")
    assert not rows[:, N + 1:].any(), "padding words"
    assert after["seeded_unpack_launches"] - before["seeded_unpack_launches"] == 2
    assert after["seeded_unpacked_samples"] == before["seeded_unpacked_samples"]
    assert uafter["unpack_launches"] - ubefore["unpack_launches"] == 2
    W.assert_words(api.kernel_ring_extract_seeded(ks, comp, count=5), U.extract_ref(ring, np.arange(5), N), "index NULL")


# ---- the unpack ----
def test_seeded_unpack_equals_the_plain_unpack_of_the_expanded_samples(L, small):
    """8,193 coefficients of three samples in any order: two chunks, two launches; the contiguous form"""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(21)
    comp = W.random_compressed(rng, 3, pp.N)
    index = rng.integers(0, 3 * pp.N, 8193)
    plain, seeded = api.CiphertextArray(pp, 8193), api.CiphertextArray(pp, 8193)
    api.unpack(api.ring_expand(comp, pp.N), ks, plain, index=index)
    s0, u0, w0 = api.stats(), api.unpack_stats(), api.seeded_stats()
    api.unpack_seeded(comp, ks, seeded, index=index)
    s1, u1, w1 = api.stats(), api.unpack_stats(), api.seeded_stats()
    assert w1["seeded_unpack_launches"] - w0["seeded_unpack_launches"] == 2
    assert w1["seeded_unpacked_samples"] - w0["seeded_unpacked_samples"] == 8193
    assert u1["unpacked_samples"] - u0["unpacked_samples"] == 8193 and u1["unpack_launches"] - u0["unpack_launches"] == 2
    assert s1["keyswitches"] - s0["keyswitches"] == 8193 and s1["flushes"] == s0["flushes"]
    W.assert_words(seeded.words(), plain.words(), "8,193 across the chunk boundary")
    # and the plain path is the restatement's: a prefix suffices, the suites of the plain unpack pin the rest
    W.assert_words(plain.words()[:64], U.unpack_ref(ks.ksk(), pp, W.ring_expand_ref(L, comp, pp.N), index[:64]), "restatement")
    plain.close()
    seeded.close()


def test_scattered_and_device_forms(L, small):
    import torch
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(22)
    comp = W.random_compressed(rng, 2, pp.N)
    index = rng.integers(0, 2 * pp.N, 100)
    want = api.CiphertextArray(pp, 100)
    api.unpack(api.ring_expand(comp, pp.N), ks, want, index=index)
    ref = want.words()
    a, b = api.CiphertextArray(pp, 60), api.CiphertextArray(pp, 40)
    targets = [(a, j) for j in range(59, -1, -1)] + [(b, j) for j in range(40)]
    api.unpack_seeded(comp, ks, [arr.at(j) for arr, j in targets], index=index)
    wa, wb = a.words(), b.words()
    W.assert_words(wa[::-1], ref[:60], "scattered, first array backwards")
    W.assert_words(wb, ref[60:], "scattered, second array")
    dev = torch.from_numpy(comp.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    d = api.CiphertextArray(pp, 100)
    api.unpack_seeded_device(dev.data_ptr(), 2, ks, d, index=index)
    assert L.tfhe_hip_stream_sync() == 0
    W.assert_words(d.words(), ref, "device form")
    assert api.last_error() == ""
    L.tfhe_hip_clear_error()
    assert L.tfhe_hip_unpack_samples_seeded(ks.cloud, None, 2, None, 5, d.ptr) == -1 and "null" in api.last_error()
    bad = np.array([2 * pp.N], dtype=np.int32)
    from peba1_amd import lib
    assert L.tfhe_hip_unpack_samples_seeded(ks.cloud, comp.ctypes.data_as(lib.I32P), 2, bad.ctypes.data_as(lib.I32P), 1, d.ptr) == -1
    assert "outside" in api.last_error()
    W.assert_words(d.words(), ref, "a refused call changes nothing")
    L.tfhe_hip_clear_error()
    del dev
    for o in (want, a, b, d):
        o.close()


def test_recorded_gates_stay_recorded_across_a_seeded_unpack(L, small):
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(23)
    xa, xb = rng.integers(0, 2, 16), rng.integers(0, 2, 16)
    L.tfhe_hip_set_encrypt_seed(2323)
    a, b = api.CiphertextArray(pp, 16).encrypt(xa, ks), api.CiphertextArray(pp, 16).encrypt(xb, ks)
    r1, r2, u = api.CiphertextArray(pp, 16), api.CiphertextArray(pp, 16), api.CiphertextArray(pp, 8)
    api.flush()
    for i in range(16):
        L.bootsAND(r2.at(i), a.at(i), b.at(i), ks.cloud)
    api.flush()
    before = api.stats()
    for i in range(16):
        L.bootsAND(r1.at(i), a.at(i), b.at(i), ks.cloud)
    api.unpack_seeded(W.random_compressed(rng, 1, pp.N), ks, u, count=8)
    mid = api.stats()
    assert mid["blind_rotates"] == before["blind_rotates"] and mid["flushes"] == before["flushes"]
    api.flush()
    assert api.stats()["blind_rotates"] - before["blind_rotates"] == 16
    W.assert_words(r1.words(), r2.words(), "gates pending across the unpack")
    for o in (a, b, r1, r2, u):
        o.close()


# ---- at P128 ----
def test_p128_bits_travel_compressed_and_gate_right(L, p128_keys):
    from peba1_amd import api
    pp, ks, _ = p128_keys
    rng = np.random.default_rng(24)
    bits = rng.integers(0, 2, 1024)
    comp = api.ring_encrypt_bits(bits, ks, compressed=True)
    assert comp.nbytes == 4136
    seeded, plain, g = api.CiphertextArray(pp, 1024), api.CiphertextArray(pp, 1024), api.CiphertextArray(pp, 512)
    api.unpack_seeded(comp, ks, seeded, count=1024)
    api.unpack(api.ring_expand(comp, pp.N), ks, plain, count=1024)
    W.assert_words(seeded.words(), plain.words(), "P128: seeded against plain")
    assert seeded.decrypt(ks).tolist() == bits.tolist()
    assert L.tfhe_hip_gate_batch(2, g.ptr, seeded.at(0), seeded.at(512), 512, ks.cloud) == 0
    api.flush()
    assert g.decrypt(ks).tolist() == (bits[:512] & bits[512:]).tolist()
    for o in (seeded, plain, g):
        o.close()


# ---- the packing key ----
@pytest.mark.parametrize("n,t,bb,N,gadget", W.KEY_CASES)
def test_device_expanded_image_equals_the_host_expanded_one(n, t, bb, N, gadget):
    from peba1_amd import api
    pp, ks = keyset(n, N, gadget)
    ck = api.CompressedPackingKey.generate_seeded(ks, W.NOISE_SEED, W.MASK_SEED, t, bb)
    dev, host = ck.expand(), ck.expand_host()
    ck.close()
    try:
        before = api.seeded_stats()
        img_d = api.pack_image(dev, ks)
        mid = api.seeded_stats()
        img_h = api.pack_image(host, ks)
        assert mid["expanded_packing_keys"] - before["expanded_packing_keys"] == 1
        assert mid["packing_expand_launches"] - before["packing_expand_launches"] == 1
        assert img_d.size == 2 * n * t * 2 * N
        W.assert_words(img_d, img_h, "image, device against host expansion")
        W.assert_words(api.pack_image(dev, ks), img_h, "the image is made once")
        assert api.seeded_stats() == mid                                # the host-expanded key counts nothing
        W.assert_words(dev.words(), host.words(), "host rows of the device-expanded key, made on demand")
    finally:
        dev.close()
        host.close()


def test_packs_under_the_device_expanded_key(L, small):
    """count 1 and count N through the raw entry, and through the slot entry, against the host-expanded key"""
    from peba1_amd import api
    pp, ks = small
    ck = api.CompressedPackingKey.generate(ks)
    dev, host = api.CompressedPackingKey.from_words(pp, ck.t, ck.basebit, ck.seed(), ck.body()).expand(), ck.expand_host()
    ck.close()
    rng = np.random.default_rng(25)
    sw = rng.integers(U.I32_MIN, U.I32_MAX + 1, size=(pp.N, pp.words), dtype=np.int64).astype(np.int32)
    arr = api.CiphertextArray(pp, pp.N)
    arr.set_words(sw)
    for count in (1, pp.N):
        W.assert_words(api.kernel_pack(dev, ks, sw[:count]), api.kernel_pack(host, ks, sw[:count]), ("kernel_pack", count))
        W.assert_words(api.pack(dev, arr, count, ks), api.pack(host, arr, count, ks), ("pack", count))
    for o in (arr, dev, host):
        o.close()


@pytest.fixture(scope="module")
def p128_pack(p128_keys):
    """(compressed packing key, host-expanded key) of the product's set, t = 8, base 4"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    ck = api.CompressedPackingKey.generate_seeded(ks, W.NOISE_SEED, W.MASK_SEED)
    host = ck.expand_host()
    yield ck, host
    host.close()
    ck.close()


def test_p128_image_and_packed_gate_outputs(L, p128_keys, p128_pack):
    from peba1_amd import api
    pp, ks, _ = p128_keys
    ck, host = p128_pack
    assert (ck.t, ck.basebit, ck.nbytes) == (8, 2, 40 + 20643840)
    dev = ck.expand()
    before = api.seeded_stats()
    W.assert_words(api.pack_image(dev, ks), api.pack_image(host, ks), "P128 image")
    after = api.seeded_stats()
    assert after["expanded_packing_keys"] - before["expanded_packing_keys"] == 1
    assert after["packing_expand_launches"] - before["packing_expand_launches"] == 1
    rng = np.random.default_rng(26)
    xa, xb = rng.integers(0, 2, 1024), rng.integers(0, 2, 1024)
    a, b = api.CiphertextArray(pp, 1024).encrypt(xa, ks), api.CiphertextArray(pp, 1024).encrypt(xb, ks)
    r = api.CiphertextArray(pp, 1024)
    assert L.tfhe_hip_gate_batch(4, r.ptr, a.ptr, b.ptr, 1024, ks.cloud) == 0
    packed = api.pack(dev, r, 1024, ks)
    W.assert_words(packed, api.pack(host, r, 1024, ks), "1,024 gate outputs, device- against host-expanded key")
    assert api.packed_decrypt(packed, 1024, ks).tolist() == (xa ^ xb).tolist()
    for o in (a, b, r, dev):
        o.close()


def test_exhausted_device_at_the_first_pack(L, p128_keys, p128_pack):
    """the cap admits the image but not the staging copy, then both but not the bodies: the pack fails with the error set
    and nothing held (the figure a refusal under a cap of one byte reports is the same before and after); with the cap
    lifted the same call gives the host-expanded key's words"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    ck, host = p128_pack
    dev = ck.expand()
    arr = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    api.flush()
    out = np.full(2 * pp.N, 7, dtype=np.int32)

    def refused(cap):
        from peba1_amd import lib
        L.tfhe_hip_test_set_alloc_cap(cap)
        L.tfhe_hip_clear_error()
        before = api.seeded_stats()
        rc = L.tfhe_hip_pack_samples(dev.ptr, arr.ptr, 4, ks.cloud, out.ctypes.data_as(lib.I32P))
        L.tfhe_hip_test_set_alloc_cap(0)
        msg = api.last_error()
        assert rc == -1 and "out of device memory" in msg and api.seeded_stats() == before and (out == 7).all(), (rc, msg)
        return msg, int(re.search(r"\((\d+) MiB held", msg).group(1))

    try:
        _, held = refused(1)
        # the image is 78.8 MiB, the staging copy 39.4 MiB, the bodies 19.7 MiB
        assert "staging copy of a packing key" in refused((held + 100) << 20)[0]
        assert "bodies of a compressed packing key" in refused((held + 125) << 20)[0]
        assert refused(1)[1] == held
        L.tfhe_hip_clear_error()
        W.assert_words(api.pack(dev, arr, 4, ks), api.pack(host, arr, 4, ks), "the same call after the cap was lifted")
        assert api.packed_decrypt(api.pack(dev, arr, 4, ks), 4, ks).tolist() == [1, 0, 1, 1]
    finally:
        L.tfhe_hip_test_set_alloc_cap(0)
        arr.close()
        dev.close()


# ---- the callers ----
def test_protocol_with_seeded_inputs(p128_keys):
    """protocol.py --seeded-inputs --nslots 2: the genuine and the impostor run give the y, the match bit and the verdict
    they give without the flag"""
    from peba1_amd import protocol
    pp, ks, _ = p128_keys
    a = protocol.parse_args(["--seeded-inputs", "--nslots", "2"])
    assert a.seeded_inputs and a.nslots == 2 and not protocol.parse_args([]).seeded_inputs
    template = [(37 * i + 11) % 255 for i in range(a.nslots)]
    runs = {"genuine": [t + 1 for t in template], "impostor": [(91 * i + 5) % 256 for i in range(a.nslots)]}
    for name, sample in runs.items():
        want = protocol.run_p1(pp, ks, sample, template, a.bound, r0=17, r1=99)
        got = protocol.run_p1(pp, ks, sample, template, a.bound, r0=17, r1=99, seeded_inputs=True)
        for field in ("y", "match_bit", "authenticated"):
            assert got[field] == want[field], (name, field, got, want)


def test_gallery_rests_compressed(p128_keys):
    """identify.unpack_templates and EncryptedVector.from_ring take compressed records, told apart by their word count"""
    from peba1_amd import circuits, identify
    pp, ks, _ = p128_keys
    values = [[5, 250, 17], [0, 255, 128]]
    comp = [circuits.ring_encrypt_vector(v, 8, ks, compressed=True) for v in values]
    plain = circuits.ring_encrypt_vector(values[0], 8, ks)
    assert comp[0].size == 10 + pp.N and plain.size == 2 * pp.N
    vecs = identify.unpack_templates(comp + [plain], pp, 3, 8, ks)
    for vec, v in zip(vecs, values + [values[0]]):
        assert [int(sum(int(b) << j for j, b in enumerate(s.decrypt(ks)))) for s in vec.slots] == v
        for s in vec.slots:
            s.close()
