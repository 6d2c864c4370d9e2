"""Seed-compressed LWE sample arrays on the GPU.  The expand kernel is compared word for word with the host expansion and
with the numpy restatement of tests/seeded_lwe_common.py, the seeded import with the plain import of the host-expanded
samples; recording across an import, decryption at P128, an exhausted device, the counters and the protocol flag are checked
by what they mean.  Every comparison is exact and every device step runs once."""
import numpy as np
import pytest

import seeded_lwe_common as S

pytestmark = pytest.mark.gpu

SEED = 0x1E5EED


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


@pytest.fixture(scope="module")
def small():
    """a device keyset of n = 10: slots of 12 words"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=S.custom_tuple(10))
    ks = api.SecretKeySet(pp, SEED, device=True)
    yield pp, ks
    ks.close()


# ---- the kernel alone ----
@pytest.mark.parametrize("n", S.DIMENSIONS)
def test_kernel_against_the_host_expansion_and_numpy(L, n):
    """257 rows and one row: sample 0, the record's last sample, a repeat, a descending run, random samples; at n = 630 and
    1,024 the record is the largest (2^20 samples: the last row starts at stream word 2^20 n - n); the body sits at word n
    and every padding word behind it is zero; the launch counter moves by the launches made, the sample counter not"""
    from peba1_amd import api
    pp = api.ParameterSet(custom=S.custom_tuple(n))
    rng = np.random.default_rng(n)
    record_count = S.RECORD_MAX if n >= 630 else 300
    rec = S.random_record(rng, record_count)
    index = S.index_cases(rng, record_count, 257)
    before = api.seeded_lwe_stats()
    got = api.kernel_lwe_expand(pp, rec, index)
    stored = api.expand_slots(S.stride_of(n))
    one = api.kernel_lwe_expand(pp, rec, [record_count - 1])
    head = api.kernel_lwe_expand(pp, rec, count=5)
    after = api.seeded_lwe_stats()
    assert after["seeded_import_launches"] - before["seeded_import_launches"] == 3
    assert after["seeded_imported_samples"] == before["seeded_imported_samples"]
    host = api.lwe_expand(rec, n, index)
    S.assert_words(host, S.expand_ref(L, rec, n, index), "host expansion against numpy")
    S.assert_words(got, host, ("257 rows", n))
    S.assert_words(one, host[1:2], "one row: the last sample")
    S.assert_words(head, api.lwe_expand(rec, n, count=5), "index NULL")
    assert stored.shape == (257, S.stride_of(n))
    S.assert_words(stored[:, :n + 1], got, "the rows as stored")
    S.assert_words(stored[:, n], rec[10 + index.astype(np.int64)], "the body at word n")
    assert not stored[:, n + 1:].any(), "padding words"


# ---- the import ----
def test_import_equals_the_plain_import_of_the_host_expansion(L, small):
    """8,193 samples of a record of 9,000 in random order: two chunks, two launches; no flush, no key switch"""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(31)
    rec = S.random_record(rng, 9000)
    index = rng.integers(0, 9000, 8193).astype(np.int32)
    index[:3] = (8999, 0, 8999)
    plain, seeded = api.CiphertextArray(pp, 8193), api.CiphertextArray(pp, 8193)
    plain.set_words(api.lwe_expand(rec, pp.n, index))
    s0, w0 = api.stats(), api.seeded_lwe_stats()
    api.import_seeded(rec, pp, seeded, index=index)
    s1, w1 = api.stats(), api.seeded_lwe_stats()
    assert w1["seeded_import_launches"] - w0["seeded_import_launches"] == 2
    assert w1["seeded_imported_samples"] - w0["seeded_imported_samples"] == 8193
    assert s1["flushes"] == s0["flushes"] and s1["keyswitches"] == s0["keyswitches"]
    S.assert_words(seeded.words(), plain.words(), "8,193 across the chunk boundary")
    S.assert_words(plain.words()[:40], S.expand_ref(L, rec, pp.n, index[:40]), "restatement")
    whole = api.CiphertextArray(pp, 9000)
    api.import_seeded(rec, pp, whole)
    S.assert_words(whole.words(), api.lwe_expand(rec, pp.n), "index NULL: the whole record")
    for o in (plain, seeded, whole):
        o.close()


def test_scattered_and_device_forms(L, small):
    import torch
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(32)
    rec = S.random_record(rng, 500)
    index = rng.integers(0, 500, 100).astype(np.int32)
    ref = api.lwe_expand(rec, pp.n, index)
    a, b = api.CiphertextArray(pp, 60), api.CiphertextArray(pp, 40)
    targets = [(a, j) for j in range(59, -1, -1)] + [(b, j) for j in range(40)]
    api.import_seeded(rec, pp, [arr.at(j) for arr, j in targets], index=index)
    S.assert_words(a.words()[::-1], ref[:60], "scattered, first array backwards")
    S.assert_words(b.words(), ref[60:], "scattered, second array")
    dev = torch.from_numpy(rec).to("cuda:0")
    torch.cuda.synchronize()
    d = api.CiphertextArray(pp, 100)
    before = api.seeded_lwe_stats()
    api.import_seeded_device(dev.data_ptr(), 500, pp, d, index=index)
    assert L.tfhe_hip_stream_sync() == 0
    after = api.seeded_lwe_stats()
    assert after["seeded_imported_samples"] - before["seeded_imported_samples"] == 100
    assert after["seeded_import_launches"] - before["seeded_import_launches"] == 1
    S.assert_words(d.words(), ref, "device form")
    assert api.last_error() == ""
    from peba1_amd import lib
    bad = np.array([500], dtype=np.int32)
    assert L.tfhe_hip_import_samples_seeded(pp.ptr, rec.ctypes.data_as(lib.I32P), 500, bad.ctypes.data_as(lib.I32P), 1, d.ptr) == -1
    assert "outside" in api.last_error()
    S.assert_words(d.words(), ref, "a refused call changes nothing")
    L.tfhe_hip_clear_error()
    del dev
    for o in (a, b, d):
        o.close()


def test_recorded_gates_stay_recorded_across_a_seeded_import(L, small):
    """record, import, record on the imported samples, flush once: every word equals the same program on plainly imported
    samples"""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(33)
    xa, xb, xc = (rng.integers(0, 2, 16) for _ in range(3))
    L.tfhe_hip_set_encrypt_seed(3333)
    a, b = api.CiphertextArray(pp, 16).encrypt(xa, ks), api.CiphertextArray(pp, 16).encrypt(xb, ks)
    rec = api.encrypt_bits_compressed(xc, ks, seed=S.NOISE_SEED, mask_seed=S.MASK_SEED)
    r1, r2, q1, q2 = (api.CiphertextArray(pp, 16) for _ in range(4))
    plain, seeded = api.CiphertextArray(pp, 16), api.CiphertextArray(pp, 16)
    plain.set_words(api.lwe_expand(rec, pp.n))
    api.flush()
    for i in range(16):
        L.bootsAND(r2.at(i), a.at(i), b.at(i), ks.cloud)
        L.bootsXOR(q2.at(i), plain.at(i), r2.at(i), ks.cloud)
    api.flush()
    before = api.stats()
    for i in range(16):
        L.bootsAND(r1.at(i), a.at(i), b.at(i), ks.cloud)
    api.import_seeded(rec, pp, seeded)
    mid = api.stats()
    assert mid["blind_rotates"] == before["blind_rotates"] and mid["flushes"] == before["flushes"]
    for i in range(16):
        L.bootsXOR(q1.at(i), seeded.at(i), r1.at(i), ks.cloud)
    api.flush()
    after = api.stats()
    assert after["blind_rotates"] - before["blind_rotates"] == 32 and after["flushes"] - before["flushes"] == 1
    S.assert_words(r1.words(), r2.words(), "gates pending across the import")
    S.assert_words(q1.words(), q2.words(), "gates on the imported samples")
    assert q1.decrypt(ks).tolist() == (xc ^ (xa & xb)).tolist()
    for o in (a, b, r1, r2, q1, q2, plain, seeded):
        o.close()


# ---- at P128 ----
def test_p128_bits_travel_as_4136_bytes_and_gate_right(L, p128_keys):
    from peba1_amd import api
    pp, ks, _ = p128_keys
    rng = np.random.default_rng(34)
    x, y = rng.integers(0, 2, 1024), rng.integers(0, 2, 1024)
    rx, ry = api.encrypt_bits_compressed(x, ks), api.encrypt_bits_compressed(y, ks)
    assert rx.nbytes == 4136 and (rx[:10] != ry[:10]).any()
    ax, ay, g = api.CiphertextArray(pp, 1024), api.CiphertextArray(pp, 1024), api.CiphertextArray(pp, 1024)
    api.import_seeded(rx, pp, ax)
    api.import_seeded(ry, pp, ay)
    S.assert_words(ax.words(), api.lwe_expand(rx, pp.n), "P128: the imported words")
    assert ax.decrypt(ks).tolist() == x.tolist() and ay.decrypt(ks).tolist() == y.tolist()
    assert L.tfhe_hip_gate_batch(2, g.ptr, ax.ptr, ay.ptr, 512, ks.cloud) == 0
    assert L.tfhe_hip_gate_batch(4, g.at(512), ax.at(512), ay.at(512), 512, ks.cloud) == 0
    api.flush()
    assert g.decrypt(ks).tolist() == np.concatenate([x[:512] & y[:512], x[512:] ^ y[512:]]).tolist()
    for o in (ax, ay, g):
        o.close()


# ---- the callers ----
def test_protocol_with_seeded_lwe(p128_keys):
    """protocol.py --seeded-lwe --nslots 2: the genuine and the impostor run give the y, the match bit and the verdict they
    give without the flag"""
    from peba1_amd import protocol
    pp, ks, _ = p128_keys
    a = protocol.parse_args(["--seeded-lwe", "--nslots", "2"])
    assert a.seeded_lwe and a.nslots == 2 and not protocol.parse_args([]).seeded_lwe
    template = [(37 * i + 11) % 255 for i in range(a.nslots)]
    runs = {"genuine": [t + 1 for t in template], "impostor": [(91 * i + 5) % 256 for i in range(a.nslots)]}
    for name, sample in runs.items():
        want = protocol.run_p1(pp, ks, sample, template, a.bound, r0=17, r1=99)
        got = protocol.run_p1(pp, ks, sample, template, a.bound, r0=17, r1=99, seeded_lwe=True)
        for field in ("y", "match_bit", "authenticated"):
            assert got[field] == want[field], (name, field, got, want)


# ---- an exhausted device ----
def words_of(arr, first, count):
    """the words of arr[first .. first + count): an export moves at most 65,536 samples"""
    from peba1_amd import api, lib
    out = np.zeros((count, arr.params.words), dtype=np.int32)
    for at in range(0, count, 65536):
        part = out[at:at + 65536]
        if lib.load().tfhe_hip_export_samples(arr.at(first + at), len(part), arr.params.ptr, part.ctypes.data_as(lib.I32P)) != 0:
            raise RuntimeError(api.last_error())
    return out


def test_exhausted_device_at_the_pool_growth(L):
    """a pool of its own shape (n = 13) holds 65,536 slots when it is made; an import of 70,000 samples must grow it.
    Under a cap of one byte the growth fails: -1, the error set, results, counters and the pool as they were; with the cap
    lifted the same call succeeds"""
    from peba1_amd import api, lib
    pp = api.ParameterSet(custom=S.custom_tuple(13))
    rng = np.random.default_rng(35)
    count = 70000
    rec = S.random_record(rng, count)
    arr = api.CiphertextArray(pp, count)
    api.import_seeded(rec, pp, arr, index=[5, 4, 3])                   # makes the pool; three results hold slots
    held = words_of(arr, 0, 3)
    before = api.seeded_lwe_stats()
    L.tfhe_hip_clear_error()
    L.tfhe_hip_test_set_alloc_cap(1)
    try:
        rc = L.tfhe_hip_import_samples_seeded(pp.ptr, rec.ctypes.data_as(lib.I32P), count, None, count, arr.ptr)
    finally:
        L.tfhe_hip_test_set_alloc_cap(0)
    msg = api.last_error()
    assert rc == -1 and "out of device memory" in msg and "growing the ciphertext slot pool" in msg, (rc, msg)
    assert api.seeded_lwe_stats() == before
    S.assert_words(words_of(arr, 0, 3), held, "results after the refused import")
    L.tfhe_hip_clear_error()
    api.import_seeded(rec, pp, arr)
    after = api.seeded_lwe_stats()
    assert after["seeded_imported_samples"] - before["seeded_imported_samples"] == count
    assert after["seeded_import_launches"] - before["seeded_import_launches"] == 9      # ceil(70,000 / 8,192)
    S.assert_words(words_of(arr, 0, count), api.lwe_expand(rec, pp.n), "the same call after the cap was lifted")
    assert api.last_error() == ""
    arr.close()
