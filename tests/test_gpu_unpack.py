"""Ring-encrypted inputs on the GPU.  The extract kernel and the full unpack are compared word for word with the numpy
restatement (tests/unpack_common.py: extract_ref from the header's definition, keyswitch_ref of tests/ks_common.py behind
it); decryption, the round trip through the packing key switch, an exhausted device, the statistics and the device form
are checked by what they mean.  References are computed once per parameter set and shared."""
import ctypes as C

import numpy as np
import pytest

import unpack_common as U

pytestmark = pytest.mark.gpu

SEED = 0x7AC2
N_TILED = 256                   # the narrowest LWE width the tiled key-switch kernels are built for (128 threads)


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


@pytest.fixture(scope="module", autouse=True)
def deferred():
    """the mode an unmodified caller runs in; one test below asks for immediate mode itself"""
    from peba1_amd import api
    was = api.get_deferred()
    api.set_deferred(True)
    yield
    api.set_deferred(was)


def _keyset(n, N=1024, ks=(8, 2), gadget=(3, 7)):
    from peba1_amd import api
    pp = api.ParameterSet(custom=U.custom_tuple(n, N=N, ks=ks, gadget=gadget))
    return pp, api.SecretKeySet(pp, SEED, device=True)


@pytest.fixture(scope="module")
def small():
    """n = 10, N = 1,024, the default decomposition: 64-thread key-switch rows, the per-gate kernel"""
    pp, ks = _keyset(10)
    yield pp, ks
    ks.close()


@pytest.fixture(scope="module")
def tiled():
    """n = 256, (8, 2): from 32 samples on the tiled key-switch forms.  With it the ring words and the reference of 1,025
    samples in index order, of which every smaller count is a prefix"""
    pp, ks = _keyset(N_TILED)
    ring = random_ring(np.random.default_rng(11), 2, pp.N)
    ref = U.unpack_ref(ks.ksk(), pp, ring, np.arange(pp.N + 1))
    yield pp, ks, ring, ref
    ks.close()


LARGEST_NRING = [1]             # the most ring samples any unpack of this file was given (the P128 fixture and tests use 1)


def random_ring(rng, nring, N):
    LARGEST_NRING[0] = max(LARGEST_NRING[0], nring)
    return U.random_ring(rng, nring, N)


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def ks_forms(api):
    s = api.stats()
    return np.array([s["ks_pergate_launches"], s["ks_strip_launches"] + s["ks_index_launches"]])


# ---- the extract kernel ----
def test_extract_kernel_against_the_definition(small):
    """e = 0, e = N - 1, a repeat, a descending run, a mask polynomial of INT32_MIN (its negation wraps to itself), and
    more rows than one workgroup round -- the kernel's rows alone, no key switch"""
    from peba1_amd import api
    pp, ks = small
    N = pp.N
    rng = np.random.default_rng(1)
    ring = random_ring(rng, 3, N)
    ring[1, 0, :] = U.I32_MIN
    index = np.concatenate([[0, N - 1, N - 1, N, N + 5, 2 * N - 1, 2 * N, 3 * N - 1], np.arange(3 * N - 1, 3 * N - 41, -1),
                            rng.integers(0, 3 * N, 700)])
    before = api.unpack_stats()
    assert_words(api.kernel_ring_extract(ks, ring, index), U.extract_ref(ring, index, N), "extract, listed")
    assert_words(api.kernel_ring_extract(ks, ring, count=N + 3), U.extract_ref(ring, np.arange(N + 3), N), "extract, index NULL")
    after = api.unpack_stats()
    assert after["unpack_launches"] - before["unpack_launches"] == 2 and after["unpacked_samples"] == before["unpacked_samples"]


# ---- the full unpack, word for word ----
@pytest.mark.parametrize("count", [1, 31, 32, 1024, 1025])
def test_counts_around_the_tiled_key_switch(tiled, count):
    """below two tiles the per-gate key switch, from 32 on a tiled form; 1,025 reaches into the second ring sample"""
    from peba1_amd import api
    pp, ks, ring, ref = tiled
    r = api.CiphertextArray(pp, count)
    forms = ks_forms(api)
    api.unpack(ring, ks, r, count=count)
    assert list(ks_forms(api) - forms) == ([1, 0] if count < 32 else [0, 1])
    assert_words(r.words(), ref[:count], ("tiled set", count))
    r.close()


def test_chunk_boundary_and_the_statistics(small):
    """8,200 samples of nine ring samples, any order, with repeats: two chunks (8,192 and 8); the counters move by the
    samples, the launches and the key switches"""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(2)
    ring = random_ring(rng, 9, pp.N)
    index = rng.integers(0, 9 * pp.N, 8200)
    r = api.CiphertextArray(pp, 8200)
    s0, u0 = api.stats(), api.unpack_stats()
    api.unpack(ring, ks, r, index=index)
    s1, u1 = api.stats(), api.unpack_stats()
    assert u1["unpacked_samples"] - u0["unpacked_samples"] == 8200 and u1["unpack_launches"] - u0["unpack_launches"] == 2
    assert s1["keyswitches"] - s0["keyswitches"] == 8200 and s1["blind_rotates"] == s0["blind_rotates"]
    assert s1["flushes"] == s0["flushes"]
    assert_words(r.words(), U.unpack_ref(ks.ksk(), pp, ring, index), "8,200 across the chunk boundary")
    r.close()


def test_per_gate_decomposition():
    """(ks_t, ks_basebit) = (3, 7): a key switch only the per-gate kernel runs, wide enough for two tiles"""
    from peba1_amd import api
    pp, ks = _keyset(10, ks=(3, 7))
    rng = np.random.default_rng(3)
    ring = random_ring(rng, 2, pp.N)
    index = rng.integers(0, 2 * pp.N, 40)
    r = api.CiphertextArray(pp, 40)
    forms = ks_forms(api)
    api.unpack(ring, ks, r, index=index)
    assert list(ks_forms(api) - forms) == [1, 0]
    assert_words(r.words(), U.unpack_ref(ks.ksk(), pp, ring, index), "(3, 7)")
    r.close()
    ks.close()


def test_n2048():
    """a ring of 2,048: two groups per lane in the extract kernel, rows of 2,049 words in the key switch"""
    from peba1_amd import api
    pp, ks = _keyset(10, N=2048, gadget=(3, 6))
    assert pp.N == 2048
    rng = np.random.default_rng(4)
    ring = random_ring(rng, 2, pp.N)
    ring[0, 0, :] = U.I32_MIN
    index = np.concatenate([[0, 2047, 2048, 4095, 1024, 1023], rng.integers(0, 4096, 64)])
    assert_words(api.kernel_ring_extract(ks, ring, index), U.extract_ref(ring, index, pp.N), "N2048 extract")
    r = api.CiphertextArray(pp, len(index))
    api.unpack(ring, ks, r, index=index)
    assert_words(r.words(), U.unpack_ref(ks.ksk(), pp, ring, index), "N2048")
    r.close()
    ks.close()


def test_scattered_form_writes_several_arrays(small):
    """results in three arrays of different lengths, interleaved; a sample given twice ends with its last value; samples
    the call does not name keep theirs"""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(5)
    ring = random_ring(rng, 2, pp.N)
    a, b, c = api.CiphertextArray(pp, 3), api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 7)
    held = c.words()[6].copy()
    targets = [(c, 0), (a, 2), (b, 0), (c, 5), (a, 0), (c, 1), (a, 1), (c, 2), (c, 3), (c, 4), (c, 0)]
    index = rng.integers(0, 2 * pp.N, len(targets))
    api.unpack(ring, ks, [arr.at(j) for arr, j in targets], index=index)
    ref = U.unpack_ref(ks.ksk(), pp, ring, index)
    words = {id(a): a.words(), id(b): b.words(), id(c): c.words()}
    for row, (arr, j) in enumerate(targets):
        if (arr, j) != (c, 0) or row == len(targets) - 1:
            assert_words(words[id(arr)][j], ref[row], ("scattered", row))
    assert_words(c.words()[6], held, "a sample the call did not name")
    for o in (a, b, c):
        o.close()


def test_immediate_mode_refreshes_the_host_mirrors(small):
    from peba1_amd import api
    pp, ks = small
    ring = random_ring(np.random.default_rng(6), 1, pp.N)
    index = np.array([7, 0, 1023])
    r = api.CiphertextArray(pp, 3)
    api.set_deferred(False)
    try:
        api.unpack(ring, ks, r, index=index)
        mirror = np.array([list(r.at(j).contents.a[:pp.n]) + [r.at(j).contents.b] for j in range(3)], dtype=np.int32)
    finally:
        api.set_deferred(True)
    assert_words(mirror, U.unpack_ref(ks.ksk(), pp, ring, index), "host mirrors on return")
    r.close()


def test_device_form_agrees_with_the_host_form(L, small):
    """the ring words go up through a torch tensor; the call returns with the work enqueued and the stream is waited for"""
    import torch
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(7)
    ring = random_ring(rng, 2, pp.N)
    index = rng.integers(0, 2 * pp.N, 100)
    host, devr = api.CiphertextArray(pp, 100), api.CiphertextArray(pp, 100)
    api.unpack(ring, ks, host, index=index)
    dev = torch.from_numpy(ring.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    api.unpack_device(dev.data_ptr(), 2, ks, devr, index=index)
    api.unpack_device(dev.data_ptr(), 2, ks, devr, count=5, first=95)         # a second one behind it, nobody waited yet
    assert L.tfhe_hip_stream_sync() == 0
    want = host.words()
    got = devr.words()
    assert_words(got[:95], want[:95], "device form")
    assert_words(got[95:], U.unpack_ref(ks.ksk(), pp, ring, np.arange(5)), "device form, index NULL")
    assert api.last_error() == ""
    del dev
    for o in (host, devr):
        o.close()


def test_staging_area_wraps_under_stream_ordered_calls(L, small):
    """Twelve calls back to back with no host wait in between -- four rounds of a device-form import of 12,000 samples, a
    device-form unpack of 12,000 and a device-form export of the imported samples -- every one with a slot or index list
    of its own.  Their host lists (48 KB, 240 KB and 48 KB a round) pass through the engine's pinned staging area, which
    starts at 256 KB: it starts again from offset 0 at least four times and grows never.  A list written over before the
    device had read it would move other words: every exported word is the imported one, every unpacked word the
    reference's.  The pool is grown beforehand, so that no growth (a host wait) falls into the sequence."""
    import torch
    from peba1_amd import api
    pp, ks = small
    count, rounds = 12000, 4
    rng = np.random.default_rng(15)
    for warm in [api.CiphertextArray(pp, 50000) for _ in range(2)]:
        warm.set_words(np.zeros((50000, pp.words), dtype=np.int32))
        warm.close()
    ring = random_ring(rng, 2, pp.N)
    ref = U.unpack_ref(ks.ksk(), pp, ring, np.arange(2 * pp.N))          # every coefficient once; a list picks its rows
    words = [rng.integers(U.I32_MIN, U.I32_MAX + 1, (count, pp.words), dtype=np.int64).astype(np.int32) for _ in range(rounds)]
    index = [rng.integers(0, 2 * pp.N, count).astype(np.int32) for _ in range(rounds)]
    dring = torch.from_numpy(ring.reshape(-1)).to("cuda:0")
    src = [torch.from_numpy(w.reshape(-1)).to("cuda:0") for w in words]
    dst = [torch.zeros(count * pp.words, dtype=torch.int32, device="cuda:0") for _ in range(rounds)]
    arrays = [api.CiphertextArray(pp, count) for _ in range(rounds)]
    results = [api.CiphertextArray(pp, count) for _ in range(rounds)]
    torch.cuda.synchronize()
    for r in range(rounds):
        assert L.tfhe_hip_import_samples_device_async(arrays[r].ptr, count, pp.ptr, C.c_void_p(src[r].data_ptr())) == 0
        api.unpack_device(dring.data_ptr(), 2, ks, results[r], index=index[r])
        assert L.tfhe_hip_export_samples_device_async(arrays[r].ptr, count, pp.ptr, C.c_void_p(dst[r].data_ptr())) == 0
    assert L.tfhe_hip_stream_sync() == 0
    assert api.last_error() == ""
    for r in range(rounds):
        assert_words(dst[r].cpu().numpy().reshape(count, pp.words), words[r], ("exported against imported, round", r))
        assert_words(results[r].words(), ref[index[r]], ("unpacked, round", r))
    del dring, src, dst
    for o in arrays + results:
        o.close()


def test_an_export_or_import_of_more_than_65536_samples_is_refused(L, small):
    """65,537 samples in one export: -1 and the message, the destination, the samples and the statistics as they were;
    65,536 of them go through.  An import of 65,537, from host or device words: refused the same way before a sample is
    touched -- every sample keeps its slot and its value"""
    import torch
    from peba1_amd import api
    pp, ks = small
    most = 1 << 16
    r = api.CiphertextArray(pp, most + 1)
    tail = np.random.default_rng(16).integers(U.I32_MIN, U.I32_MAX + 1, (8, pp.words), dtype=np.int64).astype(np.int32)
    tail_p = tail.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.tfhe_hip_import_samples(r.at(most - 7), 8, pp.ptr, tail_p) == 0

    def tail_words():
        out = np.zeros((8, pp.words), dtype=np.int32)
        assert L.tfhe_hip_export_samples(r.at(most - 7), 8, pp.ptr, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        return out

    dst = torch.full(((most + 1) * pp.words,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.tfhe_hip_export_samples_device(r.ptr, most, pp.ptr, C.c_void_p(dst.data_ptr())) == 0
    got = dst.cpu().numpy()
    assert_words(got[(most - 7) * pp.words:most * pp.words].reshape(7, pp.words), tail[:7], "the last of 65,536")
    assert (got[most * pp.words:] == 0x5A5A5A5A).all()
    dst.fill_(0x5A5A5A5A)
    torch.cuda.synchronize()
    before = api.stats()
    for entry in (L.tfhe_hip_export_samples_device, L.tfhe_hip_export_samples_device_async):
        assert entry(r.ptr, most + 1, pp.ptr, C.c_void_p(dst.data_ptr())) == -1
        assert api.last_error() == "too many samples in one packed transfer"
        L.tfhe_hip_clear_error()
    assert L.tfhe_hip_stream_sync() == 0
    assert (dst.cpu().numpy() == 0x5A5A5A5A).all() and api.stats() == before
    assert_words(tail_words(), tail, "samples after the refused export")
    slots = [r.at(j).contents.slot for j in range(most + 1)]
    host = np.full(((most + 1), pp.words), 0x33333333, dtype=np.int32)
    for entry, src in ((L.tfhe_hip_import_samples, host.ctypes.data_as(C.POINTER(C.c_int32))),
                       (L.tfhe_hip_import_samples_device, C.c_void_p(dst.data_ptr())),
                       (L.tfhe_hip_import_samples_device_async, C.c_void_p(dst.data_ptr()))):
        assert entry(r.ptr, most + 1, pp.ptr, src) == -1
        assert api.last_error() == "too many samples in one packed transfer"
        L.tfhe_hip_clear_error()
    assert [r.at(j).contents.slot for j in range(most + 1)] == slots and api.stats() == before
    assert_words(tail_words(), tail, "samples after the refused imports")
    del dst
    r.close()


def test_exhausted_device_refuses_without_effect(L, small):
    """no room for the call's scratch: -1, the message, results with their old values and slots; fine once there is room.
    The scratch only grows, by half again plus 4 KB beyond what a call needs, and this file holds every caller of the unpack
    in the suite: twice the most ring samples any of them was given so far, plus four, is more than the engine holds,
    so this call has to allocate whatever ran before it."""
    from peba1_amd import api
    pp, ks = small
    rng = np.random.default_rng(8)
    nring = 2 * LARGEST_NRING[0] + 4
    assert nring * 2 * pp.N * 4 > 1.5 * LARGEST_NRING[0] * 2 * pp.N * 4 + 4096
    ring = random_ring(rng, nring, pp.N)
    index = rng.integers(0, nring * pp.N, 50)
    r = api.CiphertextArray(pp, 50).set_words(rng.integers(U.I32_MIN, U.I32_MAX + 1, (50, pp.words)).astype(np.int32))
    held, slots = r.words().copy(), [r.at(j).contents.slot for j in range(50)]
    before = api.unpack_stats()
    L.tfhe_hip_test_set_alloc_cap(1)
    rc = L.tfhe_hip_unpack_samples(ks.cloud, ring.ctypes.data_as(C.POINTER(C.c_int32)), nring,
                                   index.astype(np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 50, r.ptr)
    L.tfhe_hip_test_set_alloc_cap(0)
    assert rc == -1 and "out of device memory" in api.last_error()
    L.tfhe_hip_clear_error()
    assert [r.at(j).contents.slot for j in range(50)] == slots and api.unpack_stats() == before
    assert_words(r.words(), held, "results after the refused call")
    api.unpack(ring, ks, r, index=index)
    assert_words(r.words(), U.unpack_ref(ks.ksk(), pp, ring, index), "after the cap was lifted")
    r.close()


def test_exhausted_slot_pool_refuses_without_effect(L, monkeypatch):
    """a pool of 64 slots (TFHE_HIP_POOL_SLOTS is read when the pool of a ciphertext shape is made; no other test of the
    suite uses LWE width 77, so this pool is made here): an unpack of 100 is refused with the slots it had taken given
    back -- the results keep values and slots, and an unpack of 40 afterwards finds room and writes the right words"""
    from peba1_amd import api
    monkeypatch.setenv("TFHE_HIP_POOL_SLOTS", "64")
    pp, ks = _keyset(77)
    rng = np.random.default_rng(14)
    ring = random_ring(rng, 1, pp.N)
    index = rng.integers(0, pp.N, 100)
    r = api.CiphertextArray(pp, 100)
    api.unpack(ring, ks, r, index=index[:8])                       # eight results hold slots of the small pool
    held, slots = r.words()[:8].copy(), [r.at(j).contents.slot for j in range(100)]
    before, stats = api.unpack_stats(), api.stats()
    rc = L.tfhe_hip_unpack_samples(ks.cloud, ring.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                   index.astype(np.int32).ctypes.data_as(C.POINTER(C.c_int32)), 100, r.ptr)
    assert rc == -1 and "slot pool exhausted (64 slots)" in api.last_error()
    L.tfhe_hip_clear_error()
    assert [r.at(j).contents.slot for j in range(100)] == slots and api.unpack_stats() == before
    assert api.stats()["keyswitches"] == stats["keyswitches"]
    assert_words(r.words()[:8], held, "results after the refused call")
    api.unpack(ring, ks, r, index=index[:40])                      # the refused call gave every slot back: 40 + 2 + 8 fit in 64
    assert_words(r.words()[:40], U.unpack_ref(ks.ksk(), pp, ring, index[:40]), "after the refusal")
    r.close()
    ks.close()


def test_round_trip_through_the_packing_key_switch(small):
    """bits -> one ring sample -> 1,024 LWE samples on the device -> one ring sample under a seeded packing key -> bits"""
    from peba1_amd import api
    pp, ks = small
    bits = np.random.default_rng(9).integers(0, 2, pp.N)
    words = api.ring_encrypt_bits(bits, ks, seed=0x51)
    r = api.CiphertextArray(pp, pp.N)
    api.unpack(words, ks, r, count=pp.N)
    pk = api.PackingKey(ks, seed=0x0DDB)
    back = api.pack(pk, r, pp.N, ks)
    assert list(api.packed_decrypt(back, pp.N, ks)) == list(bits)
    assert not np.array_equal(back, words)
    pk.close()
    r.close()


# ---- P128 ----
@pytest.fixture(scope="module")
def p128_unpacked(p128_keys):
    """1,024 bits encrypted by ring_encrypt_bits at P128 and unpacked once: (bits, ring words, results, their words)"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits = np.random.default_rng(10).integers(0, 2, pp.N)
    ring = api.ring_encrypt_bits(bits, ks, seed=0xB175)
    r = api.CiphertextArray(pp, pp.N)
    api.unpack(ring, ks, r, count=pp.N)
    yield bits, ring, r, r.words()
    r.close()


def test_p128_words(p128_keys, p128_unpacked):
    pp, ks, _ = p128_keys
    bits, ring, r, words = p128_unpacked
    assert_words(words, U.unpack_ref(ks.ksk(), pp, ring, np.arange(pp.N)), "P128, 1,024")


def test_p128_all_bits_decrypt_inside_an_operand_margin(p128_keys, p128_unpacked, capsys):
    """all 1,024 decrypt right and the largest phase error against +-1/8 is below 1/16, the share of a two-input gate's
    1/8 margin that one operand may use; printed beside the sigma computed in the header (2.8e-3)"""
    pp, ks, _ = p128_keys
    bits, ring, r, words = p128_unpacked
    assert list(r.decrypt(ks)) == list(bits)
    ph = U.lwe_phases(words, ks.lwe_key()).astype(np.float64) / 2.0 ** 32
    err = np.abs(ph - np.where(bits == 1, 0.125, -0.125)).max()
    sigma = U.unpack_variance(pp.N, pp.ks_t, pp.ks_basebit, U.STDEVS[0], U.STDEVS[1]) ** 0.5
    with capsys.disabled():
        print("\nunpack P128 count 1024: largest |phase error| %.3e, computed sigma %.3e (%.2f sigma)" % (err, sigma, err / sigma))
    assert abs(sigma - 2.8e-3) < 1e-4
    assert err < 1.0 / 16


def test_p128_gates_of_unpacked_operands(p128_keys):
    """bootsAND and bootsXOR of two unpacked arrays of 256 -- coefficients 0..255 and 256..511 of one ring sample"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits = np.random.default_rng(12).integers(0, 2, 512)
    ring = api.ring_encrypt_bits(bits, ks, seed=0xA2D)
    a, b = api.CiphertextArray(pp, 256), api.CiphertextArray(pp, 256)
    api.unpack(ring, ks, a, count=256)
    api.unpack(ring, ks, b, index=np.arange(256, 512))
    x, y = api.CiphertextArray(pp, 256), api.CiphertextArray(pp, 256)
    api.gate_batch("AND", x, a, b, ks)
    api.gate_batch("XOR", y, a, b, ks)
    assert list(x.decrypt(ks)) == list(bits[:256] & bits[256:]) and list(y.decrypt(ks)) == list(bits[:256] ^ bits[256:])
    for o in (a, b, x, y):
        o.close()


def test_p128_recorded_gates_stay_pending_across_an_unpack(L, p128_keys):
    """gates recorded before an unpack are neither run nor lost by it, and afterwards produce the oracle's words"""
    from peba1_amd import api
    pp, ks, oks = p128_keys
    L.tfhe_hip_set_encrypt_seed(77)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    g, r = api.CiphertextArray(pp, 3), api.CiphertextArray(pp, 5)
    wa, wb = a.words(), b.words()
    api.flush()
    ring = random_ring(np.random.default_rng(13), 1, pp.N)
    index = np.array([3, 1023, 0, 3, 512])
    before = api.stats()
    api.gate_batch("AND", g, a, b, ks)
    api.unpack(ring, ks, r, index=index)
    after = api.stats()
    assert after["blind_rotates"] == before["blind_rotates"] and after["flushes"] == before["flushes"]      # still recorded
    assert after["keyswitches"] - before["keyswitches"] == 5
    assert_words(r.words(), U.unpack_ref(ks.ksk(), pp, ring, index), "unpacked beside pending gates")
    got = g.words()
    assert api.stats()["blind_rotates"] - before["blind_rotates"] == 3
    for i in range(3):
        assert (got[i] == oks.gate("AND", wa[i], wb[i])).all(), i
    assert list(g.decrypt(ks)) == [0, 1, 0]
    for o in (a, b, g, r):
        o.close()


def test_template_from_ring_matches_like_a_template_of_samples(L, p128_keys):
    """a 4-slot template that arrived as one ring sample, against a probe through function_f_fast: the same match bit as the
    same template encrypted sample by sample, for a genuine and an impostor probe"""
    from peba1_amd import api, circuits, identify
    pp, ks, _ = p128_keys
    L.tfhe_hip_set_encrypt_seed(4)
    tmpl, bitsize = [17, 200, 3, 96], 8
    ring = circuits.ring_encrypt_vector(tmpl, bitsize, ks, seed=0x7E)
    from_ring = identify.unpack_templates([ring], pp, len(tmpl), bitsize, ks)[0]
    assert [circuits.decrypt_number(s, ks) for s in from_ring.slots] == tmpl
    by_sample = circuits.EncryptedVector(pp, tmpl, bitsize, ks)
    bound = circuits.encrypt_number(pp, 50, 3 * bitsize, ks)
    for probe, want in (([18, 199, 4, 95], 0), ([90, 13, 250, 7], 1)):
        S = circuits.EncryptedVector(pp, probe, bitsize, ks)
        ra, rb = api.CiphertextArray(pp, 3 * bitsize), api.CiphertextArray(pp, 3 * bitsize)
        circuits.function_f_fast(ra, S, from_ring, bound, bitsize, ks)
        circuits.function_f_fast(rb, S, by_sample, bound, bitsize, ks)
        assert ra.decrypt(ks).tolist() == rb.decrypt(ks).tolist() == [want] + [0] * (3 * bitsize - 1)
