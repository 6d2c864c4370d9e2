"""Encrypted inner products on the GPU.  The product-and-extract kernel is compared word for word with the numpy restatement
(tests/inner_common.py over tests/select_common.py), with the CMUX kernel on d1 = c, d0 = 0 and, through the public entry,
with the unpack of the raw product; the Hamming route on top (identify.match_by_inner) is checked by what it means, outside
the computed decision band; the public entry's refusals leave slots and values as they were."""
import ctypes as C

import numpy as np
import pytest

import inner_common as K
import select_common as S

pytestmark = pytest.mark.gpu


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


def params_of(name, n=10):
    from peba1_amd import api
    N, l, Bgbit = S.SETS[name]
    return api.ParameterSet(custom=S.custom_tuple(n, N=N, gadget=(l, Bgbit)))


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---- the kernel, word for word ----
class _RawCases:
    """per parameter set, made at first use: a selector of two samples of random words (polynomial samples are arbitrary
    words), the SECOND of which is used -- its image lies one sample into the selector's --, three random ring samples (two
    at N = 2,048) and their products by the restatement"""

    def __init__(self):
        self.made = {}

    def get(self, name):
        from peba1_amd import api
        if name not in self.made:
            N, l, Bgbit = S.SETS[name]
            pp = params_of(name)
            rng = np.random.default_rng(911 + N + l)
            words = S.random_ring(rng, 2 * 2 * l, N).reshape(2, 2 * l, 2, N)
            ring = S.random_ring(rng, 3 if N == 1024 else 2, N)
            want = np.stack([K.product(words[1], c, l, Bgbit) for c in ring])
            self.made[name] = (pp, api.Selector(pp, words), ring, want)
        return self.made[name]


@pytest.fixture(scope="module")
def raw_cases():
    cases = _RawCases()
    yield cases
    for _, sel, _, _ in cases.made.values():
        sel.close()


@pytest.mark.parametrize("name", list(S.SETS))
def test_raw_product_against_the_restatement_and_the_cmux_kernel(raw_cases, name):
    from peba1_amd import api
    pp, sel, ring, want = raw_cases.get(name)
    N = pp.N
    got = api.kernel_ring_product(sel, 1, ring).reshape(-1, 2, N)
    assert_words(got, want, (name, "product against the restatement"))
    cm = api.kernel_ring_cmux(sel, 1, ring, np.zeros_like(ring)).reshape(-1, 2, N)
    assert_words(got, cm, (name, "product against CMUX(G, c, 0)"))
    assert_words(api.kernel_ring_product(sel, 1, ring[:1]).reshape(-1, 2, N), want[:1], (name, "one sample"))


ROWS = [("P128", 1024, 3), ("P128", 128, 19), ("P128", 16, 131), ("P128", 1, 5), ("P128", 1, 2051), ("P128", 128, 24),
        ("P80", 128, 19), ("P2048", 256, 11)]                  # (set, w, M): M = 2 S + 3 where three samples hold it


def test_rows_of_more_than_one_chunk_against_the_restatement():
    """w = 1, R = 9, M = 8,192 + 5: the second chunk starts at sample 8 and holds five rows -- the per-chunk operand
    offset and workgroup count of the engine's loop"""
    from peba1_amd import api
    N, l, Bgbit = S.SETS["P128"]
    pp = params_of("P128")
    rng = np.random.default_rng(4242)
    words = S.random_ring(rng, 2 * l, N).reshape(1, 2 * l, 2, N)
    ring = S.random_ring(rng, 9, N)
    sel = api.Selector(pp, words)
    M = 8192 + 5
    got = api.kernel_ring_inner_rows(sel, 0, ring, M, 1)
    want = np.stack([K.product(words[0], c, l, Bgbit) for c in ring])
    assert_words(got, K.inner_rows(want, M, 1), "rows of two chunks")
    sel.close()


@pytest.mark.parametrize("name,w,M", ROWS)
def test_extracted_rows_against_the_restatement(raw_cases, name, w, M):
    from peba1_amd import api
    pp, sel, ring, want = raw_cases.get(name)
    R = api.lookup_samples(pp, M, w)
    assert R <= len(ring)
    got = api.kernel_ring_inner_rows(sel, 1, ring[:R], M, w)
    assert_words(got, K.inner_rows(want[:R], M, w), (name, w, M))
    # the padded rows as the kernel stored them: three zeros behind every body, nothing behind row M - 1
    rows = api.extract_rows(pp.N + 4)
    assert rows.shape[0] == M and (rows[:, pp.N + 1:] == 0).all()
    assert_words(rows[:, :pp.N + 1], got, "padded rows")


@pytest.mark.parametrize("name", list(S.SETS))
def test_crafted_worst_case_reaches_the_crt_bounds_left_side(name):
    """selector rows all 0x80000000 against a ring sample whose digits are all -Bg/2: every product of the sum has the
    largest magnitude and one sign, coefficient N - 1 is (k+1) l N (Bg/2) 2^31 exactly (closed form in Python integers)"""
    from peba1_amd import api
    N, l, Bgbit = S.SETS[name]
    pp = params_of(name)
    word = S.extreme_difference(l, Bgbit, "min")
    c = S.to_i32(np.full((1, 2, N), word, dtype=np.int64))
    assert (S.decompose(c[0, 0], l, Bgbit) == -2 ** (Bgbit - 1)).all()
    want, most = S.extreme_closed_form(N, l, S.I32_MIN, -2 ** (Bgbit - 1), np.zeros((2, N), dtype=np.int64))
    assert most == 2 * l * N * 2 ** (Bgbit - 1) * 2 ** 31 < S.CRT_EXACT_LIMIT
    sel = api.Selector(pp, np.full((1, 2 * l, 2, N), S.I32_MIN, dtype=np.int32))
    assert_words(api.kernel_ring_product(sel, 0, c).reshape(2, N), want, (name, "product"))
    assert_words(api.kernel_ring_inner_rows(sel, 0, c, N // 128, 128), K.inner_rows(want[None], N // 128, 128), (name, "rows"))
    sel.close()


# ---- the public entry ----
@pytest.fixture(scope="module")
def small_keys():
    from peba1_amd import api
    pp = params_of("P128", n=12)
    ks = api.SecretKeySet(pp, 0x1AE7, device=True)
    yield pp, ks
    ks.close()


@pytest.mark.parametrize("w,M", [(128, 19), (1024, 2), (16, 70), (1, 8192 + 5)])       # the last: two chunks, two key-switch plans
def test_ring_inner_equals_the_unpack_of_the_raw_product_host_and_device_forms(L, small_keys, w, M):
    import torch
    from peba1_amd import api
    pp, ks = small_keys
    N, l, Bgbit = S.SETS["P128"]
    rng = np.random.default_rng(5 + w)
    words = S.random_ring(rng, 2 * 2 * l, N).reshape(2, 2 * l, 2, N)
    R = api.lookup_samples(pp, M, w)
    ring = S.random_ring(rng, R, N)
    sel = api.Selector(pp, words)
    L.tfhe_hip_clear_error()                                      # (the channel keeps what an earlier test provoked)
    prod = api.kernel_ring_product(sel, 1, ring)
    per = N // w
    index = [(i // per) * N + (i % per) * w for i in range(M)]
    want = api.CiphertextArray(pp, M)
    # (from device memory: the unpack's host-side ring buffer stays as small as tests/test_gpu_unpack.py expects to find it)
    dprod = torch.from_numpy(np.ascontiguousarray(prod.reshape(-1))).to("cuda:0")
    torch.cuda.synchronize()
    api.unpack_device(dprod.data_ptr(), R, ks, want, index=index)
    assert L.tfhe_hip_stream_sync() == 0
    del dprod
    before = api.stats()
    host = api.CiphertextArray(pp, M)
    api.ring_inner(sel, 1, ring, M, w, ks, host)
    assert api.stats()["keyswitches"] - before["keyswitches"] == M
    assert sorted(host.at(j).contents.slot for j in range(M)) == sorted(set(host.at(j).contents.slot for j in range(M)))
    assert min(host.at(j).contents.slot for j in range(M)) >= 0
    assert_words(host.words(), want.words(), ("host form", w, M))
    dev = torch.from_numpy(ring.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.CiphertextArray(pp, M)
    api.ring_inner(sel, 1, dev, M, w, ks, out, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.words(), want.words(), ("device form", w, M))
    assert_words(dev.cpu().numpy(), ring.reshape(-1), "the resident gallery is read only")
    assert api.last_error() == ""
    del dev
    sel.close()
    for o in (want, host, out):
        o.close()


def test_recorded_gates_stay_pending_across_ring_inner(L, small_keys):
    from peba1_amd import api
    pp, ks = small_keys
    N, l, Bgbit = S.SETS["P128"]
    rng = np.random.default_rng(77)
    sel = api.Selector(pp, S.random_ring(rng, 2 * l, N).reshape(1, 2 * l, 2, N))
    ring = S.random_ring(rng, 1, N)
    L.tfhe_hip_set_encrypt_seed(31)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    g = api.CiphertextArray(pp, 3)
    api.gate_batch("AND", g, a, b, ks)
    before = api.stats()
    r = api.CiphertextArray(pp, 8)
    api.ring_inner(sel, 0, ring, 8, 128, ks, r)
    after = api.stats()
    for f in ("blind_rotates", "levels", "flushes", "br_launches"):
        assert after[f] == before[f], f
    assert list(g.decrypt(ks)) == [0, 1, 0] and api.stats()["blind_rotates"] - before["blind_rotates"] == 3
    sel.close()
    for o in (a, b, g, r):
        o.close()


def test_public_entry_refusals_leave_slots_and_values(L, small_keys, monkeypatch):
    """on the device: misaligned device words, device memory exhausted (a selector used for the first time has to allocate
    its image), the slot pool exhausted (a pool of 64 slots of an LWE width no other test uses) -- each -1 with the message,
    the results with their values and slots; the same call goes through afterwards"""
    import torch
    from peba1_amd import api
    pp, ks = small_keys
    N, l, Bgbit = S.SETS["P128"]
    rng = np.random.default_rng(8)
    words = S.random_ring(rng, 2 * l, N).reshape(1, 2 * l, 2, N)
    ring = S.random_ring(rng, 2, N)
    r = api.CiphertextArray(pp, 12).set_words(rng.integers(S.I32_MIN, S.I32_MAX + 1, (12, pp.words)).astype(np.int32))
    held, slots = r.words().copy(), [r.at(j).contents.slot for j in range(12)]

    def unchanged(what):
        assert [r.at(j).contents.slot for j in range(12)] == slots, what
        assert_words(r.words(), held, what)

    sel = api.Selector(pp, words)                                 # (no image yet)
    flat = np.ascontiguousarray(ring.reshape(-1))
    stats = api.stats()
    L.tfhe_hip_test_set_alloc_cap(1)
    rc = L.tfhe_hip_ring_inner(sel.ptr, 0, ks.cloud, _i32p(flat), 12, 128, r.ptr)
    L.tfhe_hip_test_set_alloc_cap(0)
    assert rc == -1 and "out of device memory" in api.last_error(), api.last_error()
    L.tfhe_hip_clear_error()
    unchanged("device memory exhausted")
    assert api.stats()["keyswitches"] == stats["keyswitches"]
    dev = torch.zeros(2 * 2 * N + 4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = L.tfhe_hip_ring_inner_device(sel.ptr, 0, ks.cloud, C.c_void_p(dev.data_ptr() + 4), 12, 128, r.ptr)
    assert rc == -1 and "16-byte aligned" in api.last_error()
    L.tfhe_hip_clear_error()
    unchanged("misaligned device words")
    rc = L.tfhe_hip_ring_inner(sel.ptr, 1, ks.cloud, _i32p(flat), 12, 128, r.ptr)
    assert rc == -1 and "sample_index must be in 0..0" in api.last_error()
    L.tfhe_hip_clear_error()
    unchanged("sample_index outside the selector")
    api.ring_inner(sel, 0, ring, 12, 128, ks, r)
    prod = api.kernel_ring_product(sel, 0, ring)
    want = api.CiphertextArray(pp, 12)
    api.unpack(prod, ks, want, index=[(i // 8) * N + (i % 8) * 128 for i in range(12)])
    assert_words(r.words(), want.words(), "after the refusals")
    del dev
    # the slot pool
    monkeypatch.setenv("TFHE_HIP_POOL_SLOTS", "64")
    pp83 = params_of("P128", n=83)
    ks83 = api.SecretKeySet(pp83, 0x83, device=True)
    big = api.CiphertextArray(pp83, 100)
    api.ring_inner(sel, 0, ring[:1], 8, 128, ks83, big)           # eight results hold slots of the small pool
    held83, slots83 = big.words()[:8].copy(), [big.at(j).contents.slot for j in range(100)]
    ring13 = S.random_ring(rng, 13, N)
    flat13 = np.ascontiguousarray(ring13.reshape(-1))
    rc = L.tfhe_hip_ring_inner(sel.ptr, 0, ks83.cloud, _i32p(flat13), 100, 128, big.ptr)
    assert rc == -1 and "slot pool exhausted (64 slots)" in api.last_error(), api.last_error()
    L.tfhe_hip_clear_error()
    assert [big.at(j).contents.slot for j in range(100)] == slots83
    assert_words(big.words()[:8], held83, "results after the refused call")
    api.ring_inner(sel, 0, ring13[:5], 40, 128, ks83, big)
    assert api.last_error() == ""
    sel.close()
    ks83.close()
    for o in (r, want, big):
        o.close()


# ---- decrypt level at P128 ----
def _gallery_at_distances(rng, probe, distances):
    entries = []
    for d in distances:
        e = probe.copy()
        e[rng.choice(len(probe), d, replace=False)] ^= 1
        entries.append(e)
    return np.array(entries)


DECISIONS = [
    # (w, tau, distances): at most a quarter of the 24 entries inside the band |d - tau| < g (g = 12 at w = 128, 2 at 16)
    (128, 40, [0, 3, 9, 10, 15, 20, 24, 26, 28, 52, 53, 55, 60, 64, 70, 90, 100, 128, 35, 39, 40, 41, 45, 50]),
    (16, 6, [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 8, 9, 10, 12, 14, 16, 8, 11, 5, 6, 7, 6, 5, 7]),
]


@pytest.mark.parametrize("w,tau,distances", DECISIONS)
def test_p128_distances_before_the_key_switch_and_decisions_outside_the_band(p128_keys, capsys, w, tau, distances):
    """24 entries on both sides of the band.  The rows before the key switch, decrypted under the extracted ring key, plus
    the plain addend round to the exact Hamming distance for EVERY entry; match_by_inner is right for every entry with
    |d - tau| >= g (inner_decision_band); entries inside the band are reported, not asserted, and are at most a quarter"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    N = pp.N
    rng = np.random.default_rng(1000 + w)
    probe = rng.integers(0, 2, w)
    entries = _gallery_at_distances(rng, probe, distances)
    M = len(entries)
    assert M == 24 and [int((e ^ probe).sum()) for e in entries] == distances
    g = identify.inner_decision_band(pp, w)
    assert g == {128: 12, 16: 2}[w]
    outside = [i for i, d in enumerate(distances) if abs(d - tau) >= g]
    assert 4 * len(outside) >= 3 * M and any(distances[i] < tau for i in outside) and any(distances[i] > tau for i in outside)
    gallery = identify.pack_gallery_inner(entries, w, ks, seed=0x1A0 + w)
    tgsw, addend = identify.hamming_probe(probe, w, ks, seed=0x2B0 + w)
    sel = api.Selector(pp, tgsw)
    delta = identify.inner_delta(w)
    # before the key switch
    rows = api.kernel_ring_inner_rows(sel, 0, gallery, M, w)
    ph = K.row_phases(rows, ks.tlwe_key()).astype(np.int64) + int(probe.sum()) * delta
    err = ((ph - np.array(distances, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31) / 2.0 ** 32
    sigma = K.inner_variance(N, pp.l, pp.Bgbit, S.STDEVS[1], float(w), S.STDEVS[1] ** 2) ** 0.5
    with capsys.disabled():
        print("\ninner P128 w = %d, %d entries: largest |phase error| before the key switch %.3e = %.2f of the computed sigma %.3e "
              "(Delta / 2 = %.3e)" % (w, M, np.abs(err).max(), np.abs(err).max() / sigma, sigma, delta / 2.0 ** 33))
    assert [int(v) for v in np.rint(ph / float(delta))] == distances
    # the same gallery as tfhe_hip_ring_encrypt leaves it (NOT centred): the error is the header's truncation bias, to the same
    # 7 sigma -- the public entry computes the product as defined on the words it is given
    raw = S.to_i32(gallery.astype(np.int64) - 2 ** (31 - pp.l * pp.Bgbit))
    ph_raw = K.row_phases(api.kernel_ring_inner_rows(sel, 0, raw, M, w), ks.tlwe_key()).astype(np.int64) + int(probe.sum()) * delta
    err_raw = (ph_raw - np.array(distances, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31
    per = N // w
    bias = K.truncation_bias(K.probe_poly(1 - 2 * probe, N), ks.tlwe_key(), pp.l, pp.Bgbit)[[(i % per) * w for i in range(M)]]
    with capsys.disabled():
        print("inner P128 w = %d, gallery not centred: largest |phase error| %.3e, largest computed bias %.3e"
              % (w, np.abs(err_raw).max() / 2.0 ** 32, np.abs(bias).max() / 2.0 ** 32))
    assert np.abs(err_raw - bias).max() < 7 * sigma * 2 ** 32
    # the decisions
    bits = identify.match_by_inner(sel, gallery, M, w, addend, tau, ks)
    got = [int(b) for b in bits.decrypt(ks)]
    inside = [(distances[i], got[i]) for i in range(M) if i not in outside]
    with capsys.disabled():
        print("inner P128 w = %d, tau = %d, band g = %d: (distance, decision) inside the band, reported only: %s" % (w, tau, g, inside))
    for i in outside:
        assert got[i] == (1 if distances[i] <= tau else 0), (i, distances[i], got[i])
    sel.close()
    for o in (bits, addend):
        o.close()
