"""A ring sample times public polynomials on the GPU.  The product kernel and its fused extraction are compared word for word
with the numpy restatement (tests/public_common.py), the public entry with that restatement's key switch
(tests/ks_common.py); the Hamming route on top (identify.match_clear_gallery) is checked by what it means, outside the
computed decision band, and against the TGSW route on the same templates; the existing entries give the words they gave."""
import ctypes as C

import numpy as np
import pytest

import public_common as K

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


def params_of(N, n=10):
    from peba1_amd import api
    return api.ParameterSet(custom=K.custom_tuple(n, N=N, gadget=(3, 7) if N == 1024 else (3, 6)))


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---- the kernel, word for word ----
ROT = 129                    # the monomial X^ROT of the cases below
IDX_WORST, IDX_ONE, IDX_MONO = 3, 4, 5


class _RawCases:
    """per ring size, made at first use: a gallery of three random polynomials with coefficients in [-T, T] (both ends
    present), the all -T polynomial, 1 and X^ROT; three random ring samples; the products of the three pairs (reference
    computed once)"""

    def __init__(self):
        self.made = {}

    def get(self, name):
        from peba1_amd import api
        if name not in self.made:
            N = K.RINGS[name]
            T = K.max_coef(N)
            pp = params_of(N)
            rng = np.random.default_rng(1213 + N)
            polys = np.zeros((6, N), dtype=np.int64)
            polys[:3] = rng.integers(-T, T + 1, (3, N))
            polys[0, 0], polys[0, N - 1], polys[1, 1] = T, -T, -T
            polys[IDX_WORST] = -T
            polys[IDX_ONE, 0] = 1
            polys[IDX_MONO, ROT] = 1
            ring = K.random_ring(rng, 3, N)
            self.made[name] = (pp, api.PublicGallery(pp, polys), polys, ring, K.products(polys, ring, 0, 3))
        return self.made[name]


@pytest.fixture(scope="module")
def raw_cases():
    cases = _RawCases()
    yield cases
    for _, g, _, _, _ in cases.made.values():
        g.close()


@pytest.mark.parametrize("name", list(K.RINGS))
def test_raw_product_in_the_three_broadcast_forms(L, raw_cases, name):
    import torch
    from peba1_amd import api
    pp, g, polys, ring, pair = raw_cases.get(name)
    N = pp.N
    got = api.kernel_ring_public_product(g, ring, 0, 3).reshape(-1, 2, N)
    assert_words(got, pair, (name, "pairwise, count 3"))
    assert_words(api.kernel_ring_public_product(g, ring[1:2], 1, 1).reshape(-1, 2, N), pair[1:2], (name, "one pair"))
    one_poly = api.kernel_ring_public_product(g, ring, 2, 1).reshape(-1, 2, N)
    assert_words(one_poly, K.products(polys, ring, 2, 1), (name, "one polynomial over three samples"))
    one_sample = api.kernel_ring_public_product(g, ring[2:3], 0, 3).reshape(-1, 2, N)
    assert_words(one_sample, K.products(polys, ring[2:3], 0, 3), (name, "one sample under three polynomials"))
    assert_words(one_poly[2], pair[2], "the forms meet at (2, 2)")
    assert_words(one_sample[2], pair[2], "the forms meet at (2, 2)")
    # the public entry, host and device forms: the same words
    assert_words(api.ring_mul_public(g, ring, 0, 3).reshape(-1, 2, N), pair, (name, "public entry, host"))
    dev = torch.from_numpy(ring.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_mul_public(g, dev, 2, 1, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.cpu().numpy().reshape(-1, 2, N), one_poly, (name, "public entry, device"))
    assert_words(dev.cpu().numpy(), ring.reshape(-1), "the resident samples are read only")
    assert api.last_error() == ""
    del dev, out


@pytest.mark.parametrize("name", list(K.RINGS))
def test_worst_case_identity_and_monomial(raw_cases, name):
    """all q[j] = -T against words 0x80000000 reaches N T 2^31 at coefficient N - 1 (closed form in Python integers, below
    CRT_EXACT_LIMIT); q = 1 gives the sample back; q = X^r gives the lookup's monomial multiple with the sign of the
    exponent flipped: X^r (X^(-r) c) = c"""
    from peba1_amd import api
    pp, g, polys, ring, _ = raw_cases.get(name)
    N = pp.N
    coef, most = K.worst_case(N)
    assert most == N * K.max_coef(N) * 2 ** 31 < K.CRT_EXACT_LIMIT
    worst = np.full((1, 2, N), K.I32_MIN, dtype=np.int32)
    want = K.to_i32(np.array([v % 2 ** 32 for v in coef], dtype=np.int64))
    got = api.kernel_ring_public_product(g, worst, IDX_WORST, 1).reshape(2, N)
    assert_words(got, np.stack([want, want]), (name, "worst case, closed form"))
    assert_words(got, K.product(polys[IDX_WORST], worst[0]), (name, "worst case, restatement"))
    # words at both ends of the signed range under the random polynomials
    ends = np.stack([np.full((2, N), K.I32_MAX, dtype=np.int32), np.full((2, N), K.I32_MIN, dtype=np.int32), ring[0]])
    assert_words(api.kernel_ring_public_product(g, ends, 0, 3).reshape(-1, 2, N), K.products(polys, ends, 0, 3), (name, "range ends"))
    assert_words(api.kernel_ring_public_product(g, ring, IDX_ONE, 1).reshape(-1, 2, N), ring, (name, "q = 1"))
    mono = api.kernel_ring_public_product(g, ring, IDX_MONO, 1).reshape(-1, 2, N)
    assert_words(mono, np.stack([K.monomial(c, ROT) for c in ring]), (name, "q = X^r"))
    back = np.stack([K.inverse_monomial(c, ROT) for c in ring])
    assert_words(api.kernel_ring_public_product(g, back, IDX_MONO, 1).reshape(-1, 2, N), ring, (name, "X^r (X^(-r) c) = c"))


ROWS = [("P128", 1), ("P128", 16), ("P128", 128), ("P128", 1024), ("P2048", 128)]


@pytest.mark.parametrize("name,w", ROWS)
def test_extracted_rows_against_the_restatement(L, raw_cases, name, w):
    """R = 2 polynomials, M = S + 1: the second workgroup writes one row.  Rows at or past M keep the sentinel; the padded
    rows as the kernel stored them carry three zeros behind every body"""
    from peba1_amd import api
    pp, g, polys, ring, _ = raw_cases.get(name)
    N = pp.N
    M = N // w + 1
    want = K.rows(polys, ring[0], M, w)
    assert_words(api.kernel_ring_public_rows(g, ring[0], M, w), want, (name, w))
    rows = api.extract_rows(N + 4)
    assert rows.shape[0] == M and (rows[:, N + 1:] == 0).all()
    assert_words(rows[:, :N + 1], want, "padded rows")
    held = np.full((M + 2, N + 1), 0x5A5A5A5A, dtype=np.int32)
    probe = np.ascontiguousarray(ring[0].reshape(-1))
    assert L.tfhe_hip_kernel_ring_public_rows(g.ptr, _i32p(probe), M, w, _i32p(held)) == 0
    assert_words(held[:M], want, "rows below M")
    assert (held[M:] == 0x5A5A5A5A).all()


# ---- the public entry ----
@pytest.fixture(scope="module")
def small_keys():
    from peba1_amd import api
    pp = params_of(1024, n=12)
    ks = api.SecretKeySet(pp, 0x1AE9, device=True)
    yield pp, ks
    ks.close()


# (1, 8192 + 5): nine polynomials and the one shape with a second chunk -- done / S != 0, a cut last workgroup, two key-switch plans
@pytest.mark.parametrize("w,M", [(128, 11), (1024, 2), (16, 70), (1, 8192 + 5)])
def test_ring_inner_public_equals_the_restatement_with_its_key_switch(L, small_keys, w, M):
    import torch
    from peba1_amd import api
    pp, ks = small_keys
    N = pp.N
    rng = np.random.default_rng(50 + w)
    R = api.lookup_samples(pp, M, w)
    polys = rng.integers(0, 2, (R, N))
    probe = K.random_ring(rng, 1, N)[0]
    g = api.PublicGallery(pp, polys)
    L.tfhe_hip_clear_error()                                      # (the channel keeps what an earlier test provoked)
    want = K.keyswitched(ks.ksk(), pp, K.rows(polys, probe, M, w))
    before = api.stats()
    host = api.CiphertextArray(pp, M)
    api.ring_inner_public(g, probe, M, w, ks, host)
    assert api.stats()["keyswitches"] - before["keyswitches"] == M
    slots = [host.at(j).contents.slot for j in range(M)]
    assert len(set(slots)) == M and min(slots) >= 0
    assert_words(host.words(), want, ("host form", w, M))
    dev = torch.from_numpy(probe.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.CiphertextArray(pp, M)
    api.ring_inner_public(g, dev, M, w, ks, out, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.words(), host.words(), ("device form equals host form", w, M))
    assert_words(dev.cpu().numpy(), probe.reshape(-1), "the resident probe is read only")
    assert api.last_error() == ""
    del dev
    g.close()
    for o in (host, out):
        o.close()


def test_recorded_gates_stay_pending_across_ring_inner_public(L, small_keys):
    from peba1_amd import api
    pp, ks = small_keys
    N = pp.N
    rng = np.random.default_rng(78)
    polys = rng.integers(0, 2, (1, N))
    g = api.PublicGallery(pp, polys)
    probe = K.random_ring(rng, 1, N)[0]
    L.tfhe_hip_set_encrypt_seed(31)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    gate = api.CiphertextArray(pp, 3)
    api.gate_batch("AND", gate, a, b, ks)
    before = api.stats()
    r = api.CiphertextArray(pp, 8)
    api.ring_inner_public(g, probe, 8, 128, ks, r)
    prod = api.ring_mul_public(g, probe[None])
    after = api.stats()
    for f in ("blind_rotates", "levels", "flushes", "br_launches"):
        assert after[f] == before[f], f
    assert list(gate.decrypt(ks)) == [0, 1, 0] and api.stats()["blind_rotates"] - before["blind_rotates"] == 3
    assert_words(prod.reshape(2, N), K.product(polys[0], probe), "product beside pending gates")
    assert_words(r.words(), K.keyswitched(ks.ksk(), pp, K.rows(polys, probe, 8, 128)), "inner products beside pending gates")
    g.close()
    for o in (a, b, gate, r):
        o.close()


# ---- decrypt level at P128 ----
W, TAU = 128, 40
DISTANCES = [0, 10, 20, 27, 53, 64, 100, 41]      # band g = 12 at w = 128: seven outside |d - tau| >= 12, on both sides; 41 inside


def _templates(rng, probe):
    entries = []
    for d in DISTANCES:
        e = probe.copy()
        e[rng.choice(len(probe), d, replace=False)] ^= 1
        entries.append(e)
    return np.array(entries)


@pytest.fixture(scope="module")
def p128_case(p128_keys):
    """eight 128-bit templates as ONE clear polynomial, a seeded probe sample and its addend (made once, shared)"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    rng = np.random.default_rng(1128)
    probe = rng.integers(0, 2, W)
    entries = _templates(rng, probe)
    assert [int((e ^ probe).sum()) for e in entries] == DISTANCES
    g_band = identify.inner_decision_band(pp, W)
    assert g_band == 12
    outside = [i for i, d in enumerate(DISTANCES) if abs(d - TAU) >= g_band]
    assert len(outside) >= 6 and any(DISTANCES[i] < TAU for i in outside) and any(DISTANCES[i] > TAU for i in outside)
    polys = identify.clear_gallery_polys(entries, W, pp.N)
    assert polys.shape == (1, pp.N)
    gal = api.PublicGallery(pp, polys)
    ring, addend = identify.hamming_probe_ring(probe, W, ks, seed=0x3C0)
    yield pp, ks, probe, entries, polys, gal, ring, addend, outside
    gal.close()
    addend.close()


def test_p128_distances_before_the_key_switch_and_decisions_outside_the_band(p128_case, capsys):
    """every phase before the key switch is within Delta / 2 of d Delta (a condition: the distance rounds exactly);
    match_clear_gallery is right for every template outside inner_decision_band; the one inside is reported, not asserted"""
    from peba1_amd import api, identify
    pp, ks, probe, entries, polys, gal, ring, addend, outside = p128_case
    M, delta = len(entries), identify.inner_delta(W)
    rows = api.kernel_ring_public_rows(gal, ring, M, W)
    assert_words(rows, K.rows(polys, ring.reshape(2, pp.N), M, W), "rows against the restatement")
    ph = K.U.extracted_phases(rows, ks.tlwe_key()).astype(np.int64) + int(probe.sum()) * delta
    err = (ph - np.array(DISTANCES, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31
    sigma = K.variance(float((polys[0].astype(np.int64) ** 2).sum()), K.BK_STDEVS["P128"] ** 2) ** 0.5
    with capsys.disabled():
        print("\npublic P128 w = %d, %d templates: largest |phase error| before the key switch %.3e = %.2f of the computed sigma %.3e "
              "(Delta / 2 = %.3e)" % (W, M, np.abs(err).max() / 2.0 ** 32, np.abs(err).max() / 2.0 ** 32 / sigma, sigma, delta / 2.0 ** 33))
    assert np.abs(err).max() < delta // 2
    assert [int(v) for v in np.rint(ph / float(delta))] == DISTANCES
    bits = identify.match_clear_gallery(gal, ring, M, W, addend, TAU, ks)
    got = [int(b) for b in bits.decrypt(ks)]
    inside = [(DISTANCES[i], got[i]) for i in range(M) if i not in outside]
    with capsys.disabled():
        print("public P128 w = %d, tau = %d, band g = 12: (distance, decision) inside the band, reported only: %s" % (W, TAU, inside))
    for i in outside:
        assert got[i] == (1 if DISTANCES[i] <= TAU else 0), (i, DISTANCES[i], got[i])
    # the probe resident on the card, and its seed-compressed form: the same words (evaluation draws nothing)
    import torch
    dev = torch.from_numpy(ring.copy()).to("cuda:0")
    torch.cuda.synchronize()
    bits_dev = identify.match_clear_gallery(gal, dev, M, W, addend, TAU, ks)
    assert_words(bits_dev.words(), bits.words(), "match bits from a resident probe")
    del dev
    packed, addend2 = identify.hamming_probe_ring(probe, W, ks, compressed=True, seed=0x3C2)
    assert packed.nbytes == 4136 and ring.nbytes == 8192
    bits_packed = identify.match_clear_gallery(gal, packed, M, W, addend, TAU, ks)
    got_packed = [int(b) for b in bits_packed.decrypt(ks)]
    for i in outside:
        assert got_packed[i] == got[i], (i, DISTANCES[i])
    for o in (bits, bits_dev, bits_packed, addend2):
        o.close()


def test_agreement_with_the_tgsw_route_on_the_same_templates(p128_case):
    """the same templates as a centred trivial gallery under a TGSW probe (tfhe_hip_kernel_ring_inner_rows) and as a clear
    gallery under a ring probe: both decrypt, before the key switch, to the same distances"""
    from peba1_amd import api, identify
    pp, ks, probe, entries, polys, gal, ring, addend, _ = p128_case
    M, delta = len(entries), identify.inner_delta(W)
    trivial = api.ring_trivial(pp, polys[0].astype(np.int64) * delta)
    centred = identify.inner_round_gallery(trivial[None, :], pp)
    tgsw, addend2 = identify.hamming_probe(probe, W, ks, seed=0x3C1)
    sel = api.Selector(pp, tgsw)
    old = K.U.extracted_phases(api.kernel_ring_inner_rows(sel, 0, centred, M, W), ks.tlwe_key()).astype(np.int64)
    new = K.U.extracted_phases(api.kernel_ring_public_rows(gal, ring, M, W), ks.tlwe_key()).astype(np.int64)
    d_old = [int(v) for v in np.rint((old + int(probe.sum()) * delta) / float(delta))]
    d_new = [int(v) for v in np.rint((new + int(probe.sum()) * delta) / float(delta))]
    assert d_old == d_new == DISTANCES
    sel.close()
    addend2.close()


def test_existing_entries_give_their_words_after_the_new_ones(L, small_keys):
    """tfhe_hip_ring_inner and tfhe_hip_ring_select on one small case: the same words before and after a product, a rows
    call and an inner-product call of this file's entries (which share the select's events and the unpack's row buffer)"""
    from peba1_amd import api
    import select_common as S
    pp, ks = small_keys
    N, l, Bgbit = S.SETS["P128"]
    rng = np.random.default_rng(404)
    words = S.random_ring(rng, 2 * l, N).reshape(1, 2 * l, 2, N)
    gallery = S.random_ring(rng, 2, N)
    sel = api.Selector(pp, words)

    def existing():
        r = api.CiphertextArray(pp, 9)
        api.ring_inner(sel, 0, gallery, 9, 128, ks, r)
        w = r.words().copy()
        r.close()
        return w, api.ring_select(sel, gallery).copy()

    inner0, select0 = existing()
    assert_words(select0.reshape(2, N), S.tree(words, gallery, l, Bgbit), "select against its restatement")
    g = api.PublicGallery(pp, rng.integers(0, 2, (2, N)))
    api.ring_mul_public(g, gallery)
    api.kernel_ring_public_rows(g, gallery[0], 9, 128)
    r = api.CiphertextArray(pp, 9)
    api.ring_inner_public(g, gallery[1], 9, 128, ks, r)
    inner1, select1 = existing()
    assert_words(inner1, inner0, "tfhe_hip_ring_inner")
    assert_words(select1, select0, "tfhe_hip_ring_select")
    assert api.last_error() == ""
    g.close()
    sel.close()
    r.close()
