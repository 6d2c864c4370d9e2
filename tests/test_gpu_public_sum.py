"""Public products over several ring samples on the GPU.  The summed product kernel and its fused extraction are compared
word for word with the numpy restatement (tests/public_sum_common.py) -- no tolerance anywhere at word level --, the public
entry with that restatement's rows under the key switch of tests/ks_common.py; the long and the masked Hamming routes on top
(peba1_amd.identify) are checked by what they mean, at distances chosen outside the computed decision band on purpose."""
import numpy as np
import pytest

import public_common as K
import public_sum_common as Q

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


# ---- the kernel, word for word ----
GROUPS = 5


@pytest.mark.parametrize("name,terms", [("P128", 1), ("P128", 2), ("P128", 3), ("P128", Q.MAX_TERMS), ("P2048", 2)])
def test_summed_products_against_the_restatement(L, name, terms):
    """random words, random coefficients with the per-term maxima summing to T or less (both ends present), 1 and 5 groups,
    a group range that does not start at 0; terms = 1 is also public_kernel's words; host and device entries agree"""
    import torch
    from peba1_amd import api
    N = K.RINGS[name]
    T = K.max_coef(N)
    pp = params_of(N)
    rng = np.random.default_rng(977 + N + terms)
    c = T // terms
    polys = rng.integers(-c, c + 1, (GROUPS * terms, N))
    polys[0, 0], polys[0, N - 1], polys[terms - 1, 1] = c, -c, -c
    ring = K.random_ring(rng, terms, N)
    g = api.PublicGallery(pp, polys)
    want = Q.sum_products(polys, ring, terms)
    assert want.shape == (GROUPS, 2, N)
    assert_words(api.kernel_ring_public_sum_product(g, ring, terms).reshape(-1, 2, N), want, (name, terms, "five groups"))
    assert_words(api.kernel_ring_public_sum_product(g, ring, terms, 0, 1).reshape(-1, 2, N), want[:1], (name, terms, "one group"))
    assert_words(api.kernel_ring_public_sum_product(g, ring, terms, 3 * terms, 2).reshape(-1, 2, N), want[3:], (name, terms, "groups 3, 4"))
    if terms == 1:
        assert_words(api.kernel_ring_public_sum_product(g, ring, 1), api.kernel_ring_public_product(g, ring, 0, GROUPS), "K = 1 word parity")
    assert_words(api.ring_mul_public_sum(g, ring, terms).reshape(-1, 2, N), want, (name, terms, "public entry, host"))
    dev = torch.from_numpy(ring.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_mul_public_sum(g, dev, terms, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.cpu().numpy().reshape(-1, 2, N), want, (name, terms, "public entry, device"))
    assert_words(dev.cpu().numpy(), ring.reshape(-1), "the resident samples are read only")
    assert api.last_error() == ""
    del dev, out
    g.close()


@pytest.mark.parametrize("name", list(K.RINGS))
def test_worst_magnitude_reaches_the_crt_bound_exactly(name):
    """every coefficient -T / MAX_TERMS against words 0x80000000: N T 2^31 at coefficient N - 1, as ring_public.hpp describes
    for one term; closed form in Python integers and the restatement"""
    from peba1_amd import api
    N = K.RINGS[name]
    pp = params_of(N)
    polys, ring, coef = Q.worst_group(N, Q.MAX_TERMS)
    assert max(abs(v) for v in coef) == N * K.max_coef(N) * 2 ** 31 < K.CRT_EXACT_LIMIT
    g = api.PublicGallery(pp, polys)
    got = api.kernel_ring_public_sum_product(g, ring, Q.MAX_TERMS).reshape(2, N)
    want = K.to_i32(np.array([v % 2 ** 32 for v in coef], dtype=np.int64))
    assert_words(got, np.stack([want, want]), (name, "worst case, closed form"))
    assert_words(got, Q.sum_product(polys, ring), (name, "worst case, restatement"))
    # the same magnitudes with the words at the other end of the signed range, and mixed signs of the coefficients
    ring[1::2] = K.I32_MAX
    polys[::3] *= -1
    g2 = api.PublicGallery(pp, polys)
    assert_words(api.kernel_ring_public_sum_product(g2, ring, Q.MAX_TERMS).reshape(2, N), Q.sum_product(polys, ring), (name, "range ends"))
    for o in (g, g2):
        o.close()


@pytest.fixture(scope="module")
def rows_case():
    """three groups of two 0 / +-small polynomials at N = 1024 and a probe of two random samples"""
    from peba1_amd import api
    N = 1024
    pp = params_of(N)
    rng = np.random.default_rng(4242)
    polys = rng.integers(-40, 41, (6, N))
    probe = K.random_ring(rng, 2, N)
    g = api.PublicGallery(pp, polys)
    yield pp, g, polys, probe
    g.close()


# widths 1, 16, N; M = S + 1 and 2 S + 3 are no multiples of S (the last workgroup is cut); M = 1
@pytest.mark.parametrize("w,M", [(1, 1025), (16, 2 * 64 + 3), (16, 1), (1024, 3), (1024, 1)])
def test_extracted_rows_against_the_restatement(L, rows_case, w, M):
    from peba1_amd import api
    pp, g, polys, probe = rows_case
    N = pp.N
    want = Q.sum_rows(polys, probe, 2, M, w)
    assert_words(api.kernel_ring_public_sum_rows(g, probe, 2, M, w), want, (w, M))
    rows = api.extract_rows(N + 4)
    assert rows.shape[0] == M and (rows[:, N + 1:] == 0).all()
    assert_words(rows[:, :N + 1], want, "padded rows")
    assert api.last_error() == ""


# ---- the public entry ----
@pytest.fixture(scope="module")
def small_keys():
    from peba1_amd import api
    pp = params_of(1024, n=12)
    ks = api.SecretKeySet(pp, 0x1AEA, device=True)
    yield pp, ks
    ks.close()


@pytest.mark.parametrize("terms,w,M", [(2, 16, 70), (4, 1024, 2), (3, 128, 11)])
def test_ring_inner_public_sum_is_its_rows_under_the_unpacks_key_switch(L, small_keys, terms, w, M):
    """host and device forms, with a recorded gate pending before the call and still pending after it: the exported words
    are the key switch (tests/ks_common.py, the unpack's) of the rows the raw entry returns, which are the restatement's"""
    import torch
    from peba1_amd import api
    pp, ks = small_keys
    N = pp.N
    rng = np.random.default_rng(60 + w)
    groups = api.lookup_samples(pp, M, w)
    polys = rng.integers(-9, 10, (groups * terms, N))
    probe = K.random_ring(rng, terms, N)
    g = api.PublicGallery(pp, polys)
    L.tfhe_hip_clear_error()
    rows = api.kernel_ring_public_sum_rows(g, probe, terms, M, w)
    assert_words(rows, Q.sum_rows(polys, probe, terms, M, w), "rows against the restatement")
    want = K.keyswitched(ks.ksk(), pp, rows)
    L.tfhe_hip_set_encrypt_seed(33)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    gate = api.CiphertextArray(pp, 3)
    api.gate_batch("AND", gate, a, b, ks)
    before = api.stats()
    host = api.CiphertextArray(pp, M)
    api.ring_inner_public_sum(g, probe, terms, M, w, ks, host)
    dev = torch.from_numpy(probe.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.CiphertextArray(pp, M)
    api.ring_inner_public_sum(g, dev, terms, M, w, ks, out, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    after = api.stats()
    assert after["keyswitches"] - before["keyswitches"] == 2 * M
    for f in ("blind_rotates", "levels", "flushes", "br_launches"):
        assert after[f] == before[f], f                           # the gate is still pending (reading words out would flush it)
    slots = [host.at(j).contents.slot for j in range(M)] + [out.at(j).contents.slot for j in range(M)]
    assert len(set(slots)) == 2 * M and min(slots) >= 0
    assert_words(host.words(), want, ("host form", terms, w, M))
    assert_words(out.words(), want, ("device form", terms, w, M))
    assert_words(dev.cpu().numpy(), probe.reshape(-1), "the resident probe is read only")
    assert list(gate.decrypt(ks)) == [0, 1, 0] and api.stats()["blind_rotates"] - before["blind_rotates"] == 3
    assert api.last_error() == ""
    del dev
    g.close()
    for o in (a, b, gate, host, out):
        o.close()


# ---- decrypt level at P128: 2,048-bit codes ----
LENGTH, WIDTH = 2048, 1024


def _phase_errors(words, lwe_key, want_units, delta):
    ph = K.U.lwe_phases(words, lwe_key).astype(np.int64)
    return (ph - np.asarray(want_units, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31


def test_p128_long_templates_decide_right_outside_the_band(p128_keys, capsys):
    """8 entries of 2,048 bits as groups of two polynomials, terms = 2, tau = 655 (8/25 of 2,048): every distance is chosen at
    least clear_decision_band away from tau, on both sides, the nearest two exactly on its edge; all must decide right"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    terms, tau = LENGTH // WIDTH, 655
    delta = identify.inner_delta(LENGTH)
    band = identify.clear_decision_band(pp, delta)
    assert band == 184
    distances = [0, 200, tau - band, tau + band, 1000, 1400, 2048, 330]
    assert all(abs(d - tau) >= band for d in distances)          # a condition, not a measurement
    assert any(d < tau for d in distances) and any(d > tau for d in distances)
    rng = np.random.default_rng(2048)
    probe = rng.integers(0, 2, LENGTH)
    entries = []
    for d in distances:
        e = probe.copy()
        e[rng.choice(LENGTH, d, replace=False)] ^= 1
        entries.append(e)
    polys = identify.clear_gallery_polys_long(entries, WIDTH, pp.N, terms)
    assert polys.shape == (len(entries) * terms, pp.N)
    gal = api.PublicGallery(pp, polys)
    ring, addend = identify.hamming_probe_ring_long(probe, WIDTH, terms, ks, seed=0x4C0)
    M = len(entries)
    inner = api.CiphertextArray(pp, M)
    api.ring_inner_public_sum(gal, ring, terms, M, WIDTH, ks, inner)
    err = _phase_errors(inner.words(), ks.lwe_key(), [d - int(probe.sum()) for d in distances], delta)
    with capsys.disabled():
        print("\npublic sum P128 long, %d x %d bits, terms = %d: largest |phase error| before the bootstrap %.3e beside the computed "
              "sigma_dec %.3e (Delta = %.3e, band %d)" % (M, LENGTH, terms, np.abs(err).max() / 2.0 ** 32, identify.inner_decision_sigma(pp),
                                                         delta / 2.0 ** 32, band))
    inner.close()
    bits = identify.match_clear_gallery_long(gal, ring, terms, M, WIDTH, addend, tau, ks)
    got = [int(b) for b in bits.decrypt(ks)]
    assert got == [1 if d <= tau else 0 for d in distances], (distances, got)
    gal.close()
    for o in (bits, addend):
        o.close()


def test_p128_masked_templates_decide_right_outside_the_band(L, p128_keys, capsys):
    """8 masked entries of 2,048 bits at 8/25 as groups of four polynomials, terms = 4, one of them with a mask that drops
    half the bits: every D is chosen outside clear_decision_band on purpose, on both sides of 0; all must decide right, at
    exactly the key switches and bootstraps of an unmasked match of as many entries"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    num, den, terms = 8, 25, 2 * LENGTH // WIDTH
    delta = identify.masked_delta(den, LENGTH)
    band = identify.clear_decision_band(pp, delta)
    assert band == 5869 and terms == 4
    rng = np.random.default_rng(825)
    b, m = rng.integers(0, 2, LENGTH), (rng.random(LENGTH) < 0.9).astype(np.int64)
    # (fraction of the gallery mask kept, disagreeing fraction of the valid bits)
    plan = [(1.0, 0.0), (0.9, 0.10), (0.8, 0.20), (0.5, 0.05), (1.0, 0.45), (0.9, 0.50), (0.8, 0.60), (0.5, 0.70)]
    codes, masks, D, want = [], [], [], []
    for keep, frac in plan:
        n = (rng.random(LENGTH) < keep).astype(np.int64)
        if keep == 0.5:
            n = np.arange(LENGTH) % 2                             # a mask that drops half the bits
        both = np.flatnonzero(m & n)
        g = b.copy()
        g[rng.choice(both, int(round(frac * len(both))), replace=False)] ^= 1
        g[np.flatnonzero(1 - (m & n))] = rng.integers(0, 2, LENGTH - len(both))       # what a mask drops does not count
        codes.append(g), masks.append(n)
        D.append(identify.masked_decision(b, g, m, n, num, den))
        valid, disagree = Q.masked_counts(b, g, m, n)
        want.append(1 if den * disagree <= num * valid else 0)
    assert all(abs(d) >= band for d in D), (D, band)             # a condition, not a measurement
    assert sorted(set(want)) == [0, 1] and want == [1 if d <= 0 else 0 for d in D]
    polys = identify.masked_gallery_polys(codes, masks, WIDTH, pp.N, num, den)
    M = len(plan)
    assert polys.shape == (M * terms, pp.N)
    gal = api.PublicGallery(pp, polys)
    ring = identify.masked_probe_ring(b, m, WIDTH, num, den, ks, seed=0x4D0)
    assert ring.shape == (terms, 2 * pp.N)
    inner = api.CiphertextArray(pp, M)
    api.ring_inner_public_sum(gal, ring, terms, M, WIDTH, ks, inner)
    err = _phase_errors(inner.words(), ks.lwe_key(), D, delta)
    with capsys.disabled():
        print("\npublic sum P128 masked %d/%d, %d x %d bits, terms = %d: D = %s; largest |phase error| before the bootstrap %.3e beside the "
              "computed sigma_dec %.3e (Delta = %.3e, band %d)" % (num, den, M, LENGTH, terms, D, np.abs(err).max() / 2.0 ** 32,
                                                                 identify.inner_decision_sigma(pp), delta / 2.0 ** 32, band))
    inner.close()
    counted = ("keyswitches", "blind_rotates", "br_launches", "levels", "flushes", "ks_pergate_launches", "ks_strip_launches",
               "ks_index_launches")
    before = api.stats()
    bits = identify.match_clear_gallery_masked(gal, ring, M, WIDTH, LENGTH, num, den, ks)
    after = api.stats()
    masked = {f: after[f] - before[f] for f in counted}
    got = [int(x) for x in bits.decrypt(ks)]
    assert got == want, (D, got, want)
    # an unmasked match of as many entries (128-bit templates in one polynomial): no fewer key switches, bootstraps or launches
    plain_gal = api.PublicGallery(pp, identify.clear_gallery_polys(rng.integers(0, 2, (M, 128)), 128, pp.N))
    plain_ring, addend = identify.hamming_probe_ring(rng.integers(0, 2, 128), 128, ks, seed=0x4D9)
    before = api.stats()
    plain_bits = identify.match_clear_gallery(plain_gal, plain_ring, M, 128, addend, 40, ks)
    after = api.stats()
    plain = {f: after[f] - before[f] for f in counted}
    with capsys.disabled():
        print("masked match %s\nunmasked match %s" % (masked, plain))
    assert masked["blind_rotates"] == plain["blind_rotates"] == M
    for f in counted:
        assert masked[f] <= plain[f], (f, masked, plain)
    for o in (gal, plain_gal, bits, plain_bits, addend):
        o.close()
