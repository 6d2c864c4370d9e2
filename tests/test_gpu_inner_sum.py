"""Sums of TGSW products over several ring samples on the GPU.  The summed product kernel and its fused extraction are
compared word for word with the numpy restatement (tests/inner_sum_common.py) -- no tolerance anywhere at word level --, on
both sides of every fold of the accumulator and at the operands that reach the CRT bound exactly; the public entry with that
restatement's rows under the key switch of tests/ks_common.py; the long and the masked Hamming routes on top
(peba1_amd.identify) are checked by what they mean, at distances chosen outside the computed decision band on purpose."""
import numpy as np
import pytest

import inner_common as I
import inner_sum_common as Q
import public_common as K
import select_common as S

pytestmark = pytest.mark.gpu

GADGETS = {1024: (3, 7), 2048: (3, 6)}
GROUPS = 5


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


def params_of(N, n=10, gadget=None):
    from peba1_amd import api
    return api.ParameterSet(custom=K.custom_tuple(n, N=N, gadget=gadget or GADGETS[N]))


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def random_selector_words(rng, samples, l, N):
    """arbitrary 32-bit words: tfhe_hip_new_selector takes them, and both bounds take the row words as arbitrary"""
    return S.random_ring(rng, samples * 2 * l, N).reshape(samples, 2 * l, 2, N)


# ---- the kernel, word for word ----
# (3, 7) at N = 1024 folds after 18 rows = 3 terms: terms 3 and 4 sit on either side of the first fold, 7 = max_terms crosses
# two; (3, 6) at N = 2048 folds after 16 rows, inside term 3; (4, 5) has 8 rows a term: the fold after row 18 falls inside
# term 3 and the one after row 36 inside term 5
CASES = [(1024, (3, 7), 1), (1024, (3, 7), 2), (1024, (3, 7), 3), (1024, (3, 7), 4), (1024, (3, 7), 7), (2048, (3, 6), 2),
         (2048, (3, 6), 3), (1024, (4, 5), 3), (1024, (4, 5), 5)]


@pytest.mark.parametrize("N,gadget,terms", CASES)
def test_summed_products_and_rows_against_the_restatement(L, N, gadget, terms):
    """random ring words, random selector words, a sample_index of 1, 5 groups and 1 group, the product and the rows; host and
    device entries agree and the resident words are read only; terms = 1 is tfhe_hip_kernel_ring_product's and
    tfhe_hip_kernel_ring_inner_rows' words"""
    import torch
    from peba1_amd import api
    l, Bg = gadget
    pp = params_of(N, gadget=gadget)
    assert terms <= api.inner_sum_max_terms(pp) == Q.max_terms(N, l, Bg)
    if gadget == GADGETS[N]:
        assert api.inner_sum_max_terms(pp) == 7
    rng = np.random.default_rng(1300 + N + 10 * l + terms)
    first = 1
    words = random_selector_words(rng, first + terms, l, N)
    sel = api.Selector(pp, words)
    ring = S.random_ring(rng, GROUPS * terms, N)
    want = Q.sum_products(words, first, terms, ring, l, Bg)
    assert want.shape == (GROUPS, 2, N)
    assert_words(api.kernel_ring_inner_sum_product(sel, first, terms, ring).reshape(-1, 2, N), want, (N, gadget, terms, "five groups"))
    assert_words(api.kernel_ring_inner_sum_product(sel, first, terms, ring[3 * terms:4 * terms]).reshape(-1, 2, N), want[3:4],
                 (N, gadget, terms, "one group"))
    # the rows: width N / 4, the last group cut after its second entry
    w, M = N // 4, 4 * (GROUPS - 1) + 2
    rows = api.kernel_ring_inner_sum_rows(sel, first, terms, ring, M, w)
    assert_words(rows, I.inner_rows(want, M, w), (N, gadget, terms, "rows"))
    assert_words(api.kernel_ring_inner_sum_rows(sel, first, terms, ring[:terms], 1, N), I.inner_rows(want[:1], 1, N), "one group, one row")
    if terms == 1:
        assert_words(api.kernel_ring_inner_sum_product(sel, first, 1, ring), api.kernel_ring_product(sel, first, ring), "K = 1 product parity")
        assert_words(rows, api.kernel_ring_inner_rows(sel, first, ring, M, w), "K = 1 rows parity")
    assert_words(api.ring_mul_tgsw_sum(sel, first, terms, ring).reshape(-1, 2, N), want, (N, gadget, terms, "public entry, host"))
    dev = torch.from_numpy(ring.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_mul_tgsw_sum(sel, first, terms, dev, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.cpu().numpy().reshape(-1, 2, N), want, (N, gadget, terms, "public entry, device"))
    assert_words(dev.cpu().numpy(), ring.reshape(-1), "the resident samples are read only")
    assert api.last_error() == ""
    del dev, out
    sel.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_worst_magnitudes_reach_the_crt_bound_exactly(N):
    """max_terms = 7 terms, every digit -Bg/2, every selector word 0x80000000: 7 (k+1) l N (Bg/2) 2^31 at coefficient N - 1,
    the CRT bound's left side, against the closed form in Python integers and the restatement.  Then the MAC side as far as
    row words reach it: every digit +Bg/2 - 1 (the forward transform's largest input) against rows at both ends of the signed
    range and random rows, whose image words range over all of [0, P)"""
    from peba1_amd import api
    l, Bg = GADGETS[N]
    pp = params_of(N)
    terms = api.inner_sum_max_terms(pp)
    assert terms == 7
    words, ring, coef = Q.worst_case(N, l, Bg, terms)
    top = terms * 2 * l * N * 2 ** (Bg - 1) * 2 ** 31
    assert max(abs(v) for v in coef) == coef[N - 1] == top < S.CRT_EXACT_LIMIT < top // terms * (terms + 1)
    sel = api.Selector(pp, words)
    got = api.kernel_ring_inner_sum_product(sel, 0, terms, ring).reshape(2, N)
    want = S.to_i32(np.array([v % 2 ** 32 for v in coef], dtype=np.int64))
    assert_words(got, np.stack([want, want]), (N, "worst case, closed form"))
    assert_words(got, Q.sum_product(words, ring, l, Bg), (N, "worst case, restatement"))
    sel.close()
    # the MAC side
    rng = np.random.default_rng(77 + N)
    ring2 = S.to_i32(np.full((terms, 2, N), S.extreme_difference(l, Bg, "max"), dtype=np.int64))
    assert (S.decompose(ring2[0, 1], l, Bg) == 2 ** (Bg - 1) - 1).all()
    words2 = random_selector_words(rng, terms, l, N)
    words2[0::3, :, :, 0::2] = S.I32_MAX
    words2[1::3, :, :, 1::2] = S.I32_MIN
    sel2 = api.Selector(pp, words2)
    assert_words(api.kernel_ring_inner_sum_product(sel2, 0, terms, ring2).reshape(2, N), Q.sum_product(words2, ring2, l, Bg), (N, "largest digits"))
    sel2.close()


def test_plain_and_compressed_selectors_give_the_same_words(L):
    """one seed-compressed record of three probe polynomials: the compressed selector (masks written on the card) and a plain
    selector over the host expansion of the same record return the same sums and rows, which are the restatement's"""
    from peba1_amd import api
    N = 1024
    l, Bg = GADGETS[N]
    pp = params_of(N, n=12)
    ks = api.SecretKeySet(pp, 0x5E1, device=False)
    rng = np.random.default_rng(31)
    polys = rng.integers(-1, 2, (3, N))
    record = api.tgsw_encrypt_polys_compressed(polys, ks, seed=0x5E2)
    plain_words = api.tgsw_expand(record, pp)
    ring = S.random_ring(rng, 2 * 3, N)
    comp, plain = api.Selector.from_compressed(pp, record), api.Selector(pp, plain_words)
    want = Q.sum_products(plain_words.reshape(3, 2 * l, 2, N), 0, 3, ring, l, Bg)
    a, b = api.kernel_ring_inner_sum_product(comp, 0, 3, ring), api.kernel_ring_inner_sum_product(plain, 0, 3, ring)
    assert_words(a, b, "compressed against plain")
    assert_words(a.reshape(-1, 2, N), want, "against the restatement")
    assert_words(api.kernel_ring_inner_sum_rows(comp, 0, 3, ring, 9, 128), api.kernel_ring_inner_sum_rows(plain, 0, 3, ring, 9, 128), "rows")
    assert_words(api.kernel_ring_inner_sum_product(comp, 1, 2, ring[:4]), api.kernel_ring_inner_sum_product(plain, 1, 2, ring[:4]), "from sample 1")
    assert api.last_error() == ""
    for o in (comp, plain, ks):
        o.close()


# ---- the public entry ----
@pytest.fixture(scope="module")
def small_keys():
    from peba1_amd import api
    pp = params_of(1024, n=12)
    ks = api.SecretKeySet(pp, 0x1AEB, device=True)
    yield pp, ks
    ks.close()


@pytest.mark.parametrize("terms,w,M", [(2, 16, 70), (4, 1024, 2), (3, 128, 11)])
def test_ring_inner_sum_is_its_rows_under_the_unpacks_key_switch(L, small_keys, terms, w, M):
    """host and device forms, with a recorded gate pending before the call and still pending after it: the exported words
    are the key switch (tests/ks_common.py, the unpack's) of the rows the raw entry returns, which are the restatement's"""
    import torch
    from peba1_amd import api
    pp, ks = small_keys
    N = pp.N
    l, Bg = GADGETS[N]
    rng = np.random.default_rng(160 + w)
    groups = api.lookup_samples(pp, M, w)
    words = random_selector_words(rng, terms, l, N)
    sel = api.Selector(pp, words)
    ring = S.random_ring(rng, groups * terms, N)
    L.tfhe_hip_clear_error()
    rows = api.kernel_ring_inner_sum_rows(sel, 0, terms, ring, M, w)
    assert_words(rows, Q.sum_rows(words, 0, terms, ring, M, w, l, Bg), "rows against the restatement")
    want = K.keyswitched(ks.ksk(), pp, rows)
    L.tfhe_hip_set_encrypt_seed(34)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    gate = api.CiphertextArray(pp, 3)
    api.gate_batch("AND", gate, a, b, ks)
    before = api.stats()
    host = api.CiphertextArray(pp, M)
    api.ring_inner_sum(sel, 0, terms, ring, M, w, ks, host)
    dev = torch.from_numpy(ring.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.CiphertextArray(pp, M)
    api.ring_inner_sum(sel, 0, terms, dev, M, w, ks, out, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    after = api.stats()
    assert after["keyswitches"] - before["keyswitches"] == 2 * M
    for f in ("blind_rotates", "levels", "flushes", "br_launches"):
        assert after[f] == before[f], f                           # the gate is still pending (reading words out would flush it)
    slots = [host.at(j).contents.slot for j in range(M)] + [out.at(j).contents.slot for j in range(M)]
    assert len(set(slots)) == 2 * M and min(slots) >= 0
    assert_words(host.words(), want, ("host form", terms, w, M))
    assert_words(out.words(), want, ("device form", terms, w, M))
    assert_words(dev.cpu().numpy(), ring.reshape(-1), "the resident gallery is read only")
    assert list(gate.decrypt(ks)) == [0, 1, 0] and api.stats()["blind_rotates"] - before["blind_rotates"] == 3
    # a refusal on the device leaves everything as it was
    held = host.words().copy()
    assert L.tfhe_hip_ring_inner_sum(sel.ptr, 0, 8, ks.cloud, ring.ctypes.data_as(L.tfhe_hip_ring_inner_sum.argtypes[4]), M, w, host.ptr) == -1
    assert "terms must be in 1..7" in api.last_error()
    L.tfhe_hip_clear_error()
    assert_words(host.words(), held, "a refused call changes nothing")
    del dev
    sel.close()
    for o in (a, b, gate, host, out):
        o.close()


# ---- decrypt level at P128: 2,048-bit codes ----
LENGTH, WIDTH = 2048, 1024


def _phase_errors(words, lwe_key, want_units, delta):
    ph = K.U.lwe_phases(words, lwe_key).astype(np.int64)
    return (ph - np.asarray(want_units, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31


def _row_errors(rows, tlwe_key, want_units, delta):
    ph = I.row_phases(rows, tlwe_key).astype(np.int64)
    return (ph - np.asarray(want_units, dtype=np.int64) * delta + 2 ** 31) % 2 ** 32 - 2 ** 31


def test_p128_long_templates_decide_right_outside_the_band(p128_keys, capsys):
    """8 entries of 2,048 bits as groups of two ring samples, terms = 2, w = 1,024, tau = 655 (8/25 of 2,048): every distance
    is chosen at least inner_sum_decision_band away from tau, on both sides, the nearest two exactly on its edge; all must
    decide right.  A seed-compressed probe record."""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    terms, tau = LENGTH // WIDTH, 655
    delta = identify.inner_delta(LENGTH)
    band = identify.inner_sum_decision_band(pp, delta, terms)
    assert band == 185
    distances = [0, 200, tau - band, tau + band, 1000, 1400, 2048, 330]
    assert all(abs(d - tau) >= band for d in distances)          # a condition, not a measurement
    assert any(d < tau for d in distances) and any(d > tau for d in distances)
    rng = np.random.default_rng(2049)
    probe = rng.integers(0, 2, LENGTH)
    entries = []
    for d in distances:
        e = probe.copy()
        e[rng.choice(LENGTH, d, replace=False)] ^= 1
        entries.append(e)
    M = len(entries)
    gal = identify.pack_gallery_inner_long(entries, WIDTH, terms, ks, seed=0x6C0)
    assert gal.shape == (M * terms, 2 * pp.N)
    record, addend = identify.hamming_probe_long(probe, WIDTH, terms, ks, compressed=True, seed=0x6C1)
    sel = api.Selector.from_compressed(pp, record)
    want_units = [d - int(probe.sum()) for d in distances]
    rows = api.kernel_ring_inner_sum_rows(sel, 0, terms, gal, M, WIDTH)
    err0 = _row_errors(rows, ks.tlwe_key(), want_units, delta)
    sigma0 = Q.variance(pp.N, pp.l, pp.Bgbit, 2.0 ** -25, [WIDTH] * terms, 2.0 ** -50) ** 0.5
    inner = api.CiphertextArray(pp, M)
    api.ring_inner_sum(sel, 0, terms, gal, M, WIDTH, ks, inner)
    err = _phase_errors(inner.words(), ks.lwe_key(), want_units, delta)
    with capsys.disabled():
        print("\ninner sum P128 long, %d x %d bits, terms = %d: largest |phase error| before the key switch %.3e beside the computed sigma "
              "%.3e; before the bootstrap %.3e beside the computed sigma_dec %.3e (Delta = %.3e, band %d)"
              % (M, LENGTH, terms, np.abs(err0).max() / 2.0 ** 32, sigma0, np.abs(err).max() / 2.0 ** 32, identify.inner_decision_sigma(pp),
                 delta / 2.0 ** 32, band))
    inner.close()
    bits = identify.match_by_inner_long(sel, gal, terms, M, WIDTH, addend, tau, ks)
    got = [int(b) for b in bits.decrypt(ks)]
    assert got == [1 if d <= tau else 0 for d in distances], (distances, got)
    sel.close()
    for o in (bits, addend):
        o.close()


def test_p128_masked_templates_decide_right_outside_the_band(L, p128_keys, capsys):
    """8 masked entries of 2,048 bits at 8/25 as groups of four ring samples, terms = 4, one of them with a mask that drops
    half the bits: every D is chosen outside masked_inner_band on purpose, on both sides of 0; all must decide right,
    at one key switch and one bootstrap an entry"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    num, den, terms = 8, 25, 2 * LENGTH // WIDTH
    delta = identify.masked_delta(den, LENGTH)
    band = identify.masked_inner_band(pp, LENGTH, WIDTH, den)
    assert band == 6571 and terms == 4
    rng = np.random.default_rng(826)
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
    M = len(plan)
    gal = identify.masked_gallery_inner(codes, masks, WIDTH, num, den, ks, seed=0x6D0)
    assert gal.shape == (M * terms, 2 * pp.N)
    words = identify.masked_probe_tgsw(b, m, WIDTH, num, den, ks, seed=0x6D1)
    sel = api.Selector(pp, words)
    rows = api.kernel_ring_inner_sum_rows(sel, 0, terms, gal, M, WIDTH)
    err0 = _row_errors(rows, ks.tlwe_key(), D, delta)
    values = [v for c in range(2) for v in ((1 - 2 * b[c * WIDTH:(c + 1) * WIDTH]) * m[c * WIDTH:(c + 1) * WIDTH], m[c * WIDTH:(c + 1) * WIDTH])]
    weights = [identify.probe_rounding_weight(v, pp.N) for v in values]          # (the mask polynomials have one sign)
    sigma0 = Q.variance_weighted(pp.N, pp.l, pp.Bgbit, 2.0 ** -25, [int(np.abs(v).sum()) for v in values], weights, 2.0 ** -50) ** 0.5
    inner = api.CiphertextArray(pp, M)
    api.ring_inner_sum(sel, 0, terms, gal, M, WIDTH, ks, inner)
    err = _phase_errors(inner.words(), ks.lwe_key(), D, delta)
    with capsys.disabled():
        print("\ninner sum P128 masked %d/%d, %d x %d bits, terms = %d: D = %s; largest |phase error| before the key switch %.3e beside the "
              "computed sigma %.3e; before the bootstrap %.3e beside the computed sigma_dec %.3e (Delta = %.3e, band %d)"
              % (num, den, M, LENGTH, terms, D, np.abs(err0).max() / 2.0 ** 32, sigma0, np.abs(err).max() / 2.0 ** 32,
                 identify.inner_decision_sigma(pp), delta / 2.0 ** 32, band))
    inner.close()
    before = api.stats()
    bits = identify.match_by_inner_masked(sel, gal, M, WIDTH, LENGTH, num, den, ks)
    after = api.stats()
    got = [int(x) for x in bits.decrypt(ks)]
    assert got == want, (D, got, want)
    assert after["keyswitches"] - before["keyswitches"] == 2 * M and after["blind_rotates"] - before["blind_rotates"] == M
    sel.close()
    bits.close()


# ---- the chunk boundary, the launch timer, the protocol routes ----
def test_rows_across_the_chunk_boundary_and_the_launch_timer(L, small_keys):
    """w = 1, terms = 2, M = 8,192 + 5: nine groups, the second chunk starts at group 8, whose samples lie (done / S) terms
    ring samples into the gallery.  The raw rows against the restatement on both sides of the boundary; the slot form's words
    for the entries around it; tfhe_hip_last_select_ms covers the launches of the call"""
    from peba1_amd import api
    pp, ks = small_keys
    N = pp.N
    l, Bg = GADGETS[N]
    terms, w, M = 2, 1, 8192 + 5
    groups = api.lookup_samples(pp, M, w)
    assert groups == 9
    rng = np.random.default_rng(8197)
    words = random_selector_words(rng, terms, l, N)
    sel = api.Selector(pp, words)
    ring = S.random_ring(rng, groups * terms, N)
    rows = api.kernel_ring_inner_sum_rows(sel, 0, terms, ring, M, w)
    prods = Q.sum_products(words, 0, terms, ring, l, Bg)
    around = [0, 1, 1023, 1024, 8190, 8191, 8192, 8193, M - 1]
    assert_words(rows[around], np.stack([I.extract(prods[i // N], i % N) for i in around]), "rows around the chunk boundary")
    assert_words(rows[8192:], I.inner_rows(prods[8:], 5, w), "the second chunk")
    assert_words(rows[7168:8192], I.inner_rows(prods[7:8], 1024, w), "the last group of the first chunk")
    L.tfhe_hip_set_kernel_timing(1)
    out = api.CiphertextArray(pp, M)
    api.ring_inner_sum(sel, 0, terms, ring, M, w, ks, out)
    ms = api.last_select_ms()
    L.tfhe_hip_set_kernel_timing(0)
    assert 0.0 < ms < 1000.0, ms                      # from the first chunk's launch to the second's
    assert_words(out.words()[around], K.keyswitched(ks.ksk(), pp, rows[around]), "slot form around the chunk boundary")
    assert api.last_error() == ""
    sel.close()
    out.close()


def test_protocol_routes_with_seeded_selectors(p128_keys):
    """protocol.run_inner_product_long and run_masked_inner_product, the probe travelling as ONE seed-compressed selector
    record: a template equal to the probe, one far inside the threshold, two random ones; every entry outside the band decides
    as the plaintext does, and the compressed probe is about half the plain one's bytes"""
    from peba1_amd import api, protocol
    pp, ks, _ = p128_keys
    rng = np.random.default_rng(77)
    probe = rng.integers(0, 2, LENGTH)
    near = probe.copy()
    near[rng.choice(LENGTH, 150, replace=False)] ^= 1
    templates = [probe.copy(), near, rng.integers(0, 2, LENGTH), rng.integers(0, 2, LENGTH)]
    outs = list(protocol.run_inner_product_long(pp, ks, [list(t) for t in templates], list(probe), tau=655, seeded_selectors=True))
    assert [o["distance"] for o in outs][:2] == [0, 150] and not any(o["inside_band"] for o in outs)
    assert [o["decrypted"] for o in outs] == [o["plain"] for o in outs] == [1, 1, 0, 0]
    assert outs[0]["probe_bytes"] == 4 * api.tgsw_compressed_words(pp, 2) < 0.51 * outs[0]["probe_bytes_plain"]
    masks = [np.ones(LENGTH, dtype=np.int64), (rng.random(LENGTH) < 0.85).astype(np.int64), np.arange(LENGTH) % 2, np.ones(LENGTH, dtype=np.int64)]
    probe_mask = (rng.random(LENGTH) < 0.9).astype(np.int64)
    mouts = list(protocol.run_masked_inner_product(pp, ks, [list(t) for t in templates], [list(m) for m in masks], list(probe),
                                                   list(probe_mask), num=8, den=25, seeded_selectors=True))
    assert not any(o["inside_band"] for o in mouts), [o["D"] for o in mouts]
    assert [o["decrypted"] for o in mouts] == [o["plain"] for o in mouts] == [1, 1, 0, 0]
    assert mouts[0]["probe_bytes"] == 4 * api.tgsw_compressed_words(pp, 4)
