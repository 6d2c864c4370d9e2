"""Seed-compressed selectors on the GPU (include/tfhe_hip.h "seed-compressed selectors").  The core check is word equality:
for one record, a compressed selector -- bodies uploaded, masks written on the card by the expand kernel at row counts far
below a cloud key's -- and a plain selector over the host expansion of the same record must give identical words through
every entry that takes a selector, on ring samples of arbitrary 32-bit words, so that every digit and every row matters.
Decryption, the Hamming route, the bytes copied to the card and the recorder's indifference are checked by what they mean."""
import numpy as np
import pytest

import seeded_select_common as Z
import select_common as S

pytestmark = pytest.mark.gpu

MARGIN = 1.0 / 8              # the decode margin tests/test_gpu_select.py asserts (test_p128_every_index_selects_its_template)


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
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def selector_pair(pp, record, nbits=None):
    """(compressed selector, plain selector over the host expansion) of one record"""
    from peba1_amd import api
    words = api.tgsw_expand(record, pp)
    return api.Selector.from_compressed(pp, record, nbits=nbits), api.Selector(pp, words if nbits is None else words[:nbits])


# ---- word equality through the select: the smallest shapes at which the expand launch can go wrong ----
@pytest.mark.parametrize("name,nbits,M", [("P128", 1, 2),                        # 6 rows: a cloud key has 3,780
                                          ("P128", 3, 5),                        # an odd tree
                                          ("P128", Z.SELECT_MAX_BITS, 3),        # the most rows, on a tiny tree
                                          ("P2048", 2, 3)])                      # another group count per polynomial
def test_select_words_equal_those_under_the_host_expanded_selector(L, name, nbits, M):
    from peba1_amd import api
    N, l, _ = S.SETS[name]
    pp = Z.params_of(name)
    rng = np.random.default_rng(1000 * nbits + N + M)
    record = Z.random_record(rng, 1, l, N, nbits)
    gallery = S.random_ring(rng, M, N)
    # the library's host expansion is the restatement's (checked at length without a GPU): here for the words under test
    assert_words(api.tgsw_expand(record, pp), Z.expand(L, record, 1, l, N), (name, nbits, "host expansion"))
    sc, sh = selector_pair(pp, record)
    try:
        assert sc.upload_bytes() == 0 and sh.upload_bytes() == 0
        got, want = api.ring_select(sc, gallery), api.ring_select(sh, gallery)
        assert_words(got, want, (name, nbits, M))
        assert np.count_nonzero(got) > N                      # not two all-zero answers
        # the bytes copied to the card: the bodies alone, against every word
        assert sc.upload_bytes() == nbits * 2 * l * N * 4
        assert sh.upload_bytes() == 2 * sc.upload_bytes()
        assert_words(api.ring_select(sc, gallery), want, (name, nbits, M, "second use of the resident image"))
        assert sc.upload_bytes() == nbits * 2 * l * N * 4
        assert api.last_error() == ""
    finally:
        sc.close()
        sh.close()


def test_a_selector_of_fewer_bits_than_its_record_reads_the_records_first_samples(L):
    from peba1_amd import api
    N, l, _ = S.SETS["P128"]
    pp = Z.params_of("P128")
    rng = np.random.default_rng(5)
    record, gallery = Z.random_record(rng, 1, l, N, 3), S.random_ring(rng, 4, N)
    sc, sh = selector_pair(pp, record, nbits=2)
    try:
        assert_words(api.ring_select(sc, gallery), api.ring_select(sh, gallery), "2 of 3 samples")
        assert sc.upload_bytes() == 2 * 2 * l * N * 4
    finally:
        sc.close()
        sh.close()


# ---- the other entries that take a selector ----
def test_lookup_words_equal_those_under_the_host_expanded_selector(L):
    """width 8 at N = 1,024: 128 entries in one ring sample, seven rotation steps under seven bits"""
    from peba1_amd import api
    N, l, _ = S.SETS["P128"]
    pp = Z.params_of("P128")
    rng = np.random.default_rng(78)
    record, gallery = Z.random_record(rng, 1, l, N, 7), S.random_ring(rng, 1, N)
    sc, sh = selector_pair(pp, record)
    try:
        got = api.ring_lookup(sc, gallery, 128, 8)
        assert_words(got, api.ring_lookup(sh, gallery, 128, 8), "lookup, width 8, M = 128")
        assert np.count_nonzero(got) > N
    finally:
        sc.close()
        sh.close()


def test_inner_rows_equal_those_under_the_host_expanded_probe(L):
    """one compressed polynomial probe, two ring samples of eight entries of width 128, the last one partly filled"""
    from peba1_amd import api
    N, l, _ = S.SETS["P128"]
    pp = Z.params_of("P128")
    rng = np.random.default_rng(79)
    record, ring = Z.random_record(rng, 1, l, N, 1), S.random_ring(rng, 2, N)
    sc, sh = selector_pair(pp, record)
    try:
        got = api.kernel_ring_inner_rows(sc, 0, ring, 11, 128)
        assert got.shape == (11, N + 1)
        assert_words(got, api.kernel_ring_inner_rows(sh, 0, ring, 11, 128), "inner rows, width 128, M = 11")
        assert_words(api.kernel_ring_product(sc, 0, ring), api.kernel_ring_product(sh, 0, ring), "full products")
        assert np.count_nonzero(got) > N
    finally:
        sc.close()
        sh.close()


# ---- decrypt level at P128 ----
@pytest.fixture(scope="module")
def p128_gallery(p128_keys):
    """eight ring-encrypted templates of 1,024 bits under the P128 keyset"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits = np.random.default_rng(23).integers(0, 2, (8, pp.N))
    return bits, np.stack([api.ring_encrypt_bits(bits[m], ks, seed=0x6B11 + m) for m in range(8)])


def test_p128_every_index_selects_its_template_under_a_compressed_selector(p128_keys, p128_gallery, capsys):
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits, gallery = p128_gallery
    worst = 0.0
    for index in range(8):
        record = api.tgsw_encrypt_bits_compressed([(index >> j) & 1 for j in range(3)], ks, seed=0x52D + index)
        sel = api.Selector.from_compressed(pp, record)
        out = api.ring_select(sel, gallery)
        sel.close()
        assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[index]), index
        ph = api.packed_phases(out, ks).astype(np.float64) / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(bits[index] == 1, 0.125, -0.125)).max())
    sigma = (S.STDEVS[1] ** 2 + 3 * S.cmux_variance(pp.N, pp.l, pp.Bgbit, S.STDEVS[1])) ** 0.5
    with capsys.disabled():
        print("\ncompressed select P128, 8 templates, 3 levels: largest |phase error| %.3e, computed sigma bound %.3e (%.2f sigma)"
              % (worst, sigma, worst / sigma))
    assert worst < MARGIN


def test_p128_compressed_hamming_probe_decides_as_the_plaintext_outside_the_band(p128_keys, capsys):
    """identify.hamming_probe(compressed=True) through match_by_inner: 24 entries of 128 bits on both sides of tau = 40, at
    least three quarters of them outside inner_decision_band, every one of those decided as the plaintext distance says"""
    from peba1_amd import api, identify
    pp, ks, _ = p128_keys
    w, tau = 128, 40
    distances = [0, 3, 9, 10, 15, 20, 24, 26, 28, 52, 53, 55, 60, 64, 70, 90, 100, 128, 35, 39, 40, 41, 45, 50]
    rng = np.random.default_rng(2000 + w)
    probe = rng.integers(0, 2, w)
    entries = []
    for d in distances:
        e = probe.copy()
        e[rng.choice(w, d, replace=False)] ^= 1
        entries.append(e)
    M = len(entries)
    assert [int((e ^ probe).sum()) for e in entries] == distances
    g = identify.inner_decision_band(pp, w)
    outside = [i for i, d in enumerate(distances) if abs(d - tau) >= g]
    assert 4 * len(outside) >= 3 * M and any(distances[i] < tau for i in outside) and any(distances[i] > tau for i in outside)
    gallery = identify.pack_gallery_inner(np.array(entries), w, ks, seed=0x3A0)
    record, addend = identify.hamming_probe(probe, w, ks, seed=0x4B0, compressed=True)
    assert record.shape == (api.tgsw_compressed_words(pp, 1),)
    sel = api.Selector.from_compressed(pp, record)
    bits = identify.match_by_inner(sel, gallery, M, w, addend, tau, ks)
    got = [int(b) for b in bits.decrypt(ks)]
    with capsys.disabled():
        print("\ncompressed Hamming probe P128 w = %d, tau = %d, band g = %d: (distance, decision) inside the band, reported only: %s"
              % (w, tau, g, [(distances[i], got[i]) for i in range(M) if i not in outside]))
    for i in outside:
        assert got[i] == (1 if distances[i] <= tau else 0), (i, distances[i], got[i])
    assert sel.upload_bytes() == 2 * pp.l * pp.N * 4
    sel.close()
    for o in (bits, addend):
        o.close()


def test_p128_recorded_gates_stay_pending_across_a_select_under_a_compressed_selector(L, p128_keys, p128_gallery):
    """the first select makes the image (upload, expand, transform) and still names no slot and forces no flush: the
    counters stand still across it, and the gates' words afterwards are those of the same program without the select"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits, gallery = p128_gallery
    L.tfhe_hip_set_encrypt_seed(79)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()

    def program(with_select):
        g = api.CiphertextArray(pp, 3)
        api.gate_batch("AND", g, a, b, ks)
        if with_select:
            sel = api.Selector.from_compressed(pp, api.tgsw_encrypt_bits_compressed([0, 1, 0], ks, seed=0xA))
            before = api.stats()
            out = api.ring_select(sel, gallery)               # first use: the image is made here
            after = api.stats()
            for f in ("blind_rotates", "keyswitches", "levels", "flushes", "br_launches", "linear_ops"):
                assert after[f] == before[f], f
            assert sel.upload_bytes() == 3 * 2 * pp.l * pp.N * 4
            assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[2])
            sel.close()
        r0 = api.stats()["blind_rotates"]
        words = g.words()
        assert api.stats()["blind_rotates"] - r0 == 3             # they ran now, at the observation
        assert list(g.decrypt(ks)) == [0, 1, 0]
        g.close()
        return words

    assert_words(program(True), program(False), "recorded gates with and without a compressed select in between")
    for o in (a, b):
        o.close()
