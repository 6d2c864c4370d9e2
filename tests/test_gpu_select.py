"""The private selection on the GPU.  The CMUX kernel and the tree are compared word for word with the numpy restatement
(tests/select_common.py); the worst-case magnitudes follow tests/adversarial_common.py -- rows and digits at their extremes
for every gadget a cloud key is accepted with; decryption, the way on through the unpack into a gate level and the
recorder's indifference to a select are checked by what they mean.  References are computed once and shared."""
import numpy as np
import pytest

import select_common as S

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 67)             # 67: more than one launch tail's CU granularity and a multiple of nothing


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


def params_of(name):
    from peba1_amd import api
    N, l, Bgbit = S.SETS[name]
    return api.ParameterSet(custom=S.custom_tuple(10, N=N, gadget=(l, Bgbit)))


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


# ---- the raw CMUX, word for word ----
@pytest.fixture(scope="module", params=list(S.SETS))
def raw_case(request):
    """random selector words (two bits: not honest encryptions), 67 random operand pairs and their reference under bit 1"""
    from peba1_amd import api
    N, l, Bgbit = S.SETS[request.param]
    pp = params_of(request.param)
    rng = np.random.default_rng(N + 31 * l + Bgbit)
    words = S.random_ring(rng, 2 * 2 * l, N).reshape(2, 2 * l, 2, N)
    d1, d0 = S.random_ring(rng, max(COUNTS), N), S.random_ring(rng, max(COUNTS), N)
    sel = api.Selector(pp, words)
    yield request.param, pp, sel, d1, d0, S.cmux_many(words[1], d1, d0, l, Bgbit)
    sel.close()


@pytest.mark.parametrize("count", COUNTS)
def test_raw_cmux_against_the_restatement(raw_case, count):
    from peba1_amd import api
    name, pp, sel, d1, d0, ref = raw_case
    got = api.kernel_ring_cmux(sel, 1, d1[:count], d0[:count])
    assert_words(got.reshape(count, 2, pp.N), ref[:count], (name, count))


def test_raw_cmux_of_an_honest_bit_selects(L):
    """a TGSW encryption of 1 picks d1, of 0 picks d0, at decrypt level"""
    from peba1_amd import api
    pp = params_of("P128")
    ks = api.SecretKeySet(pp, 0xC3, device=False)
    bits = np.random.default_rng(1).integers(0, 2, (2, pp.N))
    ring = [api.ring_encrypt_bits(bits[m], ks, seed=40 + m) for m in range(2)]
    sel = api.Selector(pp, api.tgsw_encrypt_bits([0, 1], ks, seed=2))
    for bit in (0, 1):
        out = api.kernel_ring_cmux(sel, bit, ring[1], ring[0])[0]
        assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[bit]), bit
    sel.close()
    ks.close()


# ---- worst-case magnitudes ----
def test_extreme_operands_are_ones_the_restatement_handles_exactly():
    """on the CPU: the restatement on rows of 0x80000000 / 0x7fffffff and digits all -Bg/2 / all Bg/2 - 1 equals the closed
    form in Python integers, at the gadget whose sum is the largest the CRT range admits (N = 1,024, l = 2, Bgbit = 10:
    2^52) and at the most rows (l = 9, Bgbit = 3); no int64 sum comes near 2^63"""
    for N, l, Bgbit in ((1024, 2, 10), (1024, 9, 3), (2048, 1, 10)):
        d0 = S.random_ring(np.random.default_rng(l), 1, N)[0]
        for word in (S.I32_MIN, S.I32_MAX):
            for which, digit in (("min", -2 ** (Bgbit - 1)), ("max", 2 ** (Bgbit - 1) - 1)):
                d1 = S.to_i32(d0.astype(np.int64) + S.extreme_difference(l, Bgbit, which))
                assert (S.decompose(S.to_i32(d1.astype(np.int64) - d0), l, Bgbit) == digit).all()
                want, most = S.extreme_closed_form(N, l, word, digit, d0)
                assert most < S.CRT_EXACT_LIMIT < 2 ** 62
                assert np.array_equal(S.cmux(np.full((2 * l, 2, N), word, dtype=np.int32), d1, d0, l, Bgbit), want)


@pytest.mark.parametrize("N,Bgbit", [(N, B) for N in (1024, 2048) for B in range(1, 13)])
def test_extreme_rows_and_digits_for_every_admissible_gadget(L, N, Bgbit):
    """All accepted l of one (N, Bgbit).  Selector bit 0 holds 0x80000000 in every word, bit 1 0x7fffffff; the operand pairs
    have every digit of d1 - d0 at -Bg/2, then at Bg/2 - 1: the four corners of the product, the first of them the exact
    magnitude of the CRT bound.  Word for word against the restatement (itself checked against Python integers above)."""
    from peba1_amd import api
    gadgets = [g for g in S.grid(N) if g[2] == Bgbit and S.cloud_key_accepted(L.tfhe_hip_test_form_admissible, g)]
    if not gadgets:
        # not a skip: no l at all is accepted for these digits, because l = 1 already leaves the CRT range
        assert not S.crt_ok(N, 1, Bgbit)
        return
    rng = np.random.default_rng(N + Bgbit)
    for _, l, _ in gadgets:
        pp = api.ParameterSet(custom=S.custom_tuple(10, N=N, gadget=(l, Bgbit)))
        words = np.empty((2, 2 * l, 2, N), dtype=np.int32)
        words[0], words[1] = S.I32_MIN, S.I32_MAX
        d0 = S.random_ring(rng, 2, N)
        d1 = np.stack([S.to_i32(d0[c].astype(np.int64) + S.extreme_difference(l, Bgbit, which)) for c, which in enumerate(("min", "max"))])
        sel = api.Selector(pp, words)
        try:
            for bit in (0, 1):
                got = api.kernel_ring_cmux(sel, bit, d1, d0).reshape(2, 2, N)
                assert_words(got, S.cmux_many(words[bit], d1, d0, l, Bgbit), ((N, l, Bgbit), "rows", bit))
        finally:
            sel.close()


# ---- the tree, word for word ----
@pytest.fixture(scope="module")
def tree_case():
    """five random selector bits and eight random ring samples at the P128 ring and gadget"""
    N, l, Bgbit = S.SETS["P128"]
    rng = np.random.default_rng(77)
    return params_of("P128"), S.random_ring(rng, 5 * 2 * l, N).reshape(5, 2 * l, 2, N), S.random_ring(rng, 8, N)


@pytest.mark.parametrize("M,d", [(1, 0), (2, 1), (3, 2), (5, 3), (8, 3), (8, 5)])
def test_tree_against_the_restatement_host_and_device_forms(L, tree_case, M, d):
    import torch
    from peba1_amd import api
    pp, words, gallery = tree_case
    N, l, Bgbit = S.SETS["P128"]
    sel = api.Selector(pp, words[:d] if d else None)
    want = S.tree(words[:d], gallery[:M], l, Bgbit)
    assert_words(api.ring_select(sel, gallery[:M]).reshape(2, N), want, ("host form", M, d))
    dev = torch.from_numpy(gallery[:M].reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_select(sel, dev, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.cpu().numpy().reshape(2, N), want, ("device form", M, d))
    assert_words(dev.cpu().numpy(), gallery[:M].reshape(-1), "the resident gallery is read only")
    assert api.last_error() == ""
    del dev, out
    sel.close()


# ---- decrypt level at P128 ----
@pytest.fixture(scope="module")
def p128_gallery(p128_keys):
    """eight ring-encrypted templates of 1,024 bits under the P128 keyset"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits = np.random.default_rng(21).integers(0, 2, (8, pp.N))
    return bits, np.stack([api.ring_encrypt_bits(bits[m], ks, seed=0x6A11 + m) for m in range(8)])


def test_p128_every_index_selects_its_template(p128_keys, p128_gallery, capsys):
    """The largest |phase error| over all indices is printed beside the computed sigma bound of three levels, 2.6e-4 (as
    seen on an MI355X: 7.4e-4, 2.8 of that bound); the one assertion is the decode margin of 1/8."""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits, gallery = p128_gallery
    sigma = (S.STDEVS[1] ** 2 + 3 * S.cmux_variance(pp.N, pp.l, pp.Bgbit, S.STDEVS[1])) ** 0.5
    worst = 0.0
    for index in range(8):
        sel = api.Selector(pp, api.tgsw_encrypt_bits([(index >> j) & 1 for j in range(3)], ks, seed=0x51D + index))
        out = api.ring_select(sel, gallery)
        sel.close()
        assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[index]), index
        ph = api.packed_phases(out, ks).astype(np.float64) / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(bits[index] == 1, 0.125, -0.125)).max())
    with capsys.disabled():
        print("\nselect P128, 8 templates, 3 levels: largest |phase error| %.3e, computed sigma bound %.3e (%.2f sigma)"
              % (worst, sigma, worst / sigma))
    assert worst < 1.0 / 8


def test_p128_selected_template_goes_through_the_unpack_into_a_gate_level(L, p128_keys, p128_gallery):
    """index 5, the gallery resident on the card: device select -> tfhe_hip_unpack_samples_device -> one level of
    bootsXOR against a known vector; all 1,024 bits decrypt right"""
    import torch
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits, gallery = p128_gallery
    known = np.random.default_rng(22).integers(0, 2, pp.N)
    sel = api.Selector(pp, api.tgsw_encrypt_bits([1, 0, 1], ks, seed=0xD5))
    dev = torch.from_numpy(gallery.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_select(sel, dev, device=True)
    a, x = api.CiphertextArray(pp, pp.N), api.CiphertextArray(pp, pp.N)
    api.unpack_device(out.data_ptr(), 1, ks, a, count=pp.N)
    L.tfhe_hip_set_encrypt_seed(0xE5)
    b = api.CiphertextArray(pp, pp.N).encrypt(known, ks)
    api.gate_batch("XOR", x, a, b, ks)
    assert list(x.decrypt(ks)) == list(bits[5] ^ known)
    assert L.tfhe_hip_stream_sync() == 0
    del dev, out
    sel.close()
    for o in (a, b, x):
        o.close()


def test_p128_template_selected_for_a_match(p128_keys):
    """identify.select_template: the selected 4-slot template decrypts to the enrolled one, from a host gallery and from
    one resident on the card"""
    import torch
    from peba1_amd import api, circuits, identify
    pp, ks, _ = p128_keys
    templates, bitsize = [[17, 200, 3, 96], [1, 2, 3, 4], [250, 0, 99, 7]], 8
    gallery = np.stack([circuits.ring_encrypt_vector(t, bitsize, ks, seed=0x7E + i) for i, t in enumerate(templates)])
    sel = api.Selector(pp, api.tgsw_encrypt_bits([0, 1], ks, seed=0xA1))
    got = identify.select_template(sel, gallery, pp, 4, bitsize, ks)
    assert [circuits.decrypt_number(s, ks) for s in got.slots] == templates[2]
    dev = torch.from_numpy(gallery.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    got = identify.select_template(sel, dev, pp, 4, bitsize, ks)
    assert [circuits.decrypt_number(s, ks) for s in got.slots] == templates[2]
    del dev
    sel.close()


def test_p128_recorded_gates_stay_pending_across_a_select(L, p128_keys, p128_gallery):
    """a select issued while gates are recorded but not flushed neither runs nor loses them: the counters of blind
    rotations, key switches, levels and flushes stand still across it, and the gates' words afterwards are those of the
    same program without the select"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    bits, gallery = p128_gallery
    L.tfhe_hip_set_encrypt_seed(78)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    sel = api.Selector(pp, api.tgsw_encrypt_bits([0, 1, 0], ks, seed=0x9))

    def program(with_select):
        g = api.CiphertextArray(pp, 3)
        api.gate_batch("AND", g, a, b, ks)
        if with_select:
            before = api.stats()
            out = api.ring_select(sel, gallery)
            after = api.stats()
            for f in ("blind_rotates", "keyswitches", "levels", "flushes", "br_launches", "linear_ops"):
                assert after[f] == before[f], f
            assert list(api.packed_decrypt(out, pp.N, ks)) == list(bits[2])
        r0 = api.stats()["blind_rotates"]
        words = g.words()
        assert api.stats()["blind_rotates"] - r0 == 3             # they ran now, at the observation
        assert list(g.decrypt(ks)) == [0, 1, 0]
        g.close()
        return words

    assert_words(program(True), program(False), "recorded gates with and without a select in between")
    sel.close()
    for o in (a, b):
        o.close()
