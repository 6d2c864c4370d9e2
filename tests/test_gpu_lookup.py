"""The packed lookup on the GPU.  The rotated instantiation of the CMUX kernel and the lookup's launches are compared word
for word with the numpy restatement (tests/lookup_common.py over tests/select_common.py); decryption of every entry of a
packed sample, the way on through the unpack into the Hamming match, a public table through noiseless samples and the
recorder's indifference to a lookup are checked by what they mean."""
import numpy as np
import pytest

import lookup_common as K
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


def params_of(name):
    from peba1_amd import api
    N, l, Bgbit = S.SETS[name]
    return api.ParameterSet(custom=S.custom_tuple(10, N=N, gadget=(l, Bgbit)))


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


def bits_of(index, d):
    return [(index >> j) & 1 for j in range(d)]


# ---- the raw rotation step, word for word ----
@pytest.fixture(scope="module", params=list(S.SETS))
def raw_case(request):
    """a selector of two honest bits, the first encrypting 0 and the second 1, and three random operands"""
    from peba1_amd import api
    N, l, Bgbit = S.SETS[request.param]
    pp = params_of(request.param)
    ks = api.SecretKeySet(pp, 0xC3 + N, device=False)
    words = api.tgsw_encrypt_bits([0, 1], ks, seed=N + l)
    sel = api.Selector(pp, words)
    yield request.param, pp, sel, words, S.random_ring(np.random.default_rng(N + 31 * l + Bgbit), 3, N)
    sel.close()
    ks.close()


@pytest.mark.parametrize("rot", [1, 63, 64, 65, 128, "N/2", "N-1"])
def test_raw_rotation_step_against_the_restatement(raw_case, rot):
    """count 3 on random samples, and the two samples whose rotated difference has every digit at -Bg/2, then at Bg/2 - 1"""
    from peba1_amd import api
    name, pp, sel, words, d0 = raw_case
    N, l, Bgbit = S.SETS[name]
    rot = {"N/2": N // 2, "N-1": N - 1}.get(rot, rot)
    ext = []
    for which in ("min", "max"):
        poly = S.to_i32(K.sample_with_rotated_difference(N, rot, S.extreme_difference(l, Bgbit, which)))
        ext.append(np.stack([poly, poly]))                 # both polynomials carry it
    ext = np.stack(ext)
    digits = S.decompose(S.to_i32(K.rotate_ref(ext[0], rot).astype(np.int64) - ext[0])[0], l, Bgbit)
    assert (digits == -2 ** (Bgbit - 1)).all()
    for bit in (0, 1):
        for ops, what in ((d0, "random"), (ext, "extreme")):
            got = api.kernel_ring_cmux_rotate(sel, bit, rot, ops).reshape(len(ops), 2, N)
            want = np.stack([K.rot_step(words[bit], rot, c, l, Bgbit) for c in ops])
            assert_words(got, want, (name, rot, "bit", bit, what))


# ---- the lookup, word for word ----
LOOKUPS = [("P128", 1024, 3, 2), ("P128", 128, 8, 3), ("P128", 128, 20, 5), ("P128", 1, 5, 10), ("P128", 512, 3, 2),
           ("P2048", 2048, 3, 2), ("P2048", 256, 9, 4)]                 # (set, w, M, d)


@pytest.fixture(scope="module")
def lookup_words():
    """random selector words (ten bits at P128, four at P2048: not honest encryptions) and three random samples per set"""
    out = {}
    for name, d in (("P128", 10), ("P2048", 4)):
        N, l, Bgbit = S.SETS[name]
        rng = np.random.default_rng(177 + N)
        out[name] = (params_of(name), S.random_ring(rng, d * 2 * l, N).reshape(d, 2 * l, 2, N), S.random_ring(rng, 3, N))
    return out


@pytest.mark.parametrize("name,w,M,d", LOOKUPS)
def test_lookup_against_the_restatement_host_and_device_forms(L, lookup_words, name, w, M, d):
    import torch
    from peba1_amd import api
    pp, words, ring = lookup_words[name]
    N, l, Bgbit = S.SETS[name]
    R = api.lookup_samples(pp, M, w)
    gallery = ring[:R]
    sel = api.Selector(pp, words[:d])
    want = K.lookup_ref(words[:d], gallery, M, w, l, Bgbit)
    assert_words(api.ring_lookup(sel, gallery, M, w).reshape(2, N), want, ("host form", name, w, M, d))
    dev = torch.from_numpy(gallery.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    out = api.ring_lookup(sel, dev, M, w, device=True)
    assert L.tfhe_hip_stream_sync() == 0
    assert_words(out.cpu().numpy().reshape(2, N), want, ("device form", name, w, M, d))
    assert_words(dev.cpu().numpy(), gallery.reshape(-1), "the resident gallery is read only")
    if w == N:
        # word for word the select -- also directly behind a refused lookup, which leaves it as it was
        import ctypes as C
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                 # noqa: E731
        bad, flat = np.full(2 * N, 0x5A5A5A5A, dtype=np.int32), np.ascontiguousarray(gallery.reshape(-1))
        assert L.tfhe_hip_ring_lookup(sel.ptr, i32p(flat), M, N - 1, i32p(bad)) == -1 and "width must be a power of two" in api.last_error()
        L.tfhe_hip_clear_error()
        assert (bad == 0x5A5A5A5A).all()
        assert_words(api.ring_select(sel, gallery).reshape(2, N), want, ("the select", name, M, d))
    assert api.last_error() == ""
    del dev, out
    sel.close()


# ---- decrypt level at P128 ----
@pytest.fixture(scope="module")
def p128_packed(p128_keys):
    """eight 128-bit templates in ONE ring sample under the P128 keyset"""
    from peba1_amd import identify
    pp, ks, _ = p128_keys
    entries = np.random.default_rng(23).integers(0, 2, (8, 128))
    return entries, identify.pack_gallery(entries, 128, ks, seed=0x6A40)


def test_p128_every_index_of_one_packed_sample_decrypts_to_its_entry(p128_keys, p128_packed, capsys):
    """three rotation steps and no tree.  The largest |phase error| over the entries' 128 coefficients is printed beside the
    computed sqrt(3) * 1.5e-4 of three CMUX terms; the one assertion is the decode margin of 1/8."""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    entries, gallery = p128_packed
    assert gallery.shape == (1, 2 * pp.N)
    sigma = 3 ** 0.5 * 1.5e-4
    worst = 0.0
    for index in range(8):
        sel = api.Selector(pp, api.tgsw_encrypt_bits(bits_of(index, 3), ks, seed=0x52D + index))
        out = api.ring_lookup(sel, gallery, 8, 128)
        sel.close()
        assert list(api.packed_decrypt(out, 128, ks)) == list(entries[index]), index
        ph = api.packed_phases(out, ks).astype(np.float64)[:128] / 2.0 ** 32
        worst = max(worst, np.abs(ph - np.where(entries[index] == 1, 0.125, -0.125)).max())
    with capsys.disabled():
        print("\nlookup P128, 8 entries of 128 bits in one sample, 3 rotations: largest |phase error| %.3e, computed sqrt(3) * 1.5e-4 = "
              "%.3e (%.2f of it)" % (worst, sigma, worst / sigma))
    assert worst < 1.0 / 8


def test_p128_looked_up_template_goes_into_the_hamming_match(L, p128_keys, p128_packed):
    """identify.lookup_template from a gallery resident on the card, then peba1_hamming_match against a probe five bits
    from entry 6: index 6 gives a match (distance 5 <= 20: bit 0), index 3 a non-match (bit 1, the plaintext answer)"""
    import torch
    from peba1_amd import api, circuits, identify
    pp, ks, _ = p128_keys
    entries, gallery = p128_packed
    probe_bits = entries[6].copy()
    probe_bits[[3, 40, 77, 90, 127]] ^= 1
    bound, cw = 20, circuits.hamming_count_bits(128)
    dev = torch.from_numpy(gallery.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    L.tfhe_hip_set_encrypt_seed(0xE7)
    probe = api.CiphertextArray(pp, 128).encrypt(probe_bits, ks)
    enc_bound = circuits.encrypt_number(pp, bound, cw, ks)
    for index in (6, 3):
        hd = int((entries[index] ^ probe_bits).sum())
        sel = api.Selector(pp, api.tgsw_encrypt_bits(bits_of(index, 3), ks, seed=0xA7 + index))
        template = identify.lookup_template(sel, dev, 8, 128, ks)
        assert list(template.decrypt(ks)) == list(entries[index]), index
        rb = api.CiphertextArray(pp, cw)
        circuits.hamming_match(rb, probe, template, 128, enc_bound, ks)
        assert int(rb.decrypt(ks)[0]) == (1 if hd > bound else 0), (index, hd)
        sel.close()
        for o in (rb, template):
            o.close()
    assert int((entries[6] ^ probe_bits).sum()) == 5 and int((entries[3] ^ probe_bits).sum()) > bound
    del dev
    for o in (probe, enc_bound):
        o.close()


def test_p128_public_table_of_a_ten_bit_function(p128_keys):
    """a random function of ten bits as ONE noiseless sample (api.ring_trivial), w = 1: ten rotation steps, no tree; the
    result's coefficient 0 decrypts to f(x) for 16 random inputs x whose bits only the client knows"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    rng = np.random.default_rng(24)
    f = rng.integers(0, 2, pp.N)
    table = api.ring_trivial(pp, np.where(f == 1, 2 ** 29, -2 ** 29))
    for x in rng.integers(0, pp.N, 16):
        sel = api.Selector(pp, api.tgsw_encrypt_bits(bits_of(int(x), 10), ks, seed=0xF00 + int(x)))
        out = api.ring_lookup(sel, table, pp.N, 1)
        sel.close()
        assert int(api.packed_decrypt(out, 1, ks)[0]) == int(f[x]), x


def test_p128_recorded_gates_stay_pending_across_a_lookup(L, p128_keys, p128_packed):
    """a lookup issued while gates are recorded but not flushed neither runs nor loses them: the counters of blind
    rotations, key switches, levels and flushes stand still across it, and the gates' words afterwards are those of the
    same program without the lookup"""
    from peba1_amd import api
    pp, ks, _ = p128_keys
    entries, gallery = p128_packed
    L.tfhe_hip_set_encrypt_seed(79)
    a, b = api.CiphertextArray(pp, 3).encrypt([0, 1, 1], ks), api.CiphertextArray(pp, 3).encrypt([1, 1, 0], ks)
    api.flush()
    sel = api.Selector(pp, api.tgsw_encrypt_bits([0, 1, 0], ks, seed=0x19))

    def program(with_lookup):
        g = api.CiphertextArray(pp, 3)
        api.gate_batch("AND", g, a, b, ks)
        if with_lookup:
            before = api.stats()
            out = api.ring_lookup(sel, gallery, 8, 128)
            after = api.stats()
            for f in ("blind_rotates", "keyswitches", "levels", "flushes", "br_launches", "linear_ops"):
                assert after[f] == before[f], f
            assert list(api.packed_decrypt(out, 128, ks)) == list(entries[2])
        r0 = api.stats()["blind_rotates"]
        words = g.words()
        assert api.stats()["blind_rotates"] - r0 == 3             # they ran now, at the observation
        assert list(g.decrypt(ks)) == [0, 1, 0]
        g.close()
        return words

    assert_words(program(True), program(False), "recorded gates with and without a lookup in between")
    sel.close()
    for o in (a, b):
        o.close()
