"""An exhausted card at EVERY allocation of every upload path of a resident device image: a plain cloud key, a
seed-compressed cloud key, a plain and a seeded packing key, a selector and a public gallery.  For each path the cap
(tfhe_hip_test_set_alloc_cap) is put between every two allocations in turn: the first use fails, names the allocation that
failed, holds nothing (tfhe_hip_test_alloc_held, to the byte) and counts nothing; with the cap lifted the same first use
gives the reference's words, holds exactly the bytes the image keeps, and deleting the object gives them back.

The sizes are restated here from the parameter set (N = 1024, n = 16, l = 2, ks 8 x 2 bits), in the order the engine
allocates: the twiddle tables are 24 N words, an NTT image two words per raw word, a staging copy the raw words, the bodies
of a seeded form the words that travelled.  Every object has a twin of the same shape that is used first, so that the slot
pool and the grow-only scratch buffers stand before anything is measured."""
import numpy as np
import pytest

import compressed_common as K
import pack_common as P
import public_common as PB
import select_common as S

pytestmark = pytest.mark.gpu

N_LWE, N_RING, GADGET = 16, 1024, (2, 10)
TW = 24 * N_RING * 4                                          # the twiddle tables, bytes
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def assert_words(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got[bad[:3]], want[bad[:3]])


class Env:
    """the parameter set, a device keyset (every path's twin, and the cloud key the packing keys are used under), the
    compressed form of a second key with its host words, and the operands and reference words, made once"""

    def __init__(self, oracle):
        from peba1_amd import api
        self.pp = pp = api.ParameterSet(custom=K.custom_tuple(N_LWE, N=N_RING, gadget=GADGET))
        self.sh = K.Shape(pp)
        self.ks = api.SecretKeySet(pp, 0xA110C, device=True)
        other = api.SecretKeySet(pp, 0xA110D, device=False)
        self.ck = api.CompressedCloudKey.generate_seeded(other, K.NOISE_SEED, K.MASK_SEED)
        other.close()
        rng = np.random.default_rng(41)
        # the keys: two rotations under the second key's words, by the oracle's schoolbook evaluator
        self.lin = rng.integers(I32_MIN, I32_MAX + 1, size=(2, pp.n + 1), dtype=np.int64).astype(np.int32)
        host = self.ck.expand_host()
        self.ksk_words = host.ksk().copy()
        oks = oracle.KeySet(oracle.custom_params(n=N_LWE, N=N_RING, l=GADGET[0], Bgbit=GADGET[1]), 1)
        oks.bk()[:] = host.bk()
        oks.ksk()[:] = self.ksk_words
        host.close()
        self.rotated = np.stack([oks.bootstrap_woks(x, use_ntt=False) for x in self.lin])
        # the packing keys: five samples of random words
        self.samples = rng.integers(I32_MIN, I32_MAX + 1, size=(5, pp.n + 1), dtype=np.int64).astype(np.int32)
        # the selector: bits (1, 0) over a gallery of three
        self.sel_words = api.tgsw_encrypt_bits([1, 0], self.ks, seed=43)
        self.ring = S.random_ring(rng, 3, pp.N)
        self.selected = S.tree(self.sel_words, self.ring, pp.l, pp.Bgbit)
        # the gallery: two polynomials, pairwise with two ring samples
        T = api.public_max_coef(pp.N)
        self.polys = rng.integers(-T, T + 1, size=(2, pp.N)).astype(np.int32)
        self.products = PB.products(self.polys, self.ring[:2])

    def close(self):
        self.ck.close()
        self.ks.close()


@pytest.fixture(scope="module")
def env(oracle):
    e = Env(oracle)
    yield e
    e.close()


# ---- the six paths: make() -> the object; use(object) -> the words of its first use (RuntimeError when refused);
# check(object, words); allocs: (label, bytes) in the engine's order; kept: how many of them the image keeps; counted: the
# stats that move, once, at the first successful use ----
def key_path(e, compressed):
    from peba1_amd import api
    sh = e.sh
    ksk = (sh.ksk_body_words + 1) * sh.stride * 4

    def check(key, words):
        assert_words(words, K.compact_ksk(e.ksk_words, sh), "compact KSK against its restatement")
        assert_words(api.kernel_bootstrap_woks(key, e.lin), e.rotated, "rotations against the oracle")

    allocs = [("the twiddle tables of a key", TW), ("the bootstrapping-key image", sh.bk_words * 2 * 4),
              ("the key-switching key", ksk), ("the staging copy of the bootstrapping key", sh.bk_words * 4)]
    if compressed:
        allocs += [("the bodies of a compressed bootstrapping key", sh.bk_body_words * 4),
                   ("the bodies of a compressed key-switching key", sh.ksk_body_words * 4)]
    return dict(make=e.ck.expand if compressed else e.ck.expand_host, twin=lambda: (api.key_image(e.ks, 1), api.kernel_bootstrap_woks(e.ks, e.lin)),
                use=lambda key: api.key_image(key, 1), check=check, allocs=allocs, kept=3,
                counted=({"expanded_keys": 1, "expand_launches": 2} if compressed else {}))


def pack_path(e, seeded):
    from peba1_amd import api
    pp = e.pp
    raw = pp.n * pp.ks_t * 2 * pp.N * 4                        # rows [n][t][2][N], the set's own decomposition

    def make():
        if not seeded:
            return api.PackingKey(e.ks, seed=44)
        ck = api.CompressedPackingKey.generate_seeded(e.ks, K.NOISE_SEED, K.MASK_SEED)
        key = ck.expand()
        ck.close()
        return key

    def check(key, words):
        assert (key.t, key.basebit) == (pp.ks_t, pp.ks_basebit)
        assert_words(words, P.pack_ref(P.KeyRows(key.words()), e.samples, key.basebit), "pack against its restatement")

    allocs = [("the NTT image of a packing key", 2 * raw), ("the staging copy of a packing key", raw)]
    if seeded:
        allocs.append(("the bodies of a compressed packing key", raw // 2))

    def twin():
        key = api.PackingKey(e.ks, seed=45)
        api.kernel_pack(key, e.ks, e.samples)
        key.close()

    return dict(make=make, twin=twin, use=lambda key: api.kernel_pack(key, e.ks, e.samples), check=check, allocs=allocs, kept=1,
                counted=({"expanded_packing_keys": 1, "packing_expand_launches": 1} if seeded else {}))


def selector_path(e):
    from peba1_amd import api
    pp = e.pp
    raw = 2 * (pp.k + 1) * pp.l * (pp.k + 1) * pp.N * 4       # rows [2 bits][(k+1) l][k+1][N]

    def twin():
        sel = api.Selector(pp, api.tgsw_encrypt_bits([0, 1], e.ks, seed=46))
        api.ring_select(sel, e.ring)
        sel.close()

    return dict(make=lambda: api.Selector(pp, e.sel_words), twin=twin, use=lambda sel: api.ring_select(sel, e.ring),
                check=lambda sel, words: assert_words(words, e.selected, "the tree against its restatement"),
                allocs=[("the twiddle tables of a selector", TW), ("the NTT image of a selector", 2 * raw),
                        ("the staging copy of a selector", raw)], kept=2, counted={})


def gallery_path(e):
    from peba1_amd import api
    pp = e.pp
    raw = 2 * pp.N * 4                                         # two polynomials

    def twin():
        g = api.PublicGallery(pp, e.polys[::-1])
        api.ring_mul_public(g, e.ring[:2])
        g.close()

    return dict(make=lambda: api.PublicGallery(pp, e.polys), twin=twin, use=lambda g: api.ring_mul_public(g, e.ring[:2]),
                check=lambda g, words: assert_words(words, e.products, "the products against their restatement"),
                allocs=[("the twiddle tables of a public gallery", TW), ("the NTT image of a public gallery", 2 * raw),
                        ("the staging copy of a public gallery", raw)], kept=2, counted={})


PATHS = {"plain key": lambda e: key_path(e, False), "compressed key": lambda e: key_path(e, True),
         "plain packing key": lambda e: pack_path(e, False), "seeded packing key": lambda e: pack_path(e, True),
         "selector": selector_path, "gallery": gallery_path}


@pytest.mark.parametrize("name", list(PATHS))
def test_exhaustion_at_every_allocation_of_an_upload_path(env, name):
    from peba1_amd import api, lib
    L = lib.load()
    path = PATHS[name](env)

    def stats():
        return {**api.expand_stats(), **api.seeded_stats()}

    path["twin"]()                                            # the pool and the scratch this first use needs stand from here on
    obj = path["make"]()
    try:
        held0 = L.tfhe_hip_test_alloc_held()
        assert held0 > 0
        before = stats()
        sizes = [b for _, b in path["allocs"]]
        for k, (label, _) in enumerate(path["allocs"]):
            L.tfhe_hip_test_set_alloc_cap(held0 + sum(sizes[:k]))          # allocation k + 1 of the path is the one that fails
            try:
                with pytest.raises(RuntimeError) as refused:
                    path["use"](obj)
            finally:
                L.tfhe_hip_test_set_alloc_cap(0)
            msg = str(refused.value)
            print(name, k, L.tfhe_hip_test_alloc_held() - held0, msg[:100])
            assert "out of device memory" in msg and label in msg, (k, label, msg)
            assert L.tfhe_hip_test_alloc_held() == held0, (k, label, L.tfhe_hip_test_alloc_held() - held0)
            assert stats() == before, (k, label)
        words = path["use"](obj)
        kept = sum(sizes[:path["kept"]])
        print(name, "kept", L.tfhe_hip_test_alloc_held() - held0, "expected", kept)
        assert L.tfhe_hip_test_alloc_held() == held0 + kept
        after = stats()
        assert {f: after[f] - before[f] for f in after} == {f: path["counted"].get(f, 0) for f in after}
        path["check"](obj, words)
        assert_words(path["use"](obj), words, "the second use")
        assert L.tfhe_hip_test_alloc_held() == held0 + kept and stats() == after          # the image is made once
    finally:
        L.tfhe_hip_test_set_alloc_cap(0)
        L.tfhe_hip_clear_error()                              # (the refusals' text is not left for the next test)
        obj.close()
    assert L.tfhe_hip_test_alloc_held() == held0
