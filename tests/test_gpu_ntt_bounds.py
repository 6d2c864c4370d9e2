"""The searched worst inputs of the lazy wave NTT (tests/golden/ntt_bounds_inputs*.npz, written by
tests/golden/make_ntt_bounds_inputs.py) through the kernels, word for word against the exact negacyclic product in int64
integers reduced mod 2^32 (tests/public_common.py; never the model the inputs were searched on).

  public       public_kernel through api.kernel_ring_public_product (the raw product) and api.kernel_ring_public_rows at
               width 1 (ring_crt_rows reads the result); the img entries drive public_image_kernel, under a unit ring sample
  negacyclic   negacyclic_kernel and negacyclic_split_kernel through tfhe_hip_kernel_negacyclic
  gadget       cmux_kernel through api.kernel_ring_cmux and inner_kernel through api.kernel_ring_product and
               api.kernel_ring_inner_rows, at l = 9, Bgbit = 3 (N = 1024: 18 rows, the MAC limit) and l = 7, Bgbit = 4 (N = 2048:
               the last l a parameter set carries); the searched digits are forced as the digit fields of d1 - d0 (CMUX) or
               of the operand itself (product), the searched key rows are the selector's words, one selector sample an entry
  pack1, pack4 pack_kernel through api.kernel_pack at (t, basebit) = (18, 1) / (16, 1), the MAC limit, and (8, 4), the most
               rows 4-bit digits are accepted with (t basebit <= 32: t = 18 at basebit 4 does not exist); every entry of a
               ring and prime is one mask index of one pack, its digits the sample words' fields, its key rows the key's

An entry stores only the arrays its target depends on; the other operand is the last inv entry's of the same ring and prime.
The last test counts the entries that ran against the fixture's index: an entry without a test fails there."""
import glob
import os

import numpy as np
import pytest

import inner_common as IN
import pack_common as PK
import public_common as K
import select_common as S

pytestmark = pytest.mark.gpu

ARRAYS = {}
for _path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_bounds_inputs*.npz"))):
    with np.load(_path) as _z:
        ARRAYS.update({k: _z[k] for k in _z.files})
INDEX = sorted({k.rsplit("/", 1)[0] for k in ARRAYS})
RAN = set()


def entries(pipeline, N=None):
    return [e for e in INDEX if e.split("/")[0] == pipeline and (N is None or int(e.split("/")[1]) == N)]


def operand(entry, name):
    """the array `name` of an entry, or of the last inv entry of the same pipeline, ring and prime where it stores none"""
    if entry + "/" + name in ARRAYS:
        return ARRAYS[entry + "/" + name]
    pipeline, N, prime = entry.split("/")[:3]
    last = max((e for e in INDEX if e.startswith("%s/%s/%s/inv/" % (pipeline, N, prime))), key=lambda e: int(e.split("/")[4]))
    return ARRAYS[last + "/" + name]


def assert_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "words that differ", bad.size, "first", bad[:6], got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])


@pytest.fixture(scope="module", autouse=True)
def deferred():
    from peba1_amd import api
    was = api.get_deferred()
    api.set_deferred(True)
    yield
    api.set_deferred(was)


@pytest.fixture(scope="module")
def small_sets():
    """per ring size a small custom set and its device keyset (the kernels read its ring and twiddles alone)"""
    from peba1_amd import api
    made = {}
    for N in (1024, 2048):
        pp = api.ParameterSet(custom=K.custom_tuple(10, N=N, gadget=(3, 7) if N == 1024 else (3, 6)))
        made[N] = (pp, api.SecretKeySet(pp, 0xB0D5 + N, device=True))
    yield made
    for _, ks in made.values():
        ks.close()


def test_the_index_is_what_this_file_runs():
    assert INDEX and {e.split("/")[0] for e in INDEX} == {"public", "negacyclic", "gadget", "pack1", "pack4"}
    assert all(a.dtype == np.int32 for a in ARRAYS.values())


@pytest.mark.parametrize("entry", entries("public"))
def test_public_kernel_on_a_searched_input(small_sets, entry):
    from peba1_amd import api
    N, direction = int(entry.split("/")[1]), entry.split("/")[3]
    pp, _ = small_sets[N]
    q = operand(entry, "q").astype(np.int64)
    assert np.abs(q).max() <= K.max_coef(N)
    if direction == "img":                       # the gallery's own transform is the target: a unit ring sample
        ring = np.zeros((2, N), dtype=np.int32)
        ring[:, 0] = 1
    else:                                        # the searched words as the mask, the same reversed and negated as the body
        w = operand(entry, "words")
        ring = np.stack([w, K.to_i32(-w[::-1].astype(np.int64))])
    want = K.product(q, ring)
    if direction == "img":
        assert_words(want, K.to_i32(np.stack([q, q])), "q times 1")
    g = api.PublicGallery(pp, q[None])
    try:
        assert_words(api.kernel_ring_public_product(g, ring[None]).reshape(2, N), want, (entry, "raw product"))
        rows = api.kernel_ring_public_rows(g, ring, N, 1)
        assert_words(rows, K.rows(q[None], ring, N, 1), (entry, "rows at width 1"))
        assert_words(rows[:, N], want[1], (entry, "the rows' bodies are the product's body"))
    finally:
        g.close()
    assert api.last_error() == ""
    RAN.add(entry)


@pytest.mark.parametrize("N", [1024, 2048])
def test_negacyclic_kernels_on_the_searched_inputs(small_sets, N):
    """every entry of the ring in one launch of negacyclic_kernel and one of negacyclic_split_kernel"""
    from peba1_amd import api
    pp, ks = small_sets[N]
    todo = entries("negacyclic", N)
    assert todo
    ip = np.stack([operand(e, "digits")[0] for e in todo])
    tp = np.stack([operand(e, "key")[0] for e in todo])
    assert np.abs(ip.astype(np.int64)).max() <= K.max_coef(N) < 2 ** 12
    want = np.stack([K.product(ip[c], np.stack([tp[c], tp[c]]))[0] for c in range(len(todo))])
    got = api.kernel_negacyclic(ks, ip, tp)
    try:
        api.set_tuning("br_variant", 2)
        split = api.kernel_negacyclic(ks, ip, tp)
    finally:
        api.set_tuning("br_variant", -1)
    for c, e in enumerate(todo):
        assert_words(got[c], want[c], (e, "negacyclic_kernel"))
        assert_words(split[c], want[c], (e, "negacyclic_split_kernel"))
        RAN.add(e)


GADGET = {1024: (9, 3), 2048: (7, 4)}                # (l, Bgbit): the generator's, restated


def words_of_digits(dig, width, offset):
    """the 32-bit words whose digit fields of `width` bits, read after adding `offset`, are dig [fields][N] (signed digits
    come with their Bg/2 added); bits below the lowest field zero"""
    fields = sum((dig[p].astype(np.int64) << (32 - (p + 1) * width)) for p in range(len(dig)))
    return (fields - offset) % 2 ** 32


@pytest.mark.parametrize("N,prime", [(N, p) for N in (1024, 2048) for p in (0, 1)])
def test_cmux_and_inner_kernels_on_the_searched_inputs(N, prime):
    from peba1_amd import api
    l, Bgbit = GADGET[N]
    todo = [e for e in entries("gadget", N) if e.split("/")[2] == "p%d" % prime]
    assert todo and len(todo) <= 20
    pp = api.ParameterSet(custom=S.custom_tuple(10, N=N, gadget=(l, Bgbit)))
    rows = np.stack([operand(e, "key") for e in todo])                    # [entry][2 l][N]
    words = np.stack([rows, rows[:, ::-1]], axis=2)                       # polynomial 0: the searched rows; 1: the same, reversed order
    sel = api.Selector(pp, words)
    rng = np.random.default_rng(N + prime)
    try:
        for bit, e in enumerate(todo):
            dig = operand(e, "digits").astype(np.int64)                   # [2 l][N]: rows u l + p
            assert dig.shape == (2 * l, N) and dig.min() >= -2 ** (Bgbit - 1) and dig.max() < 2 ** (Bgbit - 1)
            c = S.to_i32(np.stack([words_of_digits(dig[u * l:(u + 1) * l] + 2 ** (Bgbit - 1), Bgbit, S.decomp_offset(l, Bgbit)) for u in range(2)]))
            assert (np.concatenate([S.decompose(c[u], l, Bgbit) for u in range(2)]) == dig).all()
            want = IN.product(words[bit], c, l, Bgbit)
            assert_words(api.kernel_ring_product(sel, bit, c[None]).reshape(2, N), want, (e, "inner_kernel, product"))
            M, w = N // 128, 128
            assert_words(api.kernel_ring_inner_rows(sel, bit, c[None], M, w), IN.inner_rows(want[None], M, w), (e, "inner_kernel, rows"))
            d0 = S.random_ring(rng, 1, N)[0]
            d1 = S.to_i32(d0.astype(np.int64) + c.astype(np.int64))
            assert_words(api.kernel_ring_cmux(sel, bit, d1[None], d0[None]).reshape(2, N), S.cmux(words[bit], d1, d0, l, Bgbit), (e, "cmux_kernel"))
            RAN.add(e)
    finally:
        sel.close()
    assert api.last_error() == ""


PACK = {"pack1": {1024: (18, 1), 2048: (16, 1)}, "pack4": {1024: (8, 4), 2048: (8, 4)}}      # (t, basebit): the generator's


@pytest.mark.parametrize("N,prime", [(N, p) for N in (1024, 2048) for p in (0, 1)])
@pytest.mark.parametrize("pipeline", list(PACK))
def test_pack_kernel_on_the_searched_inputs(pipeline, N, prime):
    """a set whose LWE width is the number of entries: mask index i of the pack is entry i"""
    from peba1_amd import api
    t, bb = PACK[pipeline][N]
    todo = [e for e in entries(pipeline, N) if e.split("/")[2] == "p%d" % prime]
    n = len(todo)
    assert n
    pp = api.ParameterSet(custom=PK.custom_tuple(n, N=N, gadget=(3, 7) if N == 1024 else (3, 6)))
    ks = api.SecretKeySet(pp, 0x9AC + N + prime, device=True)
    try:
        rows = np.stack([operand(e, "key") for e in todo])                # [n][t][N]
        key = np.stack([rows, rows[:, ::-1]], axis=2)                     # [n][t][2][N]
        sw = np.empty((N, n + 1), dtype=np.int32)                         # sample j holds coefficient j of every digit polynomial
        for i, e in enumerate(todo):
            dig = operand(e, "digits").astype(np.int64)
            assert dig.shape == (t, N) and dig.min() >= 0 and dig.max() < 2 ** bb
            sw[:, i] = PK.to_i32(words_of_digits(dig, bb, PK.prec_of(t, bb)))
        sw[:, n] = np.random.default_rng(N + prime).integers(-2 ** 31, 2 ** 31, N)
        got_digits = PK.digits_of(sw[:, :n], t, bb)                       # [N][n][t]
        assert all((got_digits[:, i, :].T == operand(e, "digits")).all() for i, e in enumerate(todo))
        pk = api.PackingKey.from_words(pp, t, bb, key.astype(np.int32))
        try:
            want = PK.pack_ref(PK.KeyRows(pk.words()), sw, bb)
            for ipw in (0, 1):                                            # the default grouping, and one mask index a workgroup
                assert_words(api.kernel_pack(pk, ks, sw, idx_per_wg=ipw), want, (pipeline, N, prime, ipw))
        finally:
            pk.close()
    finally:
        ks.close()
    RAN.update(todo)


def test_every_fixture_entry_ran():
    """after the tests above (the file runs whole): every entry of the fixture's index went through a kernel"""
    missing = [e for e in INDEX if e not in RAN]
    assert not missing and len(RAN) == len(INDEX), ("fixture entries that no test ran", len(missing), missing[:5])
