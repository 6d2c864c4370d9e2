"""The matrix key switch (ks_matrix.hip) word for word against the key switch from its definition (ks_common.keyswitch_ref).

The raw entry tfhe_hip_kernel_keyswitch_matrix runs keyswitch_matrix_kernel alone at any width: N = 1024, LWE widths 10, 255,
630 and 1024 (one column tile with 12 of 32 words, eight full ones, 20 with a last one of 24, 33 with a last one of 4), gate
counts 1, 31, 32, 33, 127 and 129 (tiles of 64: partial ones, full ones, a last tile of one gate).  The keys are crafted
files: random words with the corner words of the byte-plane split (0x80, 0x7f, 0x80808080, ...) spread over a tenth of them,
so that the carry chain of the signed bytes runs in every column.  The rows: random ones; every digit 0; every digit 3; words
at the wrap of a_i + offset; and rows with ONE non-zero digit -- at the first and at the last (i, j), and for every position j
and value v at some i.  A single non-zero digit selects exactly one key row, and the key is random (no symmetry between rows
or columns): those rows pin the K-order of the int8 MFMA's A and B operands and its result map, exactly.

Then a recorded level of a P128 key through the API, wide enough for the form under ks_matrix_min = 64: the oracle's words,
ks_matrix_launches counts it, and the same level with ks_matrix = 0 gives the same words through the index form."""
import numpy as np
import pytest

import adversarial_common as A
import ks_common as K

pytestmark = pytest.mark.gpu

N = K.N_RING
CORNERS = np.array([0, 0x80, 0x7F, 0x80808080, 0x7F7F7F7F, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)
COUNTS = (1, 31, 32, 33, 127, 129)


def crafted_rows(rng):
    """129 rows [N + 1] and the index of the first random one"""
    w = lambda digits: K.word_of_digits(digits, 8, 2)
    rows = []
    rows.append(np.zeros(N + 1, dtype=np.int64))                                   # every digit 0
    rows.append(np.full(N + 1, w([3] * 8), dtype=np.int64))                        # every digit 3
    rows.append(np.full(N + 1, 0xFFFFFFFF, dtype=np.int64))                        # a_i + offset wraps to 0
    off = 2 ** (32 - 17)                                                           # the offset: half a step of the lowest digit
    rows.append(np.full(N + 1, 2 ** 32 - off, dtype=np.int64))                     # exactly at the wrap
    rows.append(np.full(N + 1, 2 ** 32 - off - 1, dtype=np.int64))                 # one below it: every digit 3
    first = np.zeros(N + 1, dtype=np.int64); first[0] = w([1] + [0] * 7)
    last = np.zeros(N + 1, dtype=np.int64); last[N - 1] = w([0] * 7 + [3])
    rows += [first, last]
    for j in range(8):
        for v in (1, 2, 3):
            r = np.zeros(N + 1, dtype=np.int64)
            r[int(rng.integers(0, N))] = w([v if q == j else 0 for q in range(8)])
            r[N] = int(rng.integers(0, 2 ** 32))
            rows.append(r)
    crafted = len(rows)
    while len(rows) < 129:
        rows.append(rng.integers(0, 2 ** 32, N + 1))
    u = np.stack(rows) % 2 ** 32
    # a mix at the front, so that every count of COUNTS holds crafted and random rows
    order = np.concatenate([np.arange(crafted, 129)[:12], np.arange(crafted), np.arange(crafted, 129)[12:]])
    u = u[order]
    return (u - ((u >> 31) << 32)).astype(np.int32)


@pytest.fixture(scope="module", params=[10, 255, 630, 1024], ids=lambda n: "n%d" % n)
def crafted(request, tmp_path_factory):
    """(n, key, rows, reference words) -- one key file, one reference per LWE width, shared by every count"""
    from peba1_amd import api
    n = request.param
    rng = np.random.default_rng(0x4D58 + n)
    ksk = rng.integers(0, 2 ** 32, (N, 8, 4, n + 1), dtype=np.uint32)
    spread = rng.random(ksk.shape) < 0.1
    ksk[spread] = CORNERS[rng.integers(0, len(CORNERS), int(spread.sum()))]
    ksk[:, :, 0, :] = 0                                                            # digit 0 contributes nothing
    ksk = ksk.view(np.int32)
    params = K.custom_tuple(n, 8, 2)
    l, Bgbit = K.GADGET
    path = tmp_path_factory.mktemp("ksm") / ("n%d.key" % n)
    A.write_cloud_key(path, params, np.zeros(n * 2 * l * 2 * N, dtype=np.int32), ksk)
    key = api.CloudKeySet.load(path)
    u = crafted_rows(rng)
    want = K.keyswitch_ref(ksk, u, n, N, 8, 2)
    yield n, key, u, want
    key.close()


@pytest.mark.parametrize("count", COUNTS)
def test_matrix_kernel_against_the_definition(crafted, count):
    from peba1_amd import api
    n, key, u, want = crafted
    before = api.ks_matrix_stats()["ks_matrix_launches"]
    got = api.kernel_keyswitch_matrix(key, u[:count])
    assert api.ks_matrix_stats()["ks_matrix_launches"] == before + 1
    assert got.shape == (count, n + 1)
    bad = np.flatnonzero((got != want[:count]).any(axis=1))
    assert bad.size == 0, ("n = %d, %d gates: rows that differ" % (n, count), bad[:8], "first words",
                           np.flatnonzero(got[bad[0]] != want[bad[0]])[:6])


def test_the_last_rows_of_a_partial_tile_at_another_offset(crafted):
    """the same rows as gates 64 .. 128 of a launch and as gates 0 .. 64 of another: a tile's place changes nothing"""
    from peba1_amd import api
    n, key, u, want = crafted
    got = api.kernel_keyswitch_matrix(key, u[64:129])
    assert (got == want[64:129]).all()


def test_a_recorded_level_takes_the_form_and_gives_the_oracles_words(oracle):
    from peba1_amd import api
    seed, G = 0x4D59, 96                                                           # a tile of 64 gates and one of 32
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, seed, device=True)
    oks = oracle.KeySet(oracle.params("P128"), seed)
    deferred = api.get_deferred()
    try:
        rng = oracle.Rng(seed + 1)
        ca, cb = oks.encrypt(rng, np.arange(G) % 2), oks.encrypt(rng, (np.arange(G) // 2) % 2)
        want = oks.gate_batch("NAND", ca, cb, nthreads=16)
        a, b = api.CiphertextArray(pp, G).set_words(ca), api.CiphertextArray(pp, G).set_words(cb)
        counters = lambda: np.array([api.stats()[f] for f in K.KS_COUNTERS] + [api.ks_matrix_stats()["ks_matrix_launches"]])
        words = {}
        for on, delta in ((1, (0, 0, 0, 1)), (0, (0, 0, 1, 0))):
            api.set_tuning("ks_matrix", on)
            api.set_tuning("ks_matrix_min", 64)
            r = api.CiphertextArray(pp, G)
            api.set_deferred(True)
            api.flush()
            before = counters()
            api.gate_batch("NAND", r, a, b, ks)
            assert api.flush() >= 0, api.last_error()
            assert tuple(counters() - before) == delta, ("ks_matrix", on, counters() - before)
            words[on] = r.words()
            api.set_deferred(deferred)
        assert (words[1] == want).all(), np.flatnonzero((words[1] != want).any(axis=1))[:8]
        assert (words[0] == words[1]).all()
    finally:
        api.set_deferred(deferred)
        api.set_tuning("ks_matrix", 1)
        api.set_tuning("ks_matrix_min", 512)
        ks.close()
        oks.close()


def test_a_level_is_sized_and_run_by_one_plan_when_the_image_cannot_be_made(oracle):
    """Engine::prepare_flush plans a wide share for the matrix form, finds no room for the key's byte-plane image (an allocation
    cap of one byte: ensure_ks_planes' handled refusal), plans it again without the image, sizes the partial sums from THAT
    plan and hands it to run_level: the flush succeeds in the index form with the oracle's words.  With the cap lifted the
    same level makes the image and runs the matrix form, same words.  A fresh P80 key (no image yet), 72 gates: a matrix tile
    of 64 and one of 8; the first flush, matrix form off, makes every scratch buffer so that the capped one needs none."""
    from peba1_amd import api, lib
    L = lib.load()
    seed, G = 0x4D5A, 72
    pp = api.ParameterSet(80)
    ks = api.SecretKeySet(pp, seed, device=True)
    oks = oracle.KeySet(oracle.params("P80"), seed)
    deferred = api.get_deferred()
    try:
        rng = oracle.Rng(seed + 1)
        ca, cb = oks.encrypt(rng, np.arange(G) % 2), oks.encrypt(rng, (np.arange(G) // 2) % 2)
        want = oks.gate_batch("NAND", ca, cb, nthreads=16)
        a, b = api.CiphertextArray(pp, G).set_words(ca), api.CiphertextArray(pp, G).set_words(cb)
        results = [api.CiphertextArray(pp, G) for _ in range(3)]                   # (before the cap: their slots exist)
        counters = lambda: np.array([api.stats()[f] for f in K.KS_COUNTERS] + [api.ks_matrix_stats()["ks_matrix_launches"]])
        api.set_deferred(True)
        api.flush()
        words = []
        # (ks_matrix, allocation cap) -> launches per gate / strip / index / matrix
        for r, (on, cap, delta) in zip(results, ((0, 0, (0, 0, 1, 0)), (1, 1, (0, 0, 1, 0)), (1, 0, (0, 0, 0, 1)))):
            api.set_tuning("ks_matrix", on)
            api.set_tuning("ks_matrix_min", 64)
            L.tfhe_hip_test_set_alloc_cap(cap)
            before = counters()
            api.gate_batch("NAND", r, a, b, ks)
            assert api.flush() >= 0, api.last_error()
            L.tfhe_hip_test_set_alloc_cap(0)
            assert tuple(counters() - before) == delta, ("ks_matrix", on, "cap", cap, counters() - before)
            words.append(r.words())
        for w in words:
            assert (w == want).all(), np.flatnonzero((w != want).any(axis=1))[:8]
    finally:
        L.tfhe_hip_test_set_alloc_cap(0)
        api.set_deferred(deferred)
        api.set_tuning("ks_matrix", 1)
        api.set_tuning("ks_matrix_min", 512)
        ks.close()
        oks.close()
