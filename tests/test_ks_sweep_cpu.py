"""The key switch over everything the library accepts, no GPU: the 81 decompositions (ks_t, ks_basebit) a key uploads
with and the LWE widths whose workgroups differ in shape.  The sweep's reference (ks_common.keyswitch_ref, from the
definition) against the oracle on the rows the GPU file runs, the product's key material against the oracle's, a
decrypt-level bound that goes through no digit code at all, the planner's key-switch form for every shape of the sweep,
and the enumeration itself.  tests/test_gpu_ks_sweep.py runs the same rows on the kernels."""
import functools

import numpy as np
import pytest

import ks_common as K

N, NL = K.N_RING, K.N_LWE


@functools.lru_cache(maxsize=None)
def lib():
    from peba1_amd import lib as L
    return L.load()


def oracle_keys(oracle, t, bb, seed, n=NL):
    l, Bgbit = K.GADGET
    return oracle.KeySet(oracle.custom_params(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=t, ks_basebit=bb, ks_stdev=K.STDEVS[0],
                                              bk_stdev=K.STDEVS[1]), seed)


def seed_of(t, bb):
    return 0x4B5 + 64 * t + bb


def loads(t, bb, tmp_path):
    """does the library take this decomposition?  unsupported_reason runs where a parameter set is read from a file"""
    from peba1_amd import api
    path = tmp_path / ("p_%d_%d" % (t, bb))
    api.ParameterSet(custom=K.custom_tuple(NL, t, bb)).save(path)
    try:
        api.ParameterSet.load(path)
        return True
    except ValueError as e:
        assert "key-switch digits out of range" in str(e), (t, bb, str(e))
        return False


def test_enumeration_is_the_librarys_and_has_its_known_members(tmp_path):
    """The accepted set is asked of the library (a parameter file of every pair of the grid is loaded or refused with the
    key-switch reason) and is the rule ks_common restates; an empty or shrunken enumeration cannot pass for a sweep."""
    from peba1_amd import api
    acc = {g for g in K.GRID if loads(*g, tmp_path)}
    assert acc == set(K.accepted_grid()) and len(acc) == 81
    for g in ((1, 1), (31, 1), (3, 8), (15, 2)):
        assert g in acc, g
    for g in ((4, 8), (16, 2), (3, 9)):
        assert g not in acc, g
    assert (3, 9) in K.GRID and (2, 12) in K.GRID
    # t bb = 32 is no parameter set at all
    for t, bb in ((4, 8), (16, 2), (32, 1), (8, 4), (2, 16), (1, 32)):
        with pytest.raises(ValueError):
            api.ParameterSet(custom=K.custom_tuple(NL, t, bb))


@pytest.mark.parametrize("bb", range(1, 9))
def test_reference_from_the_definition_equals_the_oracle(oracle, bb):
    """All accepted t of one ks_basebit, N = 1024, n = 10: on every row of the sweep's inputs keyswitch_ref gives the
    oracle's words, and the rows are what their names say."""
    ts = [t for t, b in K.accepted_grid() if b == bb]
    assert ts == list(range(1, 31 // bb + 1))
    for t in ts:
        oks = oracle_keys(oracle, t, bb, seed_of(t, bb))
        try:
            u, names = K.inputs(N, t, bb, 1000 * t + bb)
            K.check_inputs(u, names, N, t, bb)
            ref = K.keyswitch_ref(oks.ksk(), u, NL, N, t, bb)
            for r, name in enumerate(names):
                assert (oks.keyswitch(u[r]) == ref[r]).all(), ((t, bb), name)
        finally:
            oks.close()


@pytest.mark.parametrize("bb", range(1, 9))
def test_product_key_material_equals_the_oracles(oracle, bb):
    """The product's host-only keyset of every decomposition, word for word the oracle's (the [kN][t][base][n + 1] key
    upload_key compacts)."""
    from peba1_amd import api
    for t in range(1, 31 // bb + 1):
        seed = seed_of(t, bb)
        pp = api.ParameterSet(custom=K.custom_tuple(NL, t, bb))
        ks = api.SecretKeySet(pp, seed, device=False)
        oks = oracle_keys(oracle, t, bb, seed)
        try:
            assert ks.ksk().size == N * t * 2 ** bb * (NL + 1)
            for name in ("lwe_key", "tlwe_key", "bk", "ksk"):
                assert np.array_equal(getattr(ks, name)(), getattr(oks, name)()), ((t, bb), name)
        finally:
            ks.close()
            oks.close()


def centred(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


@pytest.mark.parametrize("bb", range(1, 9))
def test_key_switch_keeps_the_phase_within_rounding_and_noise(oracle, bb):
    """Through no digit code: for every decomposition with t bb >= 16 and every random row u (an LWE sample of dimension N
    under the ring key), | phase_lwe(keyswitch(u)) - phase_tlwe(u) | <= N 2^(31 - t bb) + 8 ks_stdev 2^32 sqrt(N t).  First
    term: every u_i is rounded to t bb bits, off by at most half a step 2^(32 - t bb), and meets a key bit of 0 or 1.
    Second: at most N t key rows are subtracted, each with independent Gaussian noise of ks_stdev; eight standard
    deviations of their sum.  The oracle's output and the reference's are both held to it."""
    ts = [t for t in range(1, 31 // bb + 1) if t * bb >= 16]
    assert ts, "every ks_basebit has decompositions of 16 bits and more"
    for t in ts:
        oks = oracle_keys(oracle, t, bb, seed_of(t, bb))
        try:
            s = oks.lwe_key().astype(np.int64)
            S = oks.tlwe_key().astype(np.int64)
            assert set(np.unique(s)) <= {0, 1} and set(np.unique(S)) <= {0, 1}
            u, names = K.inputs(N, t, bb, 77 * t + bb)
            rows = [r for r, name in enumerate(names) if name.startswith("random")]
            assert len(rows) == 6
            bound = N * 2 ** (31 - t * bb) + 8 * K.STDEVS[0] * 2.0 ** 32 * np.sqrt(N * t)
            assert bound < 2 ** 28, "the bound says something: well inside a gate's margin of 2^29"
            ref = K.keyswitch_ref(oks.ksk(), u[rows], NL, N, t, bb)
            for q, r in enumerate(rows):
                uu = u[r].astype(np.int64)
                before = int(uu[N]) - int((uu[:N] * S).sum())
                for who, ct in (("oracle", oks.keyswitch(u[r])), ("reference", ref[q])):
                    ct = ct.astype(np.int64)
                    after = int(ct[NL]) - int((ct[:NL] * s).sum())
                    assert abs(int(centred(after - before))) <= bound, ((t, bb), names[r], who, int(centred(after - before)), bound)
        finally:
            oks.close()


# ---- the plan ---------------------------------------------------------------------------------------------------------
TILED_N, PERGATE_N = (256, 511, 512, 767, 1024), (10, 255, 768, 1023)
PLAN_TUNINGS = ({}, {"ks_tile": 24}, {"ks_tile": 32}, {"ks_index": 0}, {"ks_tile": 0}, {"ks_max_splits": 32},
                {"ks_max_splits": 64}, {"ks_split_ties": 1}, {"ks_max_splits": 1})


def test_plan_names_the_kernel_that_runs_for_every_row_width():
    """(8, 2) keys: the tiled kernels exist for workgroups of 128, 192 and 320 threads; a key of another width is planned
    as what it runs -- the per-gate kernel under the narrow-launch split rule, in one chunk."""
    plan = functools.partial(K.ks_plan, lib())
    for n in TILED_N:
        assert K.threads(n) in (128, 192, 320), n
        for cu in (64, 256, 304):
            for tile in (16, 24, 32):
                for count in (2 * tile, 2 * tile + 1, 77, 4096, 8192, 20000):
                    if count < 2 * tile:
                        continue
                    tiled, tl, chunk, first, last, nbytes, form = plan(n, 8, 2, {"ks_tile": tile}, cu, count)
                    assert (tiled, tl, chunk, form) == (1, tile, 8192, K.INDEX), (n, cu, tile, count)
                    assert 16 <= first <= 48 and -(-N // first) <= 64, (n, cu, tile, count, first)
                tiled, tl, chunk, first, last, nbytes, form = plan(n, 8, 2, {"ks_tile": tile, "ks_index": 0}, cu, 77)
                assert (tiled, tl, form) == (1, 16, K.STRIP) and -(-N // first) <= 64, (n, cu, tile)
                assert plan(n, 8, 2, {"ks_tile": tile}, cu, 2 * tile - 1)[:3] + plan(n, 8, 2, {"ks_tile": tile}, cu, 2 * tile - 1)[6:] == (
                    0, 0, 2 * tile - 1, K.PERGATE)
    for n in PERGATE_N:
        assert K.threads(n) in (64, 256), n
        stride = (n + 1 + 3) & ~3
        for cu in (64, 256, 304):
            for tunings in ({}, {"ks_tile": 24}, {"ks_tile": 32}, {"ks_index": 0}):
                for count in (32, 48, 64, 77, 4096, 8192, 20000):
                    tiled, tl, chunk, first, last, nbytes, form = plan(n, 8, 2, tunings, cu, count)
                    assert (tiled, tl, chunk, form) == (0, 0, count, K.PERGATE), (n, cu, tunings, count)
                    # the narrow-launch rule: ranges double while twice the workgroups stay within 32768, past 48 once
                    want = 1
                    while want < 48 and count * want * 2 <= 32768:
                        want *= 2
                    assert first == last == want and nbytes == (count * want * stride * 4 if want > 1 else 0), (n, cu, count)


@pytest.mark.parametrize("bb", range(1, 9))
def test_every_other_decomposition_is_planned_per_gate(bb):
    """Every accepted pair but (8, 2), at every count, tuning and width class: the per-gate kernel, one chunk."""
    plan = functools.partial(K.ks_plan, lib())
    counts = sorted(set(range(1, 100)) | {128, 1000, 4096, 8191, 8192, 8193, 20000})
    for t in range(1, 31 // bb + 1):
        if (t, bb) == (8, 2):
            continue
        for n in (NL, 256, 630, 1024):
            for tunings in PLAN_TUNINGS:
                for count in counts:
                    tiled, tl, chunk, first, last, nbytes, form = plan(n, t, bb, tunings, 256, count)
                    assert (tiled, tl, chunk, form) == (0, 0, count, K.PERGATE) and first == last, ((t, bb), n, tunings, count)


@pytest.mark.parametrize("n", sorted(set(TILED_N + PERGATE_N + K.ROW_WIDTHS)))
def test_ks_partial_bytes_cover_every_chunk_of_every_row_width(n):
    """test_launch_plan_cpu.test_ks_partial_bytes_cover_every_chunk for the widths of the sweep, and for the two widest
    other decompositions at them: the partial sums execute() sizes hold count x ranges x ct_stride words of every chunk
    launch_ks launches, the last chunk of a tiled launch runs what the rule gives its own width, no tiled range is longer
    than 64 coefficients."""
    plan = functools.partial(K.ks_plan, lib())
    stride = (n + 1 + 3) & ~3
    counts = sorted(set(range(1, 200)) | set(range(200, 20000, 389)) |
                    {m * t + d for t in (16, 24, 32) for m in (1, 2, 3, 100, 511, 512, 513) for d in (-1, 0, 1)} |
                    {m * 8192 + d for m in (1, 2, 3) for d in (-1, 0, 1)})
    for t, bb in ((8, 2), (3, 8), (31, 1)):
        for tunings in PLAN_TUNINGS:
            for cu in (64, 256, 304):
                for count in counts:
                    tiled, tile, chunk, first, last, nbytes, form = plan(n, t, bb, tunings, cu, count)
                    where = (n, (t, bb), tunings, cu, count)
                    nchunks = -(-count // chunk)
                    last_cnt = count - (nchunks - 1) * chunk
                    assert chunk == (8192 if tiled else count) and 1 <= last_cnt <= chunk, where
                    assert tiled == (form != K.PERGATE) and (tile > 0) == bool(tiled), where
                    need = [cnt * s * stride * 4 for cnt, s in ((min(chunk, count), first), (last_cnt, last)) if s > 1]
                    assert nbytes == max(need, default=0), where
                    # every chunk's own plan: what launch_ks asks the rule for chunk by chunk
                    assert last == plan(n, t, bb, tunings, cu, last_cnt)[3], where
                    if tiled:
                        assert (t, bb) == (8, 2) and K.threads(n) in (128, 192, 320), where
                        assert tile in (16, 24, 32) and count >= 2 * tile, where
                        assert max(2, -(-N // 64)) <= first <= dict(K.KS_DEFAULTS, **tunings)["ks_max_splits"], where
