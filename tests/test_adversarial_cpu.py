"""The crafted-key harness (tests/adversarial_common.py) is sound, and it reaches the magnitudes the kernels are admitted
for -- as conditions, without a device: the oracle's schoolbook evaluator and an integer reference agree word for word
on every case, the accumulators loaded are the ones intended, the worst case of every parameter set has an exact
coefficient EQUAL to the bound unsupported_reason() compares with CRT_EXACT_LIMIT, and the first gadget above that
limit is refused."""
import functools
import struct

import numpy as np
import pytest

import adversarial_common as A


@functools.lru_cache(maxsize=None)
def crafted(name):
    return A.build_set(name)


@pytest.mark.parametrize("name", sorted(A.SETS))
def test_loaded_accumulators_and_digits_are_the_intended_ones(oracle, name):
    """Every loading entry, run by the oracle's schoolbook CMUX on the crafted key, leaves exactly the target accumulator
    (one-step: from the test vector; two-step: through the +1 monomial), and the oracle's decomposition of its rotated
    difference gives the wanted digits: -Bg/2 and Bg/2 - 1 only for the corner and spectral patterns, and for the tie
    patterns a digit vector that differs between a word and the word one below it."""
    cs = crafted(name)
    oks = A.oracle_twin(oracle, cs)
    N, l, Bgbit, half = cs.N, cs.l, cs.Bgbit, 1 << (cs.Bgbit - 1)
    testvec = oks.blind_rotate(np.zeros(cs.n, dtype=np.int32), 0, use_ntt=False)
    assert (testvec[:N] == 0).all() and (testvec[N:] == A.MU).all()
    op = oracle.custom_params(n=cs.n, N=N, l=l, Bgbit=Bgbit)
    # step 0 of a one-step load: the single digit -2^(Bgbit-2) at coefficient 0 of row l
    d_body = oracle.decompose(A.i32(A.rot_diff(testvec[N:].astype(np.int64), 1)), op)
    want = np.zeros((l, N), dtype=np.int32)
    want[0, 0] = -(1 << (Bgbit - 2))
    assert (d_body == want).all()
    seen, one_step_count = set(), 0
    for c in cs.cases:
        if c["ia"] in seen:
            continue
        seen.add(c["ia"])
        if c["one_step"]:
            one_step_count += 1
            acc = oks.cmux_rotate(c["ia"], 1, testvec, use_ntt=False)
        else:
            pre = oks.cmux_rotate(0, 1, testvec, use_ntt=False)
            dig = np.concatenate([oracle.decompose(A.i32(A.rot_diff(pre[u * N:(u + 1) * N].astype(np.int64), N)), op) for u in range(2)])
            assert dig[0, 0] == 1 and np.count_nonzero(dig) == 1, "two-step load: the +1 monomial"
            acc = oks.cmux_rotate(c["ia"], N, pre, use_ntt=False)
        assert (acc == c["target"].reshape(-1)).all(), (name, c["name"], "loaded accumulator")
        dig = np.concatenate([oracle.decompose(A.i32(A.rot_diff(c["target"][u].astype(np.int64), c["a"])), op) for u in range(2)])
        assert (dig == c["digits_seen"]).all(), (name, c["name"], "the oracle's digits against the definition")
        if c["digits"] is not None:
            assert (dig == c["digits"]).all() and np.isin(dig, (-half, half - 1, half - 2)).all()
            assert np.isin(dig, (-half, half - 1)).mean() > 0.99 or (c["a"] == N and l * Bgbit == 32)
        elif c["pattern"] == "tie_trunc" and l * Bgbit < 32:
            # the words at 2^(32 - l Bgbit) m - 1 decompose differently from those one above: the tie is real
            D = np.stack([A.rot_diff(c["target"][u].astype(np.int64), 1) for u in range(2)])
            below = (np.arange(N) % 3) == 0
            below[-1] = False
            for u in range(2):
                assert (A.decompose(D[u], l, Bgbit)[:, below] != A.decompose(D[u] + 1, l, Bgbit)[:, below]).any(axis=0).all()
    assert len(seen) == 42
    # gadgets that leave at least Bgbit - 1 bits below their lowest digit load everything but the ties in one step
    if 32 - l * Bgbit >= Bgbit - 1:
        assert one_step_count == 40
    else:
        assert 0 < one_step_count < 40


@pytest.mark.parametrize("name", sorted(A.SETS))
def test_oracle_schoolbook_equals_the_integer_reference_on_every_case(oracle, name):
    """The whole crafted blind rotation (load, then the step under test) by the oracle's schoolbook evaluator, against
    the unreduced int64 reference, every case and every word; np.convolve on int64 is exact, the bound is below 2^53."""
    cs = crafted(name)
    oks = A.oracle_twin(oracle, cs)
    for c in cs.cases:
        bar = oks.modswitch_ct(c["lin"])
        assert (bar[:-1] == c["bara"]).all() and bar[-1] == 0
    got = A.oracle_accumulators(oks, cs)
    changed = 0
    for c, g in zip(cs.cases, got):
        assert (g == c["expected"].reshape(-1)).all(), (name, c["name"])
        assert c["most"] <= A.crt_bound(cs.N, cs.l, cs.Bgbit)
        changed += bool((c["expected"] != c["target"]).any())
    assert changed >= len(cs.cases) - 16     # (only products that are multiples of 2^32 leave the accumulator as it was)


@pytest.mark.parametrize("name", sorted(A.SETS))
def test_reach_is_the_bound_itself(name):
    """Not a measurement: the case with all (k+1) l N digits at -Bg/2 against the constant key word -2^31 has a largest
    exact coefficient EQUAL to (k+1) l N (Bg/2) 2^31, at coefficient N - 1; its product is a multiple of 2^32 (only a
    slip of the CRT range shows in it), so a second case with digits Bg/2 - 1 (Bg/2 - 2 in the lowest field of a gadget
    that uses all 32 bits) against 2^31 - 1 gives words that are not all zero, within 2^-Bgbit+2 of the bound."""
    cs = crafted(name)
    N, l, Bgbit = cs.N, cs.l, cs.Bgbit
    half, bound = 1 << (Bgbit - 1), A.crt_bound(N, l, Bgbit)
    lo, hi = A.reach_cases(cs)
    assert lo["digits_seen"].shape == (2 * l, N) and (lo["digits_seen"] == -half).all()
    assert (cs.bk[lo["ik"]] == -(1 << 31)).all()
    assert lo["most"] == bound
    s = sum(A.negacyclic_exact(lo["digits_seen"][q], cs.bk[lo["ik"], q, 1]) for q in range(2 * l))
    assert int(s[N - 1]) == bound and int(np.abs(s).argmax()) == N - 1
    assert (s % (1 << 32) == 0).all()
    assert (cs.bk[hi["ik"]] == (1 << 31) - 1).all() and (hi["digits_seen"] >= half - 2).all()
    assert (hi["digits_seen"][[q for q in range(2 * l) if (q + 1) % l]] == half - 1).all()
    assert hi["most"] > bound * (1 - 2.0 ** (2 - Bgbit)) and (hi["expected"] != hi["target"]).any()
    assert (A.w32(hi["expected"].astype(np.int64) - hi["target"]) != 0).sum() > N


def test_frontier_sets_sit_on_the_frontier_they_are_named_for():
    """The eight frontier sets are what adversarial_common.SETS says of them, by the library's own predicate: the next l
    (or the table mode named) is outside the form, so a change to a bound of br_forms.hpp that moves a frontier fails
    here instead of leaving a set that no longer probes one."""
    from peba1_amd import lib
    fn = lib.load().tfhe_hip_test_form_admissible
    forms = lambda N, l, B: [[fn(f, N, l, B, t) for t in range(3)] for f in range(4)]
    none, every = [0, 0, 0], [1, 1, 1]
    S = {k: v[:3] for k, v in A.SETS.items()}
    assert forms(*S["l9_Bg3"]) == [none, none, none, every] and not any(map(any, forms(1024, 10, 3)))
    assert forms(*S["l7_Bg4"])[A.WIDE4] == every and forms(1024, 8, 4)[A.WIDE4] == none
    assert A.tables_run(A.WIDE4, 7, 4, 1) == 1
    assert forms(*S["l5_Bg5"])[A.WAVE8] == [1, 0, 0] and forms(*S["l5_Bg5"])[A.WIDE4] == every
    assert forms(1024, 6, 5)[A.WAVE8] == none
    # a lowest field at bit 2: every mode is admitted as the one without tables, and none is run with tables
    assert forms(*S["l5_Bg6"]) == [every] * 4 and forms(1024, 5, 5)[A.WAVE8] != every
    assert [A.tables_run(f, 5, 6, t) for f in range(4) for t in range(3)] == [0] * 12
    assert forms(*S["l1_Bg11"]) == [every, every, none, every]
    assert A.crt_bound(*S["l1_Bg11"]) == A.crt_bound(*S["N2048_l1_Bg10"]) == 1 << 52
    assert forms(*S["N2048_l7_Bg4"]) == [none, [1, 0, 1], none, none] and not any(map(any, forms(2048, 8, 4)))
    assert forms(*S["N2048_l4_Bg6"])[A.SPLIT] == every and forms(2048, 5, 5)[A.SPLIT] == [1, 0, 1]
    assert forms(*S["N2048_l1_Bg10"]) == [none, every, none, none]
    assert len({v[3] for v in A.SETS.values()}) == len(A.SETS) == 15


def _load(tmp_path, fname, chunks):
    from peba1_amd import api
    with open(tmp_path / fname, "wb") as f:
        for c in chunks:
            f.write(c if isinstance(c, bytes) else c.tobytes())
    return api.CloudKeySet.load(tmp_path / fname)


@pytest.mark.parametrize("name", ["P80", "N2048_l6_Bg4"])
def test_crafted_file_roundtrips_through_the_loader(tmp_path, name):
    from peba1_amd import api
    cs = A.build_set(name, with_cases=False)
    A.write_cloud_key(tmp_path / "crafted.key", cs.params_tuple, cs.bk, cs.ksk)
    ck = api.CloudKeySet.load(tmp_path / "crafted.key")
    p = ck.params
    assert (p.n, p.N, p.k, p.l, p.Bgbit, p.ks_t, p.ks_basebit) == cs.params_tuple[:7]
    assert np.array_equal(ck.bk(), cs.bk.reshape(-1)) and np.array_equal(ck.ksk(), cs.ksk)
    ck.save(tmp_path / "again.key")
    assert (tmp_path / "again.key").read_bytes() == (tmp_path / "crafted.key").read_bytes()
    ck.close()


def test_unsupported_reason_agrees_with_the_reach(tmp_path):
    """For every set under test the asserted maximum is below CRT_EXACT_LIMIT and the loader (which applies
    unsupported_reason, the predicate of the key upload) takes its parameter record; the first gadget of the same
    (N, l) whose bound is not below the limit is refused for that reason.  N = 2048 / l = 2 / Bgbit = 9 is the accepted
    gadget with the largest bound of its ring (2^52, as the 80-bit set at N = 1024); Bgbit = 10 (2^53) is refused."""
    assert A.CRT_EXACT_LIMIT == 134111233 * 134176769 // 100 * 36
    assert A.crt_bound(1024, 2, 10) == A.crt_bound(2048, 2, 9) == 1 << 52
    assert A.crt_bound(2048, 2, 9) < A.CRT_EXACT_LIMIT <= A.crt_bound(2048, 2, 10)

    def params_only(n, N, l, Bgbit):
        hdr, rec, _, _ = A.cloud_key_bytes((n, N, 1, l, Bgbit, A.KS_T, A.KS_BASEBIT, 2.0 ** -15, 2.0 ** -25, 0.012467),
                                           np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        return [hdr, rec]

    refused = []
    for name, (N, l, Bgbit, n) in sorted(A.SETS.items()):
        assert A.crt_bound(N, l, Bgbit) < A.CRT_EXACT_LIMIT
        # accepted: the parameter record passes (the file then ends early, which is what the loader reports)
        with pytest.raises(ValueError, match="payload size does not match"):
            _load(tmp_path, "ok.key", params_only(n, N, l, Bgbit))
        above = [b for b in range(Bgbit + 1, 13) if l * b <= 32 and A.crt_bound(N, l, b) >= A.CRT_EXACT_LIMIT]
        if above:
            assert A.crt_bound(N, l, above[0] - 1) < A.CRT_EXACT_LIMIT
            with pytest.raises(ValueError, match="exceed the exact range of the two-prime NTT"):
                _load(tmp_path, "above.key", params_only(n, N, l, above[0]))
            refused.append((N, l, above[0]))
    assert (2048, 2, 10) in refused and (1024, 2, 11) in refused and (1024, 3, 10) in refused
