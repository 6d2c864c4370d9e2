"""Seed-compressed packing keys and ring samples on the host (no GPU): the stream numbering of the key rows, the phase of
every row, reproducibility, the round trips through words and files with every refusal, and compressed ring samples
against the stream and by decryption.  Keysets are host-only; every draw is seeded, and the seeds below were confirmed to
stay inside the 6-sigma tolerances before they were committed."""
import ctypes as C
import struct

import numpy as np
import pytest

import compressed_common as K
import seeded_wire_common as W


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


def _set(n, N, gadget):
    from peba1_amd import api
    pp = api.ParameterSet(custom=W.custom_tuple(n, N=N, gadget=gadget))
    return pp, api.SecretKeySet(pp, 300 + n, device=False)


@pytest.fixture(scope="module")
def small():
    pp, sk = _set(7, 1024, (3, 7))
    yield pp, sk
    sk.close()


# ---- the packing key ----
@pytest.mark.parametrize("n,t,bb,N,gadget", W.KEY_CASES)
def test_rows_lie_where_the_stream_says_and_carry_their_message(L, n, t, bb, N, gadget):
    """mask polynomial of row (i, p) = stream words (i t + p) N ..: the first, a middle and the last row; the phase of EVERY
    row is mu on coefficient 0 and 0 elsewhere within 6 bk_stdev; the device-form key materialises the same rows"""
    from peba1_amd import api
    pp, sk = _set(n, N, gadget)
    ck = api.CompressedPackingKey.generate_seeded(sk, W.NOISE_SEED, W.MASK_SEED, t, bb)
    host, lazy = ck.expand_host(), ck.expand()
    try:
        assert (ck.t, ck.basebit, ck.body().size, ck.nbytes) == (t, bb, n * t * N, 40 + 4 * n * t * N)
        rows = host.words()
        assert rows.shape == (n, t, 2, N)
        for r in sorted({0, (n * t) // 2, n * t - 1}):
            i, p = divmod(r, t)
            W.assert_words(rows[i, p, 0].view(np.uint32), W.row_mask_ref(L, W.MASK_SEED, i, p, t, N), ("mask of row", i, p))
        W.assert_words(rows[:, :, 1, :], ck.body(), "bodies")
        ph = W.ring_phases(rows, sk.tlwe_key()).astype(np.int64)
        ph[:, :, 0] -= W.row_messages(sk.lwe_key(), t, bb)
        err = np.abs(K.centred(ph))
        assert err.max() <= W.TOL, ("row phase off its message", err.max(), W.TOL)
        assert err.max() > 0                                            # (noise was drawn)
        W.assert_words(lazy.words(), rows, "rows of the device-form key, made on demand")
        plain = api.PackingKey.from_words(pp, t, bb, rows)
        W.assert_words(plain.words(), rows, "from_words of the expanded rows")
        plain.close()
    finally:
        for o in (host, lazy, ck, sk):
            o.close()


def test_reproducible_forms_fresh_seeds_and_an_untouched_keyset(L, small):
    from peba1_amd import api
    pp, sk = small
    held = [np.array(x()) for x in (sk.lwe_key, sk.tlwe_key, sk.bk, sk.ksk)]
    a = api.CompressedPackingKey.generate_seeded(sk, 1, W.MASK_SEED)
    b = api.CompressedPackingKey.generate_seeded(sk, 1, W.MASK_SEED)
    c = api.CompressedPackingKey.generate_seeded(sk, 2, W.MASK_SEED)
    d, e = api.CompressedPackingKey.generate(sk), api.CompressedPackingKey.generate(sk)
    assert (a.t, a.basebit) == (pp.ks_t, pp.ks_basebit)                  # 0, 0 = the set's own
    W.assert_words(a.body(), b.body(), "seeded form, twice")
    W.assert_words(a.seed(), W.MASK_SEED, "the seed as given")
    assert (np.asarray(a.body()) != np.asarray(c.body())).any()
    assert (d.seed() != e.seed()).any() and (d.seed() != W.MASK_SEED).any()
    mu = np.zeros(pp.N, dtype=np.int32)
    s1 = api.ring_encrypt(mu, sk, seed=5, compressed=True, mask_seed=W.MASK_SEED)
    s2 = api.ring_encrypt(mu, sk, seed=5, compressed=True, mask_seed=W.MASK_SEED)
    f1, f2 = api.ring_encrypt(mu, sk, compressed=True), api.ring_encrypt_bits([1], sk, compressed=True)
    W.assert_words(s1, s2, "seeded sample, twice")
    assert (f1[:10] != f2[:10]).any() and (f1[:10] != s1[:10]).any()
    # the default form's rows are rows too
    rows = d.expand_host()
    ph = W.ring_phases(rows.words(), sk.tlwe_key()).astype(np.int64)
    ph[:, :, 0] -= W.row_messages(sk.lwe_key(), d.t, d.basebit)
    assert np.abs(K.centred(ph)).max() <= 7 * W.SIGMA                   # (unseeded draws: 57,344 samples, one more sigma)
    rows.close()
    again = api.SecretKeySet(pp, 307, device=False)
    for was, now, fresh in zip(held, (sk.lwe_key, sk.tlwe_key, sk.bk, sk.ksk), (again.lwe_key, again.tlwe_key, again.bk, again.ksk)):
        W.assert_words(now(), was, "keyset words after these objects were made")
        W.assert_words(fresh(), was, "a keyset of the same seed made afterwards")
    for o in (a, b, c, d, e, again):
        o.close()


def test_words_and_file_round_trips(L, small, tmp_path):
    from peba1_amd import api
    pp, sk = small
    ck = api.CompressedPackingKey.generate_seeded(sk, 3, W.MASK_SEED, 4, 3)
    back = api.CompressedPackingKey.from_words(pp, 4, 3, ck.seed(), ck.body())
    W.assert_words(back.body(), ck.body(), "from_words bodies")
    W.assert_words(back.seed(), ck.seed(), "from_words seed")
    assert (back.t, back.basebit, back.nbytes) == (4, 3, ck.nbytes)
    ck.save(tmp_path / "p.key")
    assert (tmp_path / "p.key").stat().st_size == 24 + 56 + 8 + ck.nbytes
    loaded = api.CompressedPackingKey.load(tmp_path / "p.key", pp)
    W.assert_words(loaded.body(), ck.body(), "file bodies")
    W.assert_words(loaded.seed(), ck.seed(), "file seed")
    assert (loaded.t, loaded.basebit) == (4, 3)
    loaded.save(tmp_path / "q.key")
    assert (tmp_path / "q.key").read_bytes() == (tmp_path / "p.key").read_bytes()
    h1, h2 = loaded.expand_host(), ck.expand_host()
    W.assert_words(h1.words(), h2.words(), "rows of the loaded key")
    for o in (h1, h2, loaded, back, ck):
        o.close()


def test_hostile_files_are_refused_without_effect(L, small, tmp_path):
    """wrong magic / version / kind, a truncation inside every field, a declared size that does not match, a decomposition
    the constructors refuse: NULL, the error set, and the next load works"""
    from peba1_amd import api
    pp, sk = small
    ck = api.CompressedPackingKey.generate_seeded(sk, 3, W.MASK_SEED, 2, 2)
    ck.save(tmp_path / "p.key")
    blob = (tmp_path / "p.key").read_bytes()
    cc = api.CompressedCloudKey.generate_seeded(sk, 3, W.MASK_SEED)
    cc.save(tmp_path / "cloud.key")
    hdr, rec, dec, rest = blob[:24], blob[24:80], blob[80:88], blob[88:]
    resized = hdr[:16] + struct.pack("<Q", len(blob) - 24 + 4)
    cases = {
        "magic": (b"XFHP" + blob[4:], "not a libtfhe-hip file"),
        "version": (blob[:4] + struct.pack("<I", 2) + blob[8:], "unsupported file version"),
        "kind": ((tmp_path / "cloud.key").read_bytes(), "expected 6"),
        "size": (resized + blob[24:] + b"\0\0\0\0", "payload size does not match"),
        "t19": (hdr + rec + struct.pack("<2i", 19, 1) + rest, "accumulator"),
        "base5": (hdr + rec + struct.pack("<2i", 2, 5) + rest, "1..4 bits"),
        "cut_header": (blob[:20], "short read"),
        "cut_params": (blob[:50], "short read"),
        "cut_decomposition": (blob[:84], "short read"),
        "cut_seed": (blob[:100], "short read"),
        "cut_body": (blob[:len(blob) - 4], "short read"),
    }
    for name, (data, why) in cases.items():
        (tmp_path / name).write_bytes(data)
        L.tfhe_hip_clear_error()
        with pytest.raises(ValueError, match="cannot load a compressed packing key"):
            api.CompressedPackingKey.load(tmp_path / name, pp)
        assert why in api.last_error(), (name, api.last_error())
    with pytest.raises(ValueError):
        api.CompressedCloudKey.load(tmp_path / "p.key")                    # and the other way round
    ok = api.CompressedPackingKey.load(tmp_path / "p.key", pp)
    W.assert_words(ok.body(), ck.body(), "a good file after the hostile ones")
    for o in (ok, cc, ck):
        o.close()


def test_refused_decompositions_and_null_arguments(L, small):
    from peba1_amd import api, lib
    pp, sk = small
    seed = W.MASK_SEED.ctypes.data_as(lib.U32P)
    body = np.zeros(7 * 19 * 1024, dtype=np.int32)
    bp = body.ctypes.data_as(lib.I32P)
    mu = np.zeros(pp.N, dtype=np.int32)
    mp = mu.ctypes.data_as(lib.I32P)
    out = np.full(2 * pp.N, 7, dtype=np.int32)
    op = out.ctypes.data_as(lib.I32P)
    refusals = [
        (lambda: L.tfhe_hip_new_compressed_packing_key(sk.ptr, 19, 1), None, "accumulator"),
        (lambda: L.tfhe_hip_new_compressed_packing_key(sk.ptr, 2, 5), None, "1..4 bits"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_seeded(sk.ptr, 19, 1, 1, seed), None, "accumulator"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_from_words(pp.ptr, 19, 1, seed, bp), None, "accumulator"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_from_words(pp.ptr, 2, 5, seed, bp), None, "1..4 bits"),
        (lambda: L.tfhe_hip_new_compressed_packing_key(None, 0, 0), None, "null"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_seeded(sk.ptr, 0, 0, 1, None), None, "null"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_seeded(None, 0, 0, 1, seed), None, "null"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_from_words(None, 0, 0, seed, bp), None, "null"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_from_words(pp.ptr, 0, 0, None, bp), None, "null"),
        (lambda: L.tfhe_hip_new_compressed_packing_key_from_words(pp.ptr, 0, 0, seed, None), None, "null"),
        (lambda: L.tfhe_hip_expand_packing_key(None), None, "null"),
        (lambda: L.tfhe_hip_expand_packing_key_host(None), None, "null"),
        (lambda: L.tfhe_hip_compressed_packing_key_seed(None), None, "null"),
        (lambda: L.tfhe_hip_compressed_packing_key_bytes(None), -1, "null"),
        (lambda: L.tfhe_hip_compressed_packing_key_decomposition(None, None, None), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_compressed(None, mp, op), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_compressed(sk.ptr, None, op), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_compressed(sk.ptr, mp, None), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_compressed_seeded(sk.ptr, mp, op, None, 1), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_bits_compressed(sk.ptr, None, 1, op), -1, "null"),
        (lambda: L.tfhe_hip_ring_encrypt_bits_compressed(sk.ptr, mp, 0, op), -1, "count must be in 1..1024"),
        (lambda: L.tfhe_hip_ring_encrypt_bits_compressed_seeded(sk.ptr, mp, pp.N + 1, op, seed, 1), -1, "count must be in 1..1024"),
        (lambda: L.tfhe_hip_ring_expand_host(None, pp.N, op), -1, "null"),
        (lambda: L.tfhe_hip_ring_expand_host(mp, pp.N, None), -1, "null"),
        (lambda: L.tfhe_hip_ring_expand_host(mp, 0, op), -1, "at least 1"),
    ]
    for k, (call, want, why) in enumerate(refusals):
        L.tfhe_hip_clear_error()
        got = call()
        assert (not got) if want is None else (got == want), (k, got)
        assert why in api.last_error(), (k, api.last_error())
    assert (out == 7).all()                                             # no refused call wrote its output
    cnt = C.c_int64(5)
    assert not L.tfhe_hip_compressed_packing_key_body(None, C.byref(cnt)) and cnt.value == 0
    L.tfhe_hip_delete_compressed_packing_key(None)                      # a no-op
    with pytest.raises(ValueError, match="body words"):
        api.CompressedPackingKey.from_words(pp, 2, 2, W.MASK_SEED, np.zeros(5, dtype=np.int32))
    L.tfhe_hip_clear_error()


def test_counters_read_zero_without_a_device(L):
    from peba1_amd import api
    assert set(api.seeded_stats()) == {"expanded_packing_keys", "packing_expand_launches", "seeded_unpacked_samples",
                                       "seeded_unpack_launches"}


# ---- compressed ring samples ----
@pytest.mark.parametrize("N,gadget", [(1024, (3, 7)), (2048, (2, 8))])
def test_compressed_sample_expands_to_the_stream_and_decrypts(L, N, gadget):
    from peba1_amd import api
    pp, sk = _set(10, N, gadget)
    rng = np.random.default_rng(N)
    mu = rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(np.int32)
    c = api.ring_encrypt(mu, sk, seed=9, compressed=True, mask_seed=W.MASK_SEED)
    assert c.shape == (10 + N,)
    W.assert_words(c[:10].view(np.uint32), W.MASK_SEED, "the record starts with its seed")
    x = api.ring_expand(c, N)[0]
    W.assert_words(x[:N].view(np.uint32), K.stream_words(L, W.MASK_SEED, 0, N), "mask = stream words 0 .. N-1")
    W.assert_words(x[N:], c[10:], "body")
    W.assert_words(x, W.ring_expand_ref(L, c, N), "the restatement")
    err = np.abs(K.centred(api.packed_phases(x, sk).astype(np.int64) - mu))
    assert 0 < err.max() <= W.TOL, err.max()
    for count in (1, N - 1, N):
        bits = rng.integers(0, 2, count)
        cb = api.ring_encrypt_bits(bits, sk, seed=10 + count, compressed=True, mask_seed=W.seed_of(count))
        xb = api.ring_expand(cb, N)[0]
        assert api.packed_decrypt(xb, count, sk).tolist() == bits.tolist()
        ph = api.packed_phases(xb, sk).astype(np.int64)
        assert np.abs(np.abs(ph[:count]) - 2 ** 29).max() <= W.TOL
        assert count == N or np.abs(ph[count:]).max() <= W.TOL          # noise only from `count` on
    fresh = api.ring_encrypt_bits([1, 0, 0, 1], sk, compressed=True)
    assert api.packed_decrypt(api.ring_expand(fresh, N)[0], 4, sk).tolist() == [1, 0, 0, 1]
    sk.close()
