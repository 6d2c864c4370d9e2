"""The three-input bootstrapped gates (tfhe_hip_gate3: MAJ3, XOR3, XNOR3 -- not in upstream TFHE's API) and the
circuits built from them, without a GPU: the level plan of DAGs that hold them, the carry-save circuits over the
plaintext provider (their fallback to two-input gates), and over a netlist provider that HAS the three-input gate --
replayed word for word through the CPU oracle, counted, and pinned by a digest the GPU test must reproduce."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import gate3_common as G

ROOT = G.ROOT
NOT, MUX = 17, 16
GATE_LIN = [(1, -1, -1), (1, 1, 1), (-1, 1, 1), (-1, -1, -1), (2, 2, 2), (-2, -2, -2),
            (-1, -1, 1), (-1, 1, -1), (1, -1, 1), (1, 1, -1)]          # (c0 in eighths, sa, sb), tfhe boot-gates.cpp
MU = 1 << 29


def _plan(ops, keys, nkeys, entry, rot_words, unit=256, balance=0):
    from peba1_amd import lib
    L = lib.load()
    n = len(ops)
    flat = np.array(ops, dtype=np.int32).reshape(-1)
    k = np.array(keys, dtype=np.int32)
    lv = np.zeros(n, dtype=np.int32)
    sizes = np.zeros(6, dtype=np.int32)
    rot_off, ks_off = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    rot_koff, ks_koff = np.zeros(n * nkeys + 1, dtype=np.int32), np.zeros(n * nkeys + 1, dtype=np.int32)
    rot_key = np.zeros(2 * n, dtype=np.int32)
    rots = np.full(rot_words * 2 * n, -99, dtype=np.int32)
    kss = np.zeros(4 * n, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(lib.I32P)
    levels = getattr(L, entry)(p(flat), p(k), n, nkeys, unit, balance, p(lv), p(sizes), p(rot_off), p(ks_off),
                               p(rot_koff), p(ks_koff), p(rot_key), p(rots), p(kss))
    assert levels >= 0, L.tfhe_hip_last_error()
    nrot, nks = int(sizes[1]), int(sizes[2])
    return dict(levels=levels, lvl=lv, sizes=sizes, rot_off=rot_off[:levels + 1], ks_off=ks_off[:levels + 1],
                rot_koff=rot_koff[:sizes[3]], ks_koff=ks_koff[:sizes[4]], rot_key=rot_key[:sizes[5]],
                rots=rots[:rot_words * nrot].reshape(nrot, rot_words), rots_raw=rots, kss=kss[:4 * nks].reshape(nks, 4))


def _g3(name, mask):
    return 32 + 8 * G.GATE3[name][0] + mask


def _mixed_dag():
    """Slots 0..5 are inputs.  Two-input gates, a NOT, a MUX and all three new kinds under all eight masks; the last
    level reads results of the three-input gates in every operand position."""
    ops = [(2, 10, 0, 1, -1), (4, 11, 2, 3, -1), (NOT, 12, 10, -1, -1), (MUX, 13, 11, 0, 1)]
    slot = 20
    first = {}
    for name in ("MAJ3", "XOR3", "XNOR3"):
        for mask in range(8):
            ops.append((_g3(name, mask), slot, 10, 12, 4 + mask % 2))        # third operand: an input slot
            first[(name, mask)] = slot
            slot += 1
    # consumers: the third slot is a result of level 2 (and of a MUX), so they belong to level 3 or later
    ops.append((_g3("MAJ3", 1), slot, 0, 1, first[("XOR3", 0)])); slot += 1
    ops.append((_g3("XOR3", 6), slot, 0, first[("MAJ3", 3)], 13)); slot += 1
    ops.append((_g3("XNOR3", 0), slot, first[("XNOR3", 7)], 2, 3)); slot += 1
    ops.append((1, slot, slot - 1, slot - 2, -1))
    return ops


def test_level_plan_three_input_gates():
    """Fails on a library without the feature: no tfhe_hip_test_level_plan3, and kinds 32..55 are unknown."""
    ops = _mixed_dag()
    for nkeys in (1, 3):
        keys = [i % nkeys for i in range(len(ops))]
        P = _plan(ops, keys, nkeys, "tfhe_hip_test_level_plan3", 8)
        lvl = P["lvl"]
        producer = {op[1]: i for i, op in enumerate(ops)}
        for i, (kind, dst, a, b, c) in enumerate(ops):                      # every operand, the third included, is a dependence
            for s in (a, b, c):
                if s in producer:
                    p_ = producer[s]
                    assert (lvl[i] == lvl[p_]) if kind == NOT else (lvl[i] > lvl[p_]), (i, s, lvl[i], lvl[p_])
        # the plan restated: gates in the order (level, key, recording order)
        order = sorted((i for i, op in enumerate(ops) if op[0] != NOT), key=lambda i: (lvl[i], keys[i], i))
        want_rots, want_key = [], []
        pos_in_level = {}
        for i in order:
            kind, dst, a, b, c = ops[i]
            u = pos_in_level.get(lvl[i], 0)
            if kind == MUX:
                want_rots += [[a, b, 1, 1, -MU, u, -1, 0], [a, c, -1, 1, -MU, u + 1, -1, 0]]
                want_key += [keys[i]] * 2
                pos_in_level[lvl[i]] = u + 2
            elif kind >= 32:
                name, mask = G.GATE3_BY_CODE[(kind - 32) >> 3], (kind - 32) & 7
                sa, sb, sc = G.gate3_coefs(name, mask)
                want_rots.append([a, b, sa, sb, 0, u, c, sc])               # c0 = 0, the integers of include/tfhe_hip.h
                want_key.append(keys[i])
                pos_in_level[lvl[i]] = u + 1
            else:
                c8, sa, sb = GATE_LIN[kind]
                want_rots.append([a, b, sa, sb, c8 * MU, u, -1, 0])
                want_key.append(keys[i])
                pos_in_level[lvl[i]] = u + 1
        assert P["rots"].tolist() == want_rots
        assert P["kss"][:, 3].tolist() == [ops[i][1] for i in order]
        if nkeys > 1:
            assert P["rot_key"].tolist() == want_key                         # per-key grouping within every level
            for g in range(P["levels"]):
                for k in range(nkeys):
                    sg = g * nkeys + k
                    assert set(P["rot_key"][P["rot_koff"][sg]:P["rot_koff"][sg + 1]].tolist()) <= {k}
        # the six-word entry accepts the new kinds and gives the first six words of the same rotations
        P6 = _plan(ops, keys, nkeys, "tfhe_hip_test_level_plan", 6)
        assert P6["rots"].tolist() == [r[:6] for r in want_rots]
        assert (P6["rots_raw"][6 * len(want_rots):] == -99).all()            # and not a word beyond them
    # coefficients under every mask, spelled out once
    assert G.gate3_coefs("MAJ3", 0) == [1, 1, 1] and G.gate3_coefs("XOR3", 0) == [-2, -2, -2]
    assert G.gate3_coefs("XNOR3", 0) == [2, 2, 2] and G.gate3_coefs("MAJ3", 1) == [-1, 1, 1]
    assert G.gate3_coefs("XOR3", 6) == [-2, 2, 2]


def test_old_plan_entry_unchanged_for_existing_kinds():
    """A DAG of the existing kinds through the six-word entry: the arrays restated here word for word (this is what the
    library gave before the descriptor grew), and the eight-word entry adds (-1, 0) to every rotation."""
    ops = [(2, 100, 0, 1, -1), (4, 200, 20, 21, -1), (NOT, 110, 10, -1, -1), (1, 101, 1, 2, -1), (7, 201, 200, 20, -1),
           (5, 102, 2, 3, -1), (1, 111, 110, 11, -1), (0, 103, 3, 0, -1), (4, 202, 201, 21, -1), (MUX, 104, 100, 101, 102),
           (9, 105, 104, 103, -1)]
    keys = [0, 2, 1, 0, 2, 0, 1, 0, 2, 0, 0]
    P = _plan(ops, keys, 3, "tfhe_hip_test_level_plan", 6)
    assert P["levels"] == 3 and P["lvl"].tolist() == [1, 1, 0, 1, 2, 1, 1, 1, 3, 2, 3]
    assert P["rot_off"].tolist() == [0, 6, 9, 11] and P["ks_off"].tolist() == [0, 6, 8, 10]
    assert P["rots"].tolist() == [
        [0, 1, 1, 1, -MU, 0], [1, 2, 1, 1, MU, 1], [2, 3, -2, -2, -2 * MU, 2], [3, 0, -1, -1, MU, 3],
        [110, 11, 1, 1, MU, 4], [20, 21, 2, 2, 2 * MU, 5],
        [100, 101, 1, 1, -MU, 0], [100, 102, -1, 1, -MU, 1], [200, 20, 1, -1, -MU, 2],
        [104, 103, 1, -1, MU, 0], [201, 21, 2, 2, 2 * MU, 1]]
    assert P["kss"].tolist() == [[0, -1, 0, 100], [1, -1, 0, 101], [2, -1, 0, 102], [3, -1, 0, 103], [4, -1, 0, 111],
                                 [5, -1, 0, 200], [0, 1, MU, 104], [2, -1, 0, 201], [0, -1, 0, 105], [1, -1, 0, 202]]
    assert P["rot_key"].tolist() == [0, 0, 0, 0, 1, 2, 0, 0, 2, 0, 2]
    assert P["rot_koff"].tolist() == [0, 4, 5, 6, 8, 8, 9, 10, 10, 11]
    assert P["ks_koff"].tolist() == [0, 4, 5, 6, 7, 7, 8, 9, 9, 10]
    P8 = _plan(ops, keys, 3, "tfhe_hip_test_level_plan3", 8)
    assert P8["rots"].tolist() == [r + [-1, 0] for r in P["rots"].tolist()]
    for name in ("lvl", "rot_off", "ks_off", "rot_koff", "ks_koff", "rot_key", "kss"):
        assert P8[name].tolist() == P[name].tolist()


def test_unknown_kind_is_refused():
    from peba1_amd import lib
    L = lib.load()
    for kind in (10, 18, 31, 56):
        flat = np.array([(kind, 10, 0, 1, 2)], dtype=np.int32).reshape(-1)
        lv = np.zeros(1, dtype=np.int32)
        L.tfhe_hip_clear_error()
        assert L.tfhe_hip_test_schedule(flat.ctypes.data_as(lib.I32P), 1, 256, 0, lv.ctypes.data_as(lib.I32P)) == -1
        assert b"unknown op kind" in L.tfhe_hip_last_error()


# ---- circuits over the plaintext provider: the fallback to two-input gates -----------------------------------------------
PLAIN_WORKER = r'''
import ctypes as C, os, random
t = os.environ["PEBA1_TMP"]
gate = C.CDLL(t + "/libplain_tfhe.so", mode=C.RTLD_GLOBAL)
circ = C.CDLL(t + "/libcircuits_test.so")
V = C.c_void_p
gate.new_default_gate_bootstrapping_parameters.restype = V
gate.new_random_gate_bootstrapping_secret_keyset.restype = V
gate.new_random_gate_bootstrapping_secret_keyset.argtypes = [V]
gate.new_gate_bootstrapping_ciphertext_array.restype = V
gate.new_gate_bootstrapping_ciphertext_array.argtypes = [C.c_int32, V]
gate.bootsSymEncrypt.argtypes = [V, C.c_int32, V]
gate.bootsSymDecrypt.argtypes = [V, V]
gate.mock_bootstraps.restype = C.c_int64
params = gate.new_default_gate_bootstrapping_parameters(128)
key = gate.new_random_gate_bootstrapping_secret_keyset(params)
cloud = key + 24
SZ = 24
def enc(v, bits):
    p = gate.new_gate_bootstrapping_ciphertext_array(bits, params)
    for i in range(bits):
        gate.bootsSymEncrypt(p + i * SZ, (v >> i) & 1, key)
    return p
def dec(p, bits):
    return sum(gate.bootsSymDecrypt(p + i * SZ, key) << i for i in range(bits))
def arr(n):
    return gate.new_gate_bootstrapping_ciphertext_array(n, params)
circ.peba1_hamming_count_bits.restype = C.c_int
circ.peba1_hamming_distance_csa.argtypes = [V, V, V, C.c_int, V]
circ.peba1_hamming_match_csa.argtypes = [V, V, V, C.c_int, V, V]
circ.peba1_hamming_match.argtypes = [V, V, V, C.c_int, V, V]
rnd = random.Random(31)
def with_distance(a, nbits, d):
    m = 0
    for i in rnd.sample(range(nbits), d):
        m |= 1 << i
    return a ^ m
checked = 0
for nbits in (16, 128):
    w = circ.peba1_hamming_count_bits(nbits)
    pairs = []
    for _ in range(50):
        pairs.append((rnd.getrandbits(nbits), rnd.getrandbits(nbits), rnd.randrange(nbits + 1)))
    a = rnd.getrandbits(nbits)
    bound = nbits // 3
    pairs += [(a, a, 0), (a, a, bound), (a, a ^ ((1 << nbits) - 1), bound), (a, a ^ ((1 << nbits) - 1), nbits),
              (a, with_distance(a, nbits, bound), bound), (a, with_distance(a, nbits, bound + 1), bound),
              (a, with_distance(a, nbits, bound - 1), bound)]
    for a, b, bound in pairs:
        hd = bin(a ^ b).count("1")
        ca, cb, cnt, rb = enc(a, nbits), enc(b, nbits), arr(w), arr(w)
        circ.peba1_hamming_distance_csa(cnt, ca, cb, nbits, cloud)
        assert dec(cnt, w) == hd, (nbits, a, b, dec(cnt, w), hd)
        circ.peba1_hamming_match_csa(rb, ca, cb, nbits, enc(bound, w), cloud)
        assert dec(rb, w) == (1 if hd > bound else 0), (nbits, a, b, bound)
        checked += 1
a, b = rnd.getrandbits(128), rnd.getrandbits(128)
gate.mock_reset()
circ.peba1_hamming_match(arr(8), enc(a, 128), enc(b, 128), 128, enc(40, 8), cloud)
print("hamming_match128 bootstraps", gate.mock_bootstraps())
gate.mock_reset()
circ.peba1_hamming_match_csa(arr(8), enc(a, 128), enc(b, 128), 128, enc(40, 8), cloud)
print("hamming_match_csa128 fallback bootstraps", gate.mock_bootstraps())

circ.peba1_function_f_fast3.argtypes = [V, V, V, C.c_int, V, C.c_int, V]
circ.peba1_function_f_fast.argtypes = [V, V, V, C.c_int, V, C.c_int, V]
def vec(vals, bits):
    return (V * len(vals))(*[enc(v, bits) for v in vals])
cases = [([0] * 3, [0] * 3), ([255] * 3, [0] * 3), ([0] * 3, [255] * 3), ([7, 200, 13], [7, 200, 13])]
for _ in range(50):
    cases.append(([rnd.randrange(256) for _ in range(3)], [rnd.randrange(256) for _ in range(3)]))
for probe, tmpl in cases:
    d = sum((x - y) ** 2 for x, y in zip(probe, tmpl))
    for bound in sorted({0, max(d - 1, 0), d, d + 1}):
        rb = arr(24)
        circ.peba1_function_f_fast3(rb, vec(probe, 8), vec(tmpl, 8), 3, enc(bound, 24), 8, cloud)
        assert dec(rb, 24) == (1 if d > bound else 0), (probe, tmpl, bound)
        checked += 1
# over this provider the new entry issues peba1_function_f_fast's own gate sequence
gate.mock_trace_hash.restype = C.c_uint64
hashes = []
for f in (circ.peba1_function_f_fast, circ.peba1_function_f_fast3):
    S, T, B, rb = vec([40, 190, 3], 8), vec([37, 200, 250], 8), enc(100, 24), arr(24)
    gate.mock_reset()
    f(rb, S, T, 3, B, 8, cloud)
    hashes.append((gate.mock_bootstraps(), gate.mock_trace_hash()))
assert hashes[0][0] == hashes[1][0], hashes
print("checked", checked)
print("OK")
'''


@pytest.fixture(scope="module")
def plain_out(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("gate3_plain"))
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=gnu++11", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "tests/mock/plain_tfhe.cpp"), "-o", t + "/libplain_tfhe.so"])
    subprocess.check_call(["g++", "-O1", "-std=gnu++17", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "peba1_amd/csrc/circuits.cpp"),
                           os.path.join(ROOT, "peba1_amd/csrc/circuits_fast.cpp"), "-o", t + "/libcircuits_test.so"])
    with open(t + "/worker.py", "w") as f:
        f.write(PLAIN_WORKER)
    out = subprocess.run([sys.executable, t + "/worker.py"], env=dict(os.environ, PEBA1_TMP=t), capture_output=True,
                         text=True, timeout=500)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_circuits_over_plain_provider_fallback(plain_out):
    assert "OK" in plain_out
    print(plain_out)


# ---- circuits over the netlist provider: the three-input gates themselves ------------------------------------------------
@pytest.fixture(scope="module")
def netlists(tmp_path_factory):
    return G.build_netlist_provider(str(tmp_path_factory.mktemp("gate3_netlist")))


def test_netlists_evaluate_to_the_plaintext_rule(netlists):
    """The DAGs WITH the three-input gates on plaintext bits (the gates by their truth tables): the recorded netlist is a
    fixed function of its inputs, so one recording serves every input."""
    rnd = random.Random(9)
    for nbits in (16, 128):
        w = nbits.bit_length()
        rows, out = G.record_netlist(netlists, **G.hamming_job("hamming_match_csa", 0, 0, 0, nbits))
        assert any(r[0] >= G.OP_GATE3 and r[0] < G.OP_INPUT for r in rows)
        bound = nbits // 3
        cases = [(rnd.getrandbits(nbits), rnd.getrandbits(nbits), rnd.randrange(nbits + 1)) for _ in range(50)]
        a = rnd.getrandbits(nbits)
        full = (1 << nbits) - 1
        flip = lambda d: a ^ sum(1 << i for i in rnd.sample(range(nbits), d))
        cases += [(a, a, 0), (a, a ^ full, nbits), (a, a ^ full, bound), (a, flip(bound), bound),
                  (a, flip(bound + 1), bound), (a, flip(bound - 1), bound)]
        for a_, b_, bd in cases:
            bits = [(a_ >> i) & 1 for i in range(nbits)] + [(b_ >> i) & 1 for i in range(nbits)] + \
                   [(bd >> i) & 1 for i in range(w)]
            val = G.eval_plain(rows, bits)
            assert [val[o] for o in out] == [1 if bin(a_ ^ b_).count("1") > bd else 0] + [0] * (w - 1), (nbits, a_, b_, bd)
    rows, out = G.record_netlist(netlists, **G.function_f_job("function_f_fast3", [0] * 3, [0] * 3, 0, 8))
    assert any(r[0] == G.OP_GATE3 and r[1] == 1 for r in rows)               # the borrow chain: MAJ3 with a negated
    for _ in range(60):
        probe, tmpl = [rnd.randrange(256) for _ in range(3)], [rnd.randrange(256) for _ in range(3)]
        d = sum((x - y) ** 2 for x, y in zip(probe, tmpl))
        for bd in (max(d - 1, 0), d, d + 1):
            bits = [(v >> i) & 1 for v in probe + tmpl for i in range(8)] + [(bd >> i) & 1 for i in range(24)]
            val = G.eval_plain(rows, bits)
            assert val[out[0]] == (1 if d > bd else 0), (probe, tmpl, bd)


def test_circuits_word_for_word_through_the_oracle(netlists, oracle):
    """16-bit Hamming match and 2-slot function_f_fast3, every gate through the oracle (the three-input ones as its
    bootstrap and key switch of the stated linear combination): decrypted results, and the SHA-256 of the output words
    that tests/test_gpu_gate3.py must reproduce on the device."""
    oks = oracle.KeySet(oracle.params("P128"), G.KEY_SEED)
    digests = G.load_digests()
    h = G.HAMMING16
    rows, out = G.record_netlist(netlists, **G.hamming_job("hamming_match_csa", h["a"], h["b"], h["bound"], h["nbits"]))
    w = G.replay_oracle(oks, rows, oracle.Rng(G.ENC_SEED))
    assert oks.decrypt(np.stack([w[o] for o in out])).tolist() == [1, 0, 0, 0, 0]    # distance 7 > 6
    for wire, bit in G.eval_plain(rows, None).items():                       # every wire decrypts to its plaintext value
        assert oks.decrypt(w[wire])[0] == bit, wire
    assert G.sha256_words(np.stack([w[o] for o in out])) == digests["hamming_match_csa_16"]["sha256"]
    f = G.FF3_2
    rows, out = G.record_netlist(netlists, **G.function_f_job("function_f_fast3", f["probe"], f["template"], f["bound"],
                                                              f["bitsize"]))
    w = G.replay_oracle(oks, rows, oracle.Rng(G.ENC_SEED))
    assert oks.decrypt(np.stack([w[o] for o in out])).tolist() == [1] + [0] * 23     # 109 > 100
    assert G.sha256_words(np.stack([w[o] for o in out])) == digests["function_f_fast3_2"]["sha256"]
    oks.close()


def test_counts_and_depth(netlists, plain_out):
    """128-bit match: bootstraps = 128 XOR + 2 per full adder (1 in the top column) + 2 per half adder (1 in the top column)
    + the comparator, exactly as the compressor model says; at most a third of peba1_hamming_match's, and shallower."""
    rows, _ = G.record_netlist(netlists, **G.hamming_job("hamming_match_csa", 1, 2, 3, 128))
    boots, depth = G.netlist_cost(rows)
    fa, fa_top, ha, ha_top, count_depths = G.csa_model(128, 8)
    cmp_boots, cmp_depth = G.comparator_model(count_depths)
    assert boots == 128 + 2 * (fa + ha) + fa_top + ha_top + cmp_boots
    assert depth == cmp_depth
    gate3 = sum(1 for r in rows if G.OP_GATE3 <= r[0] < G.OP_INPUT)
    assert gate3 == 2 * fa + fa_top
    rows_ref, _ = G.record_netlist(netlists, **G.hamming_job("hamming_match", 1, 2, 3, 128))
    boots_ref, depth_ref = G.netlist_cost(rows_ref)
    mock_ref = int(plain_out.split("hamming_match128 bootstraps")[1].split()[0])
    assert mock_ref == boots_ref                                              # the plaintext provider counts the same
    print("hamming_match_csa 128: %d bootstraps, depth %d; hamming_match: %d, depth %d" % (boots, depth, boots_ref, depth_ref))
    assert 3 * boots <= mock_ref
    assert depth < 37 and depth < depth_ref
    rows3, _ = G.record_netlist(netlists, **G.function_f_job("function_f_fast3", [1] * 128, [2] * 128, 3, 8))
    rows2, _ = G.record_netlist(netlists, **G.function_f_job("function_f_fast", [1] * 128, [2] * 128, 3, 8))
    b3, d3 = G.netlist_cost(rows3)
    b2, d2 = G.netlist_cost(rows2)
    print("function_f_fast3 128 slots: %d bootstraps, depth %d; function_f_fast: %d, depth %d" % (b3, d3, b2, d2))
    assert b3 < b2 and d3 < d2
