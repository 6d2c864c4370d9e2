"""Shared by tests/test_gate3_cpu.py, tests/test_gpu_gate3.py and tests/golden/make_gate3_digests.py: the three-input
gates restated from their integers (include/tfhe_hip.h), the netlist provider's build and replay through the CPU
oracle, and the fixed inputs of the two circuit digests."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "tests", "golden", "gate3_circuit_digests.json")

# name -> (enum TfheHipGate3, coefficient s of t = s (+-A +- B +- C))
GATE3 = {"MAJ3": (0, 1), "XOR3": (1, -2), "XNOR3": (2, 2)}
GATE3_BY_CODE = {code: name for name, (code, _) in GATE3.items()}
GATE2_TT = {0: lambda a, b: 1 - (a & b), 1: lambda a, b: a | b, 2: lambda a, b: a & b, 3: lambda a, b: 1 - (a | b),
            4: lambda a, b: a ^ b, 5: lambda a, b: 1 - (a ^ b), 6: lambda a, b: (1 - a) & b, 7: lambda a, b: a & (1 - b),
            8: lambda a, b: (1 - a) | b, 9: lambda a, b: a | (1 - b)}
GATE2_NAMES = ["NAND", "OR", "AND", "NOR", "XOR", "XNOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
OP_MUX, OP_NOT, OP_GATE3, OP_INPUT, OP_CONST = 16, 17, 32, 100, 101

KEY_SEED, ENC_SEED = 0x5EBA2, 4242
# 16-bit Hamming match: distance 7 against the bound 6; 2-slot Euclidean match: (40-37)^2 + (190-200)^2 = 109 > 100
HAMMING16 = dict(a=0xB3C5, b=0xB3C5 ^ 0x1A4B, bound=6, nbits=16)
FF3_2 = dict(probe=[40, 190], template=[37, 200], bound=100, bitsize=8)


def gate3_coefs(name, mask):
    s = GATE3[name][1]
    return [-s if (mask >> i) & 1 else s for i in range(3)]


def gate3_lin(name, mask, A, B, Cw):
    """t = sa A + sb B + sc C in wrapping 32-bit arithmetic on all n + 1 words."""
    sa, sb, sc = gate3_coefs(name, mask)
    t = (sa * A.astype(np.int64) + sb * B.astype(np.int64) + sc * Cw.astype(np.int64)) & 0xFFFFFFFF
    return t.astype(np.uint32).view(np.int32)


def oracle_gate3(oks, name, mask, A, B, Cw):
    """The oracle's bootstrap (mu = 1/8) and key switch of the gate's linear combination; its two-prime evaluator (mode
    2: the same words as the other exact modes, four times sooner)."""
    from oracle import pyoracle as O
    lin = np.ascontiguousarray(gate3_lin(name, mask, A, B, Cw))
    u = np.zeros(oks.k * oks.N + 1, dtype=np.int32)
    O.lib().orc_bootstrap_woks(oks.h, O._p(lin), 1 << 29, O._p(u), 2)
    return oks.keyswitch(u)


def gate3_truth(name, mask, a, b, c):
    a, b, c = a ^ (mask & 1), b ^ ((mask >> 1) & 1), c ^ ((mask >> 2) & 1)
    if name == "MAJ3":
        return 1 if a + b + c >= 2 else 0
    return (a ^ b ^ c) if name == "XOR3" else 1 - (a ^ b ^ c)


# ---- the netlist provider (tests/mock/netlist_tfhe.cpp) ---------------------------------------------------------------
NETLIST_WORKER = r'''
import ctypes as C, json, os, sys
t = os.environ["PEBA1_TMP"]
gate = C.CDLL(t + "/libnetlist_tfhe.so", mode=C.RTLD_GLOBAL)
circ = C.CDLL(t + "/libcircuits_netlist.so")
V = C.c_void_p
gate.new_default_gate_bootstrapping_parameters.restype = V
gate.new_random_gate_bootstrapping_secret_keyset.restype = V
gate.new_random_gate_bootstrapping_secret_keyset.argtypes = [V]
gate.new_gate_bootstrapping_ciphertext_array.restype = V
gate.new_gate_bootstrapping_ciphertext_array.argtypes = [C.c_int32, V]
gate.bootsSymEncrypt.argtypes = [V, C.c_int32, V]
gate.netlist_wire.argtypes = [V]
gate.netlist_copy.argtypes = [C.POINTER(C.c_int32)]
params = gate.new_default_gate_bootstrapping_parameters(128)
key = gate.new_random_gate_bootstrapping_secret_keyset(params)
cloud = key + 24
SZ = 24
def enc(v, bits):
    p = gate.new_gate_bootstrapping_ciphertext_array(bits, params)
    for i in range(bits):
        gate.bootsSymEncrypt(p + i * SZ, (v >> i) & 1, key)
    return p
def arr(n):
    return gate.new_gate_bootstrapping_ciphertext_array(n, params)
job = json.loads(sys.argv[1])
circ.peba1_hamming_count_bits.restype = C.c_int
gate.netlist_reset()
if job["circuit"] in ("hamming_match", "hamming_match_csa"):
    n = job["nbits"]; w = circ.peba1_hamming_count_bits(n)
    a, b, bound, out = enc(job["a"], n), enc(job["b"], n), enc(job["bound"], w), arr(w)
    f = getattr(circ, "peba1_" + job["circuit"]); f.argtypes = [V, V, V, C.c_int, V, V]
    f(out, a, b, n, bound, cloud)
    nout = w
else:
    bits = job["bitsize"]
    S = (V * len(job["probe"]))(*[enc(v, bits) for v in job["probe"]])
    T = (V * len(job["template"]))(*[enc(v, bits) for v in job["template"]])
    bound, out = enc(job["bound"], 3 * bits), arr(3 * bits)
    f = getattr(circ, "peba1_" + job["circuit"]); f.argtypes = [V, V, V, C.c_int, V, C.c_int, V]
    f(out, S, T, len(job["probe"]), bound, bits, cloud)
    nout = 3 * bits
rows = (C.c_int32 * (6 * gate.netlist_rows()))()
gate.netlist_copy(rows)
print(json.dumps({"rows": list(rows), "out": [gate.netlist_wire(out + i * SZ) for i in range(nout)]}))
'''


def build_netlist_provider(tmp):
    """The netlist provider and the circuit library, linked to nothing: boots* and tfhe_hip_gate3 resolve at load time."""
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-O1", "-std=gnu++11", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "tests/mock/netlist_tfhe.cpp"), "-o", tmp + "/libnetlist_tfhe.so"])
    subprocess.check_call(["g++", "-O1", "-std=gnu++17", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "peba1_amd/csrc/circuits.cpp"),
                           os.path.join(ROOT, "peba1_amd/csrc/circuits_fast.cpp"), "-o", tmp + "/libcircuits_netlist.so"])
    with open(tmp + "/netlist_worker.py", "w") as f:
        f.write(NETLIST_WORKER)
    return tmp


def record_netlist(tmp, **job):
    """Runs the circuit over the netlist provider in a process of its own (its boots* symbols must not meet
    libtfhe-hip's); returns (rows [k][6] = op, mask, dst, a, b, c; output wires)."""
    out = subprocess.run([sys.executable, tmp + "/netlist_worker.py", json.dumps(job)], env=dict(os.environ, PEBA1_TMP=tmp),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout)
    return np.array(d["rows"], dtype=np.int64).reshape(-1, 6), d["out"]


def hamming_job(circuit, a, b, bound, nbits):
    return dict(circuit=circuit, a=a, b=b, bound=bound, nbits=nbits)


def function_f_job(circuit, probe, template, bound, bitsize):
    return dict(circuit=circuit, probe=probe, template=template, bound=bound, bitsize=bitsize)


def netlist_cost(rows):
    """(bootstraps, dependency depth in bootstrap levels) of a netlist."""
    depth, boots = {-2: 0}, 0
    for op, mask, dst, a, b, c in rows:
        if op in (OP_INPUT, OP_CONST):
            depth[dst] = 0
            continue
        d = max(depth[x] for x in (a, b, c) if x != -1)
        if op == OP_NOT:
            depth[dst] = d
            continue
        boots += 2 if op == OP_MUX else 1
        depth[dst] = d + 1
    return boots, max(depth.values())


def eval_plain(rows, input_bits):
    """The netlist on plaintext bits; input_bits replace the recorded INPUT values in order (None: keep them)."""
    val, k = {-2: 0}, 0
    for op, mask, dst, a, b, c in rows:
        if op == OP_INPUT:
            val[dst] = a if input_bits is None else input_bits[k]
            k += 1
        elif op == OP_CONST:
            val[dst] = a
        elif op == OP_NOT:
            val[dst] = 1 - val[a]
        elif op == OP_MUX:
            val[dst] = val[b] if val[a] else val[c]
        elif op >= OP_GATE3:
            val[dst] = gate3_truth(GATE3_BY_CODE[op - OP_GATE3], mask, val[a], val[b], val[c])
        else:
            val[dst] = GATE2_TT[op](val[a], val[b])
    return val


def replay_oracle(oks, rows, enc_rng):
    """Every wire's words: inputs encrypted by the oracle in recording order, two-input gates, MUX, NOT and constants
    by the oracle's own entries, the three-input gates as the oracle's bootstrap and key switch of their linear
    combination."""
    w = {-2: oks.constant(0)}
    for op, mask, dst, a, b, c in rows:
        if op == OP_INPUT:
            w[dst] = oks.encrypt(enc_rng, [a])[0]
        elif op == OP_CONST:
            w[dst] = oks.constant(a)
        elif op == OP_NOT:
            w[dst] = oks.gate_not(w[a])
        elif op == OP_MUX:
            w[dst] = oks.mux(w[a], w[b], w[c], use_ntt=2)
        elif op >= OP_GATE3:
            w[dst] = oracle_gate3(oks, GATE3_BY_CODE[op - OP_GATE3], mask, w[a], w[b], w[c])
        else:
            w[dst] = oks.gate(GATE2_NAMES[op], w[a], w[b], use_ntt=2)
    return w


def input_words(oks, enc_rng, values_and_bits):
    """The ciphertexts replay_oracle gives the circuit's inputs, for a run on the device: [(value, bits), ...] in the
    order the netlist worker encrypts them -> one [bits][n + 1] array each."""
    return [oks.encrypt(enc_rng, [(v >> i) & 1 for i in range(bits)]) for v, bits in values_and_bits]


def sha256_words(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.int32).tobytes()).hexdigest()


def csa_model(nbits, width):
    """The population-count compressor of circuits_fast.cpp restated on depths alone: (full adders with carry, full
    adders without, half adders with carry, half adders without, depth of every count wire)."""
    cols = [[] for _ in range(width)]
    cols[0] = [1] * nbits                                   # the XOR of every bit pair: depth 1
    fa = fa_top = ha = ha_top = 0
    out = []
    for w in range(width):
        c = cols[w]
        carry = w + 1 < width
        while len(c) > 1:
            c.sort()                                        # stable; equal depths keep their order, as the circuit's sort
            take = 3 if len(c) >= 3 else 2
            d = max(c[:take]) + 1
            del c[:take]
            c.append(d)
            if carry:
                cols[w + 1].append(d)
            if take == 3:
                fa, fa_top = fa + carry, fa_top + (not carry)
            else:
                ha, ha_top = ha + carry, ha_top + (not carry)
        out.append(c[0] if c else 0)
    return fa, fa_top, ha, ha_top, out


def comparator_model(depths):
    """greater_than of circuits_fast.cpp on real wires: (bootstraps, depth of the result)."""
    cur = [(d + 1, d + 1) for d in depths]                  # (gt, eq): ANDYN and XNOR per bit
    boots = 2 * len(depths)
    while len(cur) > 1:
        nxt = []
        for i in range(0, len(cur) - 1, 2):
            (lgt, leq), (hgt, heq) = cur[i], cur[i + 1]
            gt = max(hgt, max(heq, lgt) + 1) + 1            # OR(hi.gt, AND(hi.eq, lo.gt))
            boots += 2
            eq = None
            if len(cur) > 2:
                eq = max(heq, leq) + 1
                boots += 1
            nxt.append((gt, eq))
        if len(cur) & 1:
            nxt.append(cur[-1])
        cur = nxt
    return boots, cur[0][0]


def load_digests():
    with open(DIGESTS) as f:
        return json.load(f)
