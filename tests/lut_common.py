"""Shared by tests/test_lut_cpu.py, tests/test_gpu_lut.py and tests/golden/make_lut_digests.py: the LUT bootstrap
restated from its integers (include/tfhe_hip.h) with the CPU oracle's own pieces -- accumulator (0, X^-bbar v), the n
CMUX steps, sample extract, key switch -- and the fixed cases of tests/golden/lut_bootstrap_digests.json.  Everything a
case needs is derived from small numbers (seeds, coefficients, a generator for the test polynomial); the file holds
those, the constant c0 and the digests."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = os.path.join(ROOT, "tests", "golden", "lut_bootstrap_digests.json")

KEY_SEED = 7
CASES = {"P128": 24, "P80": 16, "P2048": 8}
OP_LUT = 64

# prelude coefficients by case, cycled: one, two and three operands, negative and +-2 coefficients
COEFS = [[1], [1, 1], [1, -1, 2], [-2], [2, -1], [-1, -1, -1], [2], [-1, 2], [1, 1, -2], [-1], [-2, 2], [2, 1, -1]]
MUS = [1 << 28, -(1 << 30) + 12345, 3 << 27]          # the constant polynomial at amplitudes other than 2^29


def load_digests():
    with open(DIGESTS) as f:
        return json.load(f)


def sha256_words(w):
    return hashlib.sha256(np.ascontiguousarray(w, dtype="<i4").tobytes()).hexdigest()


def wrap32(x):
    return (np.asarray(x, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def lut_words(gen, N):
    """The N words of a test polynomial from its generator: random full-range, a table of `slots` random sectors, or the
    constant polynomial."""
    if gen["kind"] == "constant":
        return np.full(N, gen["mu"], dtype=np.int32)
    rng = np.random.default_rng(gen["seed"])
    if gen["kind"] == "random":
        return rng.integers(-2 ** 31, 2 ** 31, N, dtype=np.int64).astype(np.int32)
    values = sector_values(gen)
    return values[np.arange(N) * gen["slots"] // N]


def sector_values(gen):
    return np.random.default_rng(gen["seed"]).integers(-2 ** 31, 2 ** 31, gen["slots"], dtype=np.int64).astype(np.int32)


def case_specs(pname, N):
    """The cases of one parameter set, without c0 and digests.  The first six force bbar to 0, 1, N-1, N, N+1 and 2N-1
    (the generator picks c0 for that); the others draw c0 at random."""
    specs = []
    targets = [0, 1, N - 1, N, N + 1, 2 * N - 1]
    base = {"P128": 100, "P80": 200, "P2048": 300}[pname]
    for i in range(CASES[pname]):
        coefs = COEFS[(i + base // 100) % len(COEFS)]
        kind = ("random", "sectors", "constant")[i % 3]
        gen = {"kind": kind, "seed": base + i}
        if kind == "sectors":
            gen["slots"] = (4, 8, 16, N)[(i // 3) % 4]
        if kind == "constant":
            gen = {"kind": kind, "mu": MUS[(i // 3) % len(MUS)]}
        rng = np.random.default_rng(7000 + base + i)
        specs.append({"index": i, "coefs": coefs, "lut": gen, "enc_seed": 5000 + base + i,
                      "bits": rng.integers(0, 2, len(coefs)).tolist(),
                      "force_bbar": targets[i] if i < len(targets) else None,
                      "c0": None if i < len(targets) else int(rng.integers(-2 ** 31, 2 ** 31))})
    return specs


def case_inputs(O, oks, case):
    """The input ciphertexts of a case: oracle encryptions of its bits from its own seed."""
    return oks.encrypt(O.Rng(case["enc_seed"]), case["bits"])


def linear(coefs, inputs, c0):
    """t = (0, c0) + sum coefs[i] inputs[i], wrapping mod 2^32 on all n + 1 words."""
    t = np.zeros(inputs.shape[1], dtype=np.int64)
    for s, ct in zip(coefs, inputs):
        t += s * ct.astype(np.int64)
    t[-1] += c0
    return wrap32(t)


def modswitch(x, N):
    """round(x 2N / 2^32) mod 2N of a Torus32 word, as the kernels and the oracle's orc_modswitch compute it."""
    log2n = int(N).bit_length()                       # log2(2N)
    return int(((int(x) & 0xFFFFFFFF) + (1 << (31 - log2n))) >> (32 - log2n)) & (2 * N - 1)


def c0_for_bbar(coefs, inputs, N, target):
    """The c0 that puts the body of t exactly on `target` / 2N."""
    body = int(linear(coefs, inputs, 0)[-1]) & 0xFFFFFFFF
    c0 = ((target << (32 - int(N).bit_length())) - body) & 0xFFFFFFFF
    return int(np.uint32(c0).view(np.int32))


def initial_acc(v, bbar):
    """(0, X^-bbar v): body coefficient j is v[j + bbar] for an index (mod 2N) below N, -v[index - N] otherwise."""
    N = len(v)
    idx = (np.arange(N) + bbar) % (2 * N)
    body = np.where(idx < N, v[idx % N].astype(np.int64), -v[idx % N].astype(np.int64))
    return np.concatenate([np.zeros(N, dtype=np.int32), wrap32(body)])


def oracle_lut_bootstrap(O, oks, lin, v, mode=2):
    """The oracle restatement: returns (key-switched sample, extracted sample, raw accumulator).  mode: the oracle's
    exact evaluators (1 Goldilocks NTT, 2 two-prime: the same words, sooner)."""
    N, n = oks.N, oks.n
    bara = [modswitch(x, N) for x in lin[:n]]
    acc = np.ascontiguousarray(initial_acc(np.asarray(v, dtype=np.int32), modswitch(lin[n], N)))
    for i, a in enumerate(bara):
        if a:
            O.lib().orc_cmux_rotate(oks.h, i, a, O._p(acc), mode)
    u = oks.sample_extract(acc)
    return oks.keyswitch(u), u, acc


# ---- the 2-bit message chain: 4 sectors of the half torus, message m at phase (2m+1)/16 ------------------------------
CHAIN = {"parameter_set": "P128", "messages": 16, "hops": 4, "perm_seed": 99, "enc_seed": 9100}


def centre(m):
    return (2 * int(m) + 1) << 28


def chain_perms(hops, seed=CHAIN["perm_seed"]):
    rng = np.random.default_rng(seed)
    return [rng.permutation(4).tolist() for _ in range(hops)]


def chain_lut(perm, N):
    """v[j] = centre(perm[sector of j]): re-encodes message m to perm[m] at the same centres."""
    return np.array([centre(perm[j * 4 // N]) for j in range(N)], dtype=np.int64).astype(np.int32)


def encode_messages(O, oks, msgs, seed):
    """Fresh encryptions of 2-bit messages: an oracle encryption of bit 1 (phase 1/8 + e) moved to (2m+1)/16."""
    cts = oks.encrypt(O.Rng(seed), [1] * len(msgs))
    for ct, m in zip(cts, msgs):
        ct[-1] = wrap32(int(ct[-1]) + centre(m) - (1 << 29))
    return cts


def phases(words, key_bits):
    """(b - <a, s>) / 2^32 in [0, 1)."""
    w = np.atleast_2d(words)
    ph = (w[:, -1].astype(np.int64) - w[:, :-1].astype(np.int64) @ np.asarray(key_bits).astype(np.int64)) & 0xFFFFFFFF
    return ph.astype(np.float64) / 2.0 ** 32


def decode(ph):
    """Sector of a phase in [0, 1/2): the 2-bit message (4 and above: the phase left the half torus)."""
    return np.floor(np.asarray(ph) * 8).astype(np.int64)


def edge_distance(ph):
    """Distance of a phase from the nearest sector edge (multiples of 1/8)."""
    x = np.asarray(ph) * 8
    return np.abs(x - np.round(x)) / 8
