#!/usr/bin/env python3
"""Multi-client throughput: K matches under K distinct cloud keys in ONE flush (tuning "batch_keys"), against the same K
matches under ONE key in one flush (the upper bound) and K sequential flushes, one per key (the path without batching).

    python tools/multikey_throughput.py [--ks 1,2,4,8,16,32] [--circuits hamming,fast,folded,reference] [--ref-max-k 8]
                                        [--out profiles/multikey_throughput.txt] [--only hamming:16:distinct]

Per (circuit, K, mode): wall ms of the flush(es), ms per match, matches per second, and the shader clock the blind-rotate
launches ran at (kernel timing on: every 61st workgroup stamps s_memtime / s_memrealtime).  Also prints the device memory
held by one key image.  `--only circuit:K:mode` runs one case and nothing else (the counter run of rocprofv3 --pmc).
Circuits: hamming = 128-bit peba1_hamming_match; fast = peba1_function_f_fast (128 slots x 8 bit); folded = the reference's
Function_f with constant folding; reference = the reference's Function_f (128 slots)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from peba1_amd import api, circuits, lib  # noqa: E402

NSLOTS, BITS, HBITS = 128, 8, 128


def key_image_mib(pp):
    """Bytes engine.cpp upload_key allocates for one key of the set: BK image [n][(k+1) l][2 primes][2][N] words, KSK
    [kN][t = 8][3 nonzero base-4 digits][ct_stride] words plus a zero row, twiddles 12 N + 2 x 6 N words."""
    ct_stride = (pp.n + 1 + 3) // 4 * 4
    bk = pp.n * 2 * pp.l * 2 * 2 * pp.N * 4
    ksk = (pp.N * 8 * 3 + 1) * ct_stride * 4
    return (bk + ksk + 24 * pp.N * 4) / 2**20


def make_inputs(pp, key, c, circuit):
    """Client c's encrypted inputs under `key` (plaintexts depend on c only)."""
    if circuit == "hamming":
        w = circuits.hamming_count_bits(HBITS)
        a = api.CiphertextArray(pp, HBITS).encrypt([(c * 7 + i * 13) % 3 == 0 for i in range(HBITS)], key)
        b = api.CiphertextArray(pp, HBITS).encrypt([(c * 5 + i * 11) % 4 == 0 for i in range(HBITS)], key)
        a.set_words(a.words()); b.set_words(b.words())
        return a, b, circuits.encrypt_number(pp, 40, w, key), w
    template = [(37 * i + 11 + c) % 255 for i in range(NSLOTS)]
    sample = [(t + 1 + (c % 3)) % 256 for t in template]
    T = circuits.EncryptedVector(pp, template, BITS, key).to_device()
    S = circuits.EncryptedVector(pp, sample, BITS, key).to_device()
    return S, T, circuits.encrypt_number(pp, 256 * (c + 1), 3 * BITS, key), 3 * BITS


def record(circuit, pp, inp, key):
    x, y, bound, w = inp
    rb = api.CiphertextArray(pp, w)
    if circuit == "hamming":
        circuits.hamming_match(rb, x, y, HBITS, bound, key)
    elif circuit == "fast":
        circuits.function_f_fast(rb, x, y, bound, BITS, key)
    else:
        circuits.function_f(rb, x, y, bound, BITS, key)
    return rb


def run_case(circuit, k, mode, pp, keys, inputs):
    """mode: distinct (K keys, one flush), one (K matches under keys[0], one flush), sequential (K flushes, K keys)."""
    api.set_tuning("fold_constants", 1 if circuit == "folded" else 0)
    api.set_tuning("batch_keys", 1 if mode == "distinct" else 0)
    api.set_deferred(True)
    api.flush()
    api.reset_stats()
    t0 = time.perf_counter()
    outs = []
    for c in range(k):
        key = keys[0] if mode == "one" else keys[c]
        outs.append(record(circuit, pp, inputs[mode == "one"][c], key))
        if mode == "sequential":
            api.flush()
    api.flush()
    wall = (time.perf_counter() - t0) * 1e3
    st = api.stats()
    api.set_tuning("batch_keys", 0)
    ghz = 0.1 * st["clk_shader_cycles"] / st["clk_ref_ticks"] if st["clk_ref_ticks"] else float("nan")
    return {"wall_ms": wall, "ms_per_match": wall / k, "matches_per_s": 1e3 * k / wall, "flushes": st["flushes"],
            "levels": st["levels"], "blind_rotates": st["blind_rotates"], "ghz": ghz, "keys": api.last_flush_keys(),
            "ms_keyswitch": st["ms_keyswitch"], "ms_blind_rotate": st["ms_blind_rotate"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--circuits", default="hamming,fast,folded,reference")
    ap.add_argument("--ref-max-k", type=int, default=8)
    ap.add_argument("--modes", default="distinct,one,sequential")
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    cases = []
    if a.only:
        c, k, m = a.only.split(":")
        cases = [(c, int(k), m)]
    else:
        for c in a.circuits.split(","):
            for k in ks:
                if c == "reference" and k > a.ref_max_k:
                    continue
                cases += [(c, k, m) for m in a.modes.split(",")]
    kmax = max(k for _, k, _ in cases)
    L = lib.load()
    L.tfhe_hip_set_kernel_timing(1)
    pp = api.ParameterSet(128)
    t = time.perf_counter()
    keys = [api.SecretKeySet(pp, 0x7000 + c, device=True) for c in range(kmax)]
    keygen_s = time.perf_counter() - t
    lines = [f"# tools/multikey_throughput.py: P128, {kmax} distinct keys made in {keygen_s:.1f} s",
             f"# device memory of one key image: {key_image_mib(pp):.1f} MiB (NTT image of BK + compact KSK + twiddles)",
             "# circuit    K  mode        wall_ms  ms/match  matches/s  flushes  levels  rotations  keys  GHz   br_ms     ks_ms"]
    out = open(a.out, "w") if a.out else None
    for line in lines:
        print(line, flush=True)
        if out:
            out.write(line + "\n")
    inputs = {}
    for circuit in dict.fromkeys(c for c, _, _ in cases):
        kc = max(k for c2, k, _ in cases if c2 == circuit)
        inputs[circuit] = ([make_inputs(pp, keys[c], c, circuit) for c in range(kc)],
                           [make_inputs(pp, keys[0], c, circuit) for c in range(kc)])
        run_case(circuit, 1, "one", pp, keys, inputs[circuit])             # warm: first flush of the circuit
    for circuit, k, mode in cases:
        r = run_case(circuit, k, mode, pp, keys, inputs[circuit])
        line = (f"{circuit:10s} {k:3d}  {mode:10s} {r['wall_ms']:9.1f} {r['ms_per_match']:9.2f} {r['matches_per_s']:10.2f} "
                f"{r['flushes']:8d} {r['levels']:7d} {r['blind_rotates']:10d} {r['keys']:5d}  {r['ghz']:.2f} "
                f"{r['ms_blind_rotate']:8.1f} {r['ms_keyswitch']:9.1f}")
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    for k in keys:
        k.close()


if __name__ == "__main__":
    main()
