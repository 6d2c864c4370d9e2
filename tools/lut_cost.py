#!/usr/bin/env python3
"""What a LUT bootstrap costs against a gate (profiles/lut_bootstrap.txt): 4,096 independent LUT bootstraps of a random
test polynomial against 4,096 independent two-input gates, variants alternating on one box, blind rotation and key switch
timed separately (kernel timing on) with the shader clock of the timed launches; then a single LUT bootstrap against a
single gate (the 8-wave form).  Usage: python tools/lut_cost.py [--rounds 3]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peba1_amd import api, lib  # noqa: E402


def timed(run):
    api.reset_stats()
    run()
    api.flush()
    s = api.stats()
    ghz = 0.1 * s["clk_shader_cycles"] / s["clk_ref_ticks"] if s["clk_ref_ticks"] else float("nan")
    return s["ms_blind_rotate"], s["ms_keyswitch"], ghz, s["lut_rotations"], s["br_wave8_launches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=4096)
    args = ap.parse_args()
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 7, device=True)
    L.tfhe_hip_set_encrypt_seed(1)
    L.tfhe_hip_set_kernel_timing(1)
    api.set_deferred(True)
    W = args.width
    rng = np.random.default_rng(0)
    a = api.CiphertextArray(pp, W).encrypt(rng.integers(0, 2, W), ks)
    b = api.CiphertextArray(pp, W).encrypt(rng.integers(0, 2, W), ks)
    r = api.CiphertextArray(pp, W)
    lut = api.Lut(pp, rng.integers(-2 ** 31, 2 ** 31, pp.N, dtype=np.int64).astype(np.int32))
    gate = lambda: api.gate_batch("AND", r, a, b, ks)
    look = lambda: api.lut_bootstrap_batch(lut, r, [a, b], [1, 1], -(1 << 29), ks)
    timed(gate), timed(look)                                  # warm-up
    rows = {"gate": [], "lut": []}
    for _ in range(args.rounds):
        rows["gate"].append(timed(gate))
        rows["lut"].append(timed(look))
    for name, rs in rows.items():
        for br, ksw, ghz, nl, _ in rs:
            print(f"{W} x {name:4s}: blind rotate {br:8.3f} ms  key switch {ksw:7.3f} ms  at {ghz:.3f} GHz  "
                  f"({br * ghz:8.2f} / {ksw * ghz:7.2f} ms GHz; lut_rotations {nl})")
    g = np.array([(x[0] * x[2], x[1] * x[2]) for x in rows["gate"]])
    t = np.array([(x[0] * x[2], x[1] * x[2]) for x in rows["lut"]])
    print(f"ratio lut / gate of the medians, clock-normalised: blind rotate {np.median(t[:, 0]) / np.median(g[:, 0]):.4f}  "
          f"key switch {np.median(t[:, 1]) / np.median(g[:, 1]):.4f};  run-to-run spread of the gate rows: blind rotate "
          f"{(g[:, 0].max() - g[:, 0].min()) / np.median(g[:, 0]):.4f}  key switch {(g[:, 1].max() - g[:, 1].min()) / np.median(g[:, 1]):.4f}")
    r1 = api.CiphertextArray(pp, 1)
    one_gate = lambda: L.bootsAND(r1.at(0), a.at(0), b.at(0), ks.cloud)
    one_lut = lambda: api.lut_bootstrap(lut, r1.at(0), [a.at(0), b.at(0)], [1, 1], -(1 << 29), ks)
    for _ in range(args.rounds):
        for name, f in (("gate", one_gate), ("lut", one_lut)):
            br, ksw, ghz, nl, w8 = timed(f)
            print(f"1 x {name:4s}: blind rotate {br:7.4f} ms  key switch {ksw:7.4f} ms  at {ghz:.3f} GHz  (8-wave launches {w8})")
    ks.close()


if __name__ == "__main__":
    main()
