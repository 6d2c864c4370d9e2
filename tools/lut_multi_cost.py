#!/usr/bin/env python3
"""What a second output costs (profiles/lut_multi.txt): 4,096 two-output bootstraps (tfhe_hip_lut_bootstrap_multi, one
rotation each) against 2 x 4,096 single LUT bootstraps of the same inputs that compute the same two functions, variants
alternating on one box, blind rotation and key switch timed separately (kernel timing on) with the shader clock of the
timed launches.  Usage: python tools/lut_multi_cost.py [--rounds 3]"""
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
    return s["ms_blind_rotate"], s["ms_keyswitch"], ghz, s["blind_rotates"], s["keyswitches"], s["multi_rotations"]


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
    lo, hi = api.CiphertextArray(pp, W), api.CiphertextArray(pp, W)
    # both bits of a 2-bit message: one rotation with two outputs, or one 4-sector table per bit
    mu = 1 << 29
    multi = api.LutMulti.from_tables(pp, mu, [[-1, 1, -1, 1], [-1, -1, 1, 1]])
    lut_lo = api.Lut.from_table(pp, np.array([-mu, mu, -mu, mu], dtype=np.int32))
    lut_hi = api.Lut.from_table(pp, np.array([-mu, -mu, mu, mu], dtype=np.int32))

    def two_singles():
        api.lut_bootstrap_batch(lut_lo, lo, [a], [1], 0, ks)
        api.lut_bootstrap_batch(lut_hi, hi, [a], [1], 0, ks)

    one_multi = lambda: api.lut_bootstrap_multi_batch(multi, [lo, hi], [a], [1], 0, ks)
    timed(two_singles), timed(one_multi)                       # warm-up
    rows = {"2 x single": [], "1 x multi ": []}
    for _ in range(args.rounds):
        rows["2 x single"].append(timed(two_singles))
        rows["1 x multi "].append(timed(one_multi))
    for name, rs in rows.items():
        for br, ksw, ghz, nrot, nks, nm in rs:
            print(f"{W} inputs, {name}: blind rotate {br:8.3f} ms  key switch {ksw:7.3f} ms  at {ghz:.3f} GHz  "
                  f"({br * ghz:8.2f} / {ksw * ghz:7.2f} ms GHz; rotations {nrot}, key switches {nks}, multi_rotations {nm})")
    g = np.array([(x[0] * x[2], x[1] * x[2]) for x in rows["2 x single"]])
    t = np.array([(x[0] * x[2], x[1] * x[2]) for x in rows["1 x multi "]])
    total = np.median(t.sum(axis=1)) / np.median(g.sum(axis=1))
    print(f"ratio multi / two singles of the medians, clock-normalised: blind rotate {np.median(t[:, 0]) / np.median(g[:, 0]):.4f}  "
          f"key switch {np.median(t[:, 1]) / np.median(g[:, 1]):.4f}  both {total:.4f};  run-to-run spread of the single rows: "
          f"blind rotate {(g[:, 0].max() - g[:, 0].min()) / np.median(g[:, 0]):.4f}  key switch "
          f"{(g[:, 1].max() - g[:, 1].min()) / np.median(g[:, 1]):.4f}")
    ks.close()


if __name__ == "__main__":
    main()
