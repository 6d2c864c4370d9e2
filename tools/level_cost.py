#!/usr/bin/env python3
"""Measured cost of one level of a flush, by width: profiles/level_cost_P128.json.

A level of w independent gates is what the leveller buys: one blind-rotate launch in the form plan_br picks for w
rotations (8-wave up to one workgroup per CU, 4-wave beyond, its last half-filled round as an 8-wave tail) and the key
switch of w gates.  This script runs such a level for every width of a grid -- 1, every multiple of 64 up to 2,048, and
finer steps around the multiples of the CU count, where the launch form changes -- in immediate mode (one level per
call, the idiom of benchkit.extras.independent_gates_sweep) and keeps the best of `--repeats` timed runs from the
stream events (ms_blind_rotate + ms_keyswitch).  One process, one device.  The table carries the CU count, the tunings
it was measured under, the hash of the kernels and the shader clock; scheduler.cpp reads a compiled-in copy
(tools/level_cost_inc.py writes it at build time) through launch_plan.hpp level_cost_us.

    python tools/level_cost.py [--out profiles/level_cost_P128.json] [--repeats 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def width_grid(cus, top=2048):
    ws = {1, 2, 8, 32} | set(range(64, top + 1, 64))
    for edge in range(cus, top + 1, cus):                   # the launch form changes at multiples of the CU count
        ws |= {edge - 32, edge - 16, edge - 1, edge, edge + 1, edge + 16, edge + 32}
    return sorted(w for w in ws if 1 <= w <= top)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_cost_P128.json"))
    ap.add_argument("--repeats", type=int, default=5)
    # the library's defaults; other values measure a table for those tunings (the threshold sweep of the matrix key switch)
    ap.add_argument("--ks-matrix", type=int, default=1)
    ap.add_argument("--ks-matrix-min", type=int, default=512)
    ap.add_argument("--widths", type=int, nargs="*", help="these widths only (a sweep; not a table for the build)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from peba1_amd import api, lib
    from peba1_amd.kernel_id import kernels_sha16

    L = lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L.tfhe_hip_set_kernel_timing(1)
    api.set_tuning("ks_matrix", args.ks_matrix)
    api.set_tuning("ks_matrix_min", args.ks_matrix_min)
    was = api.get_deferred()
    api.set_deferred(False)
    pq = api.ParameterSet(128)
    kq = api.SecretKeySet(pq, 0x5EBA2)
    rng = np.random.default_rng(13)
    widths = sorted(args.widths) if args.widths else width_grid(cus)
    G = max(widths)
    xa, xb = rng.integers(0, 2, G), rng.integers(0, 2, G)
    wa = api.CiphertextArray(pq, G).encrypt(xa, kq).words()
    wb = api.CiphertextArray(pq, G).encrypt(xb, kq).words()
    rows, cycles, ticks = [], 0, 0
    for w in widths:
        a = api.CiphertextArray(pq, w).set_words(wa[:w])
        b = api.CiphertextArray(pq, w).set_words(wb[:w])
        r = api.CiphertextArray(pq, w)
        api.gate_batch("AND", r, a, b, kq)                  # warm
        best = None
        for _ in range(args.repeats):
            api.reset_stats()
            api.gate_batch("AND", r, a, b, kq)
            s = api.stats()
            cycles += s["clk_shader_cycles"]
            ticks += s["clk_ref_ticks"]
            t = (s["ms_blind_rotate"] + s["ms_keyswitch"], s["ms_blind_rotate"], s["ms_keyswitch"], s["br_launches"], s["br8_launches"])
            if best is None or t[0] < best[0]:
                best = t
        assert list(r.decrypt(kq)[:8]) == [int(x & y) for x, y in zip(xa[:min(w, 8)], xb[:min(w, 8)])]
        rows.append({"width": w, "us": round(best[0] * 1e3, 1), "us_blind_rotate": round(best[1] * 1e3, 1),
                     "us_keyswitch": round(best[2] * 1e3, 1), "br_launches": best[3], "br8_launches": best[4]})
        print(f"{w:5d}  {best[0] * 1e3:9.1f} us  (rotate {best[1] * 1e3:8.1f}, key switch {best[2] * 1e3:7.1f})  launches {best[3]} of which 8-wave {best[4]}",
              flush=True)
        del a, b, r
    api.set_deferred(was)
    kq.close()
    table = {
        "what": "us of one level of `width` independent gates: blind-rotate launches as plan_br forms them plus the key switch",
        "set": "P128",
        "params": {"n": pq.n, "N": pq.N, "k": pq.k, "l": pq.l, "Bgbit": pq.Bgbit, "ks_t": pq.ks_t,
                   "ks_basebit": pq.ks_basebit},
        "cus": cus,
        "tunings": {"br_variant": -1, "br8_max_rotations": 1 << 30, "br_tail8": 1, "br_digit_table": 1, "ks_tile": 16,
                    "ks_index": 1, "ks_max_splits": 48, "ks_target_blocks": 32768, "ks_split_ties": 0,
                    "ks_matrix": args.ks_matrix, "ks_matrix_min": args.ks_matrix_min},
        "kernels_sha16": kernels_sha16(),
        "shader_clock_ghz": round(0.1 * cycles / ticks, 3) if ticks else None,
        "repeats": args.repeats,
        "levels": rows,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
