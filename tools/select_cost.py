#!/usr/bin/env python3
"""What a private selection costs at P128 (profiles/ring_select.txt).  Steps on the GPU, each in a child process under a
time limit of its own; after the first child that ends at its limit or with a non-zero exit code nothing more is started
on the card and the remaining steps are reported as NOT MEASURED.  The report goes between the two marker lines of the
output file; whatever else that file holds (the commentary) is kept.

  1. tfhe_hip_last_select_ms (the time between two stream events around the tree's launches) of a device-form select of
     M = 1,024 resident ring samples under 10 selector bits, median of three after three warm-up calls.  Beside it: the
     blind-rotate launch of one 1,024-gate level from the statistics with kernel timing on, and the counted estimate --
     per CMUX the image rows read, the transforms and the multiply-accumulates, times 1,023, priced as blind-rotate
     steps of that launch (a CMUX is the arithmetic of one step: (k+1) l forward transforms, (k+1) inverse ones per prime).
  2. With --parent DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 20 --warmup 5 of the parent and
     of this tree, alternating, --pairs times: gates/s per GHz of shader clock, every run.

    python tools/select_cost.py [--parent DIR] [--pairs 3] [--out profiles/ring_select.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN = "---- report of tools/select_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/select_cost.py: end ----"
M, BITS = 1024, 10


def measure():
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, (M, N))
    index = 677
    gallery = rng.integers(-2 ** 31, 2 ** 31, (M, 2 * N), dtype=np.int64).astype(np.int32)     # the time does not depend on the words
    gallery[index] = api.ring_encrypt_bits(bits[index], ks, seed=5)
    sel = api.Selector(pp, api.tgsw_encrypt_bits([(index >> j) & 1 for j in range(BITS)], ks, seed=6))
    dev = torch.from_numpy(gallery.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    L.tfhe_hip_set_kernel_timing(1)
    ms = []
    for i in range(6):
        out = api.ring_select(sel, dev, device=True)
        t = api.last_select_ms()
        if i >= 3:
            ms.append(t)
    assert L.tfhe_hip_stream_sync() == 0
    ph = api.packed_phases(out.cpu().numpy(), ks).astype(np.float64) / 2.0 ** 32
    res = {"n": pp.n, "N": N, "l": pp.l, "select_ms": ms, "selected_right": bool(list(api.packed_decrypt(out.cpu().numpy(), N, ks)) == list(bits[index])),
           "phase_err": float(np.abs(ph - np.where(bits[index] == 1, 0.125, -0.125)).max())}
    one = api.Selector(pp, api.tgsw_encrypt_bits([1], ks, seed=7))
    api.ring_select(one, dev[:2 * 2 * N], device=True)
    res["one_cmux_ms"] = api.last_select_ms()
    a, b, g = api.CiphertextArray(pp, N).encrypt(bits[0], ks), api.CiphertextArray(pp, N).encrypt(bits[1], ks), api.CiphertextArray(pp, N)
    api.flush()
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b.ptr, N, ks.cloud) == 0
    api.flush()
    st = api.stats()
    res["level_blind_rotate_1024"] = st["ms_blind_rotate"]
    res["level_ghz"] = st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else None
    print(json.dumps(res))


def child(cmd, limit, cwd=ROOT):
    """the last JSON line a command printed, or the reason there is none"""
    try:
        p = subprocess.run(cmd, cwd=cwd, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return None, "ended at its time limit of %d s" % limit
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        return None, "exit code %d: %s" % (p.returncode, p.stderr.strip().splitlines()[-1:] or "no output")
    return json.loads(lines[-1]), None


def per_ghz(res):
    """(gates/s, shader GHz, gates/s per GHz) of a bench.py result line"""
    def find(d, key):
        if isinstance(d, dict):
            if key in d and isinstance(d[key], (int, float)):
                return d[key]
            for v in d.values():
                got = find(v, key)
                if got is not None:
                    return got
        return None
    gates, ghz = res.get("value"), find(res, "shader_clock_ghz")
    return gates, ghz, find(res, "gates_per_s_per_shader_ghz") or (gates / ghz if gates and ghz else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-select", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_select.txt"))
    args = ap.parse_args()
    if args.step == "select":
        measure()
        return 0
    lines = ["tools/select_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    if not args.skip_select:
        m, why = child([sys.executable, os.path.abspath(__file__), "--step", "select"], 240)
        if m is None:
            stopped = "the select step: " + why
            lines.append("1. select at P128: NOT MEASURED (%s)" % why)
        else:
            N, l, n = m["N"], m["l"], m["n"]
            rows, fwd, inv, macs = 2 * l * 2 * 2 * N * 4, 2 * l * 2, 2 * 2, 2 * l * 2 * N * 2
            per_step = m["level_blind_rotate_1024"] / 1024 / n
            lines += [
                "1. P128 (N = %d, l = %d), select of M = %d resident ring samples under %d bits, device form, ms" % (N, l, M, BITS),
                "   tfhe_hip_last_select_ms, three calls after three warm-up calls: %s; median %.4f"
                % (", ".join("%.4f" % v for v in m["select_ms"]), float(np.median(m["select_ms"]))),
                "   the selected sample decrypts to entry 677: %s; largest |phase error| %.3e" % (m["selected_right"], m["phase_err"]),
                "   one CMUX alone (M = 2, one launch of one workgroup): %.4f" % m["one_cmux_ms"],
                "   blind-rotate launch of one 1,024-gate level, kernel timing: %.4f%s"
                % (m["level_blind_rotate_1024"], "  (shader clock %.3f GHz)" % m["level_ghz"] if m["level_ghz"] else ""),
                "   counted, per CMUX: %d bytes of image rows read (shared by the CMUXes of a level), %d bytes of operands read, %d written;"
                % (rows, 2 * 2 * N * 4, 2 * N * 4),
                "     %d forward and %d inverse transforms of N points, %d 64-bit multiply-accumulates; times %d CMUXes in %d launches"
                % (fwd, inv, macs, M - 1, BITS),
                "   counted estimate: a CMUX is the arithmetic of one blind-rotate step; that launch runs 1,024 x %d steps, %.3e ms a step"
                % (n, per_step),
                "     with the chip full: %d CMUXes = %.4f ms" % (M - 1, (M - 1) * per_step),
                "   measured select / estimate: %.1f" % (float(np.median(m["select_ms"])) / ((M - 1) * per_step)),
            ]
    lines.append("")
    bench = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = {"parent commit": [], "this tree": []}
    for pair in range(args.pairs if args.parent else 0):
        for name, cwd in (("parent commit", args.parent), ("this tree", ROOT)):
            if stopped:
                lines.append("2. bench.py, pair %d, %s: NOT MEASURED, not started (an earlier step ended badly -- %s)" % (pair + 1, name, stopped))
                continue
            res, why = child([sys.executable] + bench, 420, cwd=cwd)
            if res is None:
                stopped = "bench.py of %s: %s" % (name, why)
                lines.append("2. bench.py, pair %d, %s: NOT MEASURED (%s)" % (pair + 1, name, why))
                continue
            gates, ghz, ratio = per_ghz(res)
            runs[name].append(ratio)
            lines.append("2. bench.py --gpus 1 --steps 20 --warmup 5, pair %d, %s: %.0f gates/s at %.4f GHz = %.0f gates/s per GHz"
                         % (pair + 1, name, gates, ghz, ratio))
    if not args.parent:
        lines.append("2. bench.py against the parent commit: NOT MEASURED (no --parent checkout given)")
    elif runs["parent commit"] and runs["this tree"]:
        p, t = runs["parent commit"], runs["this tree"]
        lines.append("   per GHz, parent: median %.0f, spread %.0f .. %.0f (%.2f %%); this tree: median %.0f, spread %.0f .. %.0f; difference of the medians %+.2f %%"
                     % (np.median(p), min(p), max(p), (max(p) - min(p)) / np.median(p) * 100, np.median(t), min(t), max(t),
                        (np.median(t) - np.median(p)) / np.median(p) * 100))
    report = BEGIN + "\n" + "\n".join(lines) + "\n" + END + "\n"
    text = report
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = f.read()
        if BEGIN in old and END in old:        # the commentary around the report stays
            text = old[:old.index(BEGIN)] + report + old[old.index(END) + len(END) + 1:]
    with open(args.out, "w") as f:
        f.write(text)
    print(report)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
