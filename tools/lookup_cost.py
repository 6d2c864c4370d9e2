#!/usr/bin/env python3
"""What a packed lookup costs at P128 beside the select of the same entries (profiles/ring_lookup.txt).  The twin of
tools/select_cost.py, whose child-process discipline and bench step it uses: every step on the GPU runs in a child under a
time limit of its own, and after the first child that ends badly nothing more is started on the card.

  1. 1,024 entries of 128 bits.  Packed: 128 ring samples, 7 tree levels + 3 rotation steps (tfhe_hip_ring_lookup_device).
     Plain: the same entries as 1,024 ring samples, 10 tree levels (tfhe_hip_ring_select_device).  tfhe_hip_last_select_ms
     of both in ONE alternating loop, three warm-up rounds, then three: the medians, the gallery bytes of both, a lone
     rotation step (one sample of two entries, one launch) beside a lone CMUX (M = 2), and the shader clock of the run.
  2. With --parent DIR: tools/select_cost.py's bench step, alternating parent and this tree.

    python tools/lookup_cost.py [--parent DIR] [--pairs 3] [--out profiles/ring_lookup.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from select_cost import child, per_ghz             # noqa: E402

BEGIN = "---- report of tools/lookup_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/lookup_cost.py: end ----"
M, BITS, WIDTH, INDEX = 1024, 10, 128, 677


def measure():
    import torch
    from peba1_amd import api, identify, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    S = N // WIDTH
    rng = np.random.default_rng(1)
    entries = rng.integers(0, 2, (M, WIDTH))
    # the time does not depend on the words: random ones, but for the sample that holds the indexed entry
    packed = rng.integers(-2 ** 31, 2 ** 31, (M // S, 2 * N), dtype=np.int64).astype(np.int32)
    first = INDEX // S * S
    packed[INDEX // S] = identify.pack_gallery(entries[first:first + S], WIDTH, ks, seed=5)[0]
    plain = rng.integers(-2 ** 31, 2 ** 31, (M, 2 * N), dtype=np.int64).astype(np.int32)
    plain[INDEX] = api.ring_encrypt_bits(entries[INDEX], ks, seed=6)
    sel = api.Selector(pp, api.tgsw_encrypt_bits([(INDEX >> j) & 1 for j in range(BITS)], ks, seed=7))
    dpacked, dplain = torch.from_numpy(packed.reshape(-1)).to("cuda:0"), torch.from_numpy(plain.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    L.tfhe_hip_set_kernel_timing(1)
    lookup_ms, select_ms = [], []
    for i in range(6):
        out_l = api.ring_lookup(sel, dpacked, M, WIDTH, device=True)
        tl = api.last_select_ms()
        out_s = api.ring_select(sel, dplain, device=True)
        ts = api.last_select_ms()
        if i >= 3:
            lookup_ms.append(tl)
            select_ms.append(ts)
    assert L.tfhe_hip_stream_sync() == 0

    def looked_at(words):
        ph = api.packed_phases(words, ks).astype(np.float64)[:WIDTH] / 2.0 ** 32
        return (bool(list(api.packed_decrypt(words, WIDTH, ks)) == list(entries[INDEX])),
                float(np.abs(ph - np.where(entries[INDEX] == 1, 0.125, -0.125)).max()))
    res = {"n": pp.n, "N": N, "lookup_ms": lookup_ms, "select_ms": select_ms, "packed_bytes": int(packed.nbytes), "plain_bytes": int(plain.nbytes)}
    res["lookup_right"], res["lookup_phase_err"] = looked_at(out_l.cpu().numpy())
    res["select_right"], res["select_phase_err"] = looked_at(out_s.cpu().numpy())
    one = api.Selector(pp, api.tgsw_encrypt_bits([1], ks, seed=8))
    lone_rot, lone_cmux = [], []
    for i in range(6):
        api.ring_lookup(one, dplain[:2 * N], 2, N // 2, device=True)            # s = 1, no tree level: one rotation launch
        tr = api.last_select_ms()
        api.ring_select(one, dplain[:2 * 2 * N], device=True)                   # one tree level of one CMUX
        tc = api.last_select_ms()
        if i >= 3:
            lone_rot.append(tr)
            lone_cmux.append(tc)
    res["lone_rot_ms"], res["lone_cmux_ms"] = lone_rot, lone_cmux
    # the shader clock of this run: one 1,024-gate level with kernel timing on, as tools/select_cost.py takes it
    bits = rng.integers(0, 2, (2, N))
    a, b, g = api.CiphertextArray(pp, N).encrypt(bits[0], ks), api.CiphertextArray(pp, N).encrypt(bits[1], ks), api.CiphertextArray(pp, N)
    api.flush()
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b.ptr, N, ks.cloud) == 0
    api.flush()
    st = api.stats()
    res["ghz"] = st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else None
    print(json.dumps(res))


def fmt(ms):
    return "%s; median %.4f" % (", ".join("%.4f" % v for v in ms), float(np.median(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-lookup", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_lookup.txt"))
    args = ap.parse_args()
    if args.step == "lookup":
        measure()
        return 0
    lines = ["tools/lookup_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    if not args.skip_lookup:
        m, why = child([sys.executable, os.path.abspath(__file__), "--step", "lookup"], 240)
        if m is None:
            stopped = "the lookup step: " + why
            lines.append("1. lookup at P128: NOT MEASURED (%s)" % why)
        else:
            S = m["N"] // WIDTH
            lines += [
                "1. P128 (N = %d), %d entries of %d bits under %d selector bits, device forms, ms between two stream events"
                % (m["N"], M, WIDTH, BITS) + (" (shader clock %.3f GHz)" % m["ghz"] if m["ghz"] else ""),
                "   one alternating loop, three rounds after three warm-up rounds:",
                "   packed lookup, %d samples (%d bytes), %d tree levels + %d rotation steps: %s"
                % (M // S, m["packed_bytes"], BITS - (S.bit_length() - 1), S.bit_length() - 1, fmt(m["lookup_ms"])),
                "   plain select, %d samples (%d bytes), %d tree levels:                    %s" % (M, m["plain_bytes"], BITS, fmt(m["select_ms"])),
                "   packed / plain, medians: %.3f" % (float(np.median(m["lookup_ms"])) / float(np.median(m["select_ms"]))),
                "   entry %d decrypts right on coefficients 0 .. %d: lookup %s (largest |phase error| %.3e), select %s (%.3e)"
                % (INDEX, WIDTH - 1, m["lookup_right"], m["lookup_phase_err"], m["select_right"], m["select_phase_err"]),
                "   a lone rotation step (one launch of one workgroup): %s" % fmt(m["lone_rot_ms"]),
                "   a lone CMUX (M = 2, one launch of one workgroup):   %s" % fmt(m["lone_cmux_ms"]),
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
