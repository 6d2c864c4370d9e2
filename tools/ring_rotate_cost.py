#!/usr/bin/env python3
"""What a blind rotation of an ENCRYPTED ring sample costs at P128 beside the tuned rotation of a public test polynomial
(profiles/ring_rotate.txt).  The twin of tools/lookup_cost.py, whose child-process discipline and bench step (both from
tools/select_cost.py) it uses: every step on the GPU runs in a child under a time limit of its own, and after the first child
that ends badly nothing more is started on the card.

  1. Counts 1, 256 and 4,096.  New: tfhe_hip_ring_blind_rotate_device of `count` index samples against ONE resident table,
     tfhe_hip_last_ring_rotate_ms (two stream events around the one launch of ring_rotate_kernel).  Tuned: the same index
     samples through tfhe_hip_lut_bootstrap_batch against one public test polynomial, one level, flushed; ms_blind_rotate
     of TfheHipStats is the time between the stream events around that level's rotation launches (the raw entry
     tfhe_hip_kernel_lut_bootstrap_woks runs the same launches and has no event pair of its own).  Both in ONE alternating
     loop, three warm-up rounds, then three: the medians, their ratio, and the shader clock of the run.  No target: the ratio
     is what a reader needs to choose between a public LUT and an encrypted one.
  2. With --parent DIR: tools/select_cost.py's bench step, alternating parent and this tree.

    python tools/ring_rotate_cost.py [--parent DIR] [--pairs 3] [--out profiles/ring_rotate.txt]
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

BEGIN = "---- report of tools/ring_rotate_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/ring_rotate_cost.py: end ----"
COUNTS = (1, 256, 4096)


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
    table = rng.integers(0, 4, 8)
    mu = np.repeat((2 * table.astype(np.int64) + 1) << 28, N // 8)
    ring = api.ring_encrypt((mu - ((mu >> 31) << 32)).astype(np.int32), ks, seed=5)
    dring = torch.from_numpy(ring.reshape(-1)).to("cuda:0")
    lut = api.Lut(pp, ((2 * table[np.arange(N) * 8 // N].astype(np.int64) + 1) << 28).astype(np.int32))
    torch.cuda.synchronize()
    L.tfhe_hip_set_kernel_timing(1)
    res = {"n": pp.n, "N": N, "counts": {}}
    cycles = ticks = 0
    for count in COUNTS:
        # the time does not depend on the words: index samples of random words, imported once
        idx = api.CiphertextArray(pp, count).set_words(rng.integers(-2 ** 31, 2 ** 31, (count, pp.n + 1), dtype=np.int64).astype(np.int32))
        out = api.CiphertextArray(pp, count)
        zeros = np.zeros(count, dtype=np.int32)
        new_ms, tuned_ms = [], []
        for i in range(6):
            api.ring_blind_rotate(dring, idx, ks, count=count, ring_index=zeros, device=True)
            tn = api.last_ring_rotate_ms()
            api.reset_stats()
            api.lut_bootstrap_batch(lut, out, [idx], [1], 0, ks)
            api.flush()
            st = api.stats()
            if i >= 3:
                new_ms.append(tn)
                tuned_ms.append(st["ms_blind_rotate"])
                cycles += st["clk_shader_cycles"]
                ticks += st["clk_ref_ticks"]
        res["counts"][str(count)] = {"new_ms": new_ms, "tuned_ms": tuned_ms}
        for o in (idx, out):
            o.close()
    assert L.tfhe_hip_stream_sync() == 0
    res["ghz"] = cycles / ticks * 0.1 if ticks else None
    # one lookup through the whole new route decrypts: the figures above time the code that computes it
    one, got = api.CiphertextArray(pp, 1), api.CiphertextArray(pp, 1)
    api.encrypt_torus(one.at(0), (2 * 5 + 1) << 27, ks)
    api.ring_lut_bootstrap(ring.reshape(1, -1), one, ks, got)
    w = got.words().astype(np.int64)
    ph = int((w[0, -1] - (w[0, :-1] % 2 ** 32) @ np.asarray(ks.lwe_key(), dtype=np.int64)) % 2 ** 32)
    res["entry_5_right"] = bool(ph >> 29 == int(table[5]))
    print(json.dumps(res))


def fmt(ms):
    return "%s; median %.4f" % (", ".join("%.4f" % v for v in ms), float(np.median(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--skip-rotate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_rotate.txt"))
    args = ap.parse_args()
    if args.step == "rotate":
        measure()
        return 0
    lines = ["tools/ring_rotate_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    if not args.skip_rotate:
        m, why = child([sys.executable, os.path.abspath(__file__), "--step", "rotate"], 300)
        if m is None:
            stopped = "the rotation step: " + why
            lines.append("A. rotations at P128: NOT MEASURED (%s)" % why)
        else:
            lines += ["A. P128 (N = %d, n = %d), `count` index samples against one resident table, ms between two stream events"
                      % (m["N"], m["n"]) + (" (shader clock %.3f GHz)" % m["ghz"] if m["ghz"] else ""),
                      "   one alternating loop per count, three rounds after three warm-up rounds:"]
            for count in COUNTS:
                c = m["counts"][str(count)]
                new, tuned = float(np.median(c["new_ms"])), float(np.median(c["tuned_ms"]))
                lines += ["   count %5d  ring_rotate_kernel (encrypted table):      %s" % (count, fmt(c["new_ms"])),
                          "                tuned rotation launches (public LUT):      %s" % fmt(c["tuned_ms"]),
                          "                new / tuned, medians: %.2f; per rotation %.4f against %.4f ms"
                          % (new / tuned if tuned else float("nan"), new / count, tuned / count)]
            lines.append("   a lookup of entry 5 through tfhe_hip_ring_lut_bootstrap decrypts right: %s" % m["entry_5_right"])
    lines.append("")
    bench = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = {"parent commit": [], "this tree": []}
    for pair in range(args.pairs if args.parent else 0):
        for name, cwd in (("parent commit", args.parent), ("this tree", ROOT)):
            if stopped:
                lines.append("B. bench.py, pair %d, %s: NOT MEASURED, not started (an earlier step ended badly -- %s)" % (pair + 1, name, stopped))
                continue
            res, why = child([sys.executable] + bench, 420, cwd=cwd)
            if res is None:
                stopped = "bench.py of %s: %s" % (name, why)
                lines.append("B. bench.py, pair %d, %s: NOT MEASURED (%s)" % (pair + 1, name, why))
                continue
            gates, ghz, ratio = per_ghz(res)
            runs[name].append(ratio)
            lines.append("B. bench.py --gpus 1 --steps 20 --warmup 5, pair %d, %s: %.0f gates/s at %.4f GHz = %.0f gates/s per GHz"
                         % (pair + 1, name, gates, ghz, ratio))
    if not args.parent:
        lines.append("B. bench.py against the parent commit: NOT MEASURED (no --parent checkout given)")
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
        else:
            text = old.rstrip("\n") + "\n\n" + report
    with open(args.out, "w") as f:
        f.write(text)
    print(report)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
