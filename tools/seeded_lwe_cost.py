#!/usr/bin/env python3
"""What seed-compressed LWE sample arrays cost and save at P128 (profiles/seeded_lwe.txt), in one process on one box:

  bytes            what travels and what is copied to the card for 1,024 fresh samples, plain and as one record
  import time      the seeded import of 1,024 samples (tfhe_hip_import_samples_seeded, host record) between two stream events
                   and by the wall clock, beside tfhe_hip_import_samples of the host-expanded samples in the same
                   alternating loop, median of `--reps`; the counted estimate (bytes stored, ChaCha20 lane-operations) next to it

With --parent DIR (a built checkout of the commit before) it then runs bench.py of the parent and of this tree alternately,
parent first, `--rounds` times, each in a child process under a time limit of its own, and compares the headline per GHz of
shader clock with the parent's own spread, as tools/seeded_wire_cost.py does.  After a step that ends badly nothing more is
started on the card.  Writes the report to --out and prints it.

    python tools/seeded_lwe_cost.py [--parent DIR] [--rounds 3] [--reps 3] [--out profiles/seeded_lwe.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from compressed_key_cost import bench          # noqa: E402  (the same child-process bench run and its JSON fields)
from seeded_wire_cost import EST_VALU_PER_BLOCK, shader_ghz   # noqa: E402

COUNT = 1024


def measure(reps):
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    api.set_deferred(True)
    bits = np.random.default_rng(1).integers(0, 2, COUNT)
    rec = api.encrypt_bits_compressed(bits, ks)
    plain = api.lwe_expand(rec, pp.n)
    stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    r = api.CiphertextArray(pp, COUNT)
    ms, wall = {"plain": [], "seeded": []}, {"plain": [], "seeded": []}
    for i in range(reps + 2):                           # two rounds first: the scratch, the staging area and the code exist
        for form in ("plain", "seeded"):
            t0 = time.perf_counter()
            e0.record(stream)
            if form == "plain":
                r.set_words(plain)
            else:
                api.import_seeded(rec, pp, r)
            e1.record(stream)
            e1.synchronize()
            t1 = time.perf_counter()
            if i >= 2:
                ms[form].append(e0.elapsed_time(e1))
                wall[form].append(1e3 * (t1 - t0))
    assert list(r.decrypt(ks)) == list(bits)
    out = {"events": {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "wall": {k: float(np.median(v)) for k, v in wall.items()},
           "ghz": shader_ghz(api, L, pp, ks), "n": pp.n, "stride": (pp.n + 4) & ~3}
    r.close()
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bench-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_lwe.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Seed-compressed LWE sample arrays at P128: python tools/seeded_lwe_cost.py" + (" --parent <a built checkout of the commit before>" if args.parent else ""))
    say("=" * 100)
    m = measure(args.reps)
    n, stride = m["n"], m["stride"]
    say("1. Bytes for %d fresh samples (COUNTED from the parameter set: n = %d)" % (COUNT, n))
    say("   travels: plain samples %9d   one record %6d (seed + bodies)" % (COUNT * (n + 1) * 4, (10 + COUNT) * 4))
    say("   copied to the card: plain import %9d (words) + %d (slot list)   seeded import %d (seed, pad, bodies) + %d (index) + %d (slot list)" % (
        COUNT * (n + 1) * 4, COUNT * 4, (12 + COUNT) * 4, COUNT * 4, COUNT * 4))
    say()
    e, w = m["events"], m["wall"]
    say("2. Import of %d samples from host memory, MEASURED here, ms, median (min, max) of %d between two stream events, the two" % (COUNT, args.reps))
    say("   forms alternately in one loop after two rounds of each; shader clock of a 1,024-gate flush right after: %.4f GHz" % m["ghz"])
    say("   plain  tfhe_hip_import_samples         %.4f (%.4f, %.4f)   wall clock of the call, median %.4f" % (e["plain"][0], e["plain"][1], e["plain"][2], w["plain"]))
    say("   seeded tfhe_hip_import_samples_seeded  %.4f (%.4f, %.4f)   wall clock of the call, median %.4f" % (e["seeded"][0], e["seeded"][1], e["seeded"][2], w["seeded"]))
    say("   seeded - plain %+.4f ms, seeded / plain %.3f: the seeded import is %s the plain import" % (
        e["seeded"][0] - e["plain"][0], e["seeded"][0] / e["plain"][0], "NO SLOWER than" if e["seeded"][0] <= e["plain"][0] else "SLOWER than"))
    blocks = COUNT * ((n + 7) // 8 + 1)
    est_ms = 1e3 * blocks * EST_VALU_PER_BLOCK / (256 * 4 * 16 * m["ghz"] * 1e9)
    say("   The counted estimate beside it (NOT a measurement): one row per workgroup, at most %d blocks a row = %d blocks of about" % ((n + 7) // 8 + 1, blocks))
    say("   %d VALU operations a lane = %.2e lane-operations; on 256 CUs x 4 SIMDs x 16 lanes at that clock %.4f ms of issue;" % (EST_VALU_PER_BLOCK, blocks * EST_VALU_PER_BLOCK, est_ms))
    say("   bytes stored: %d rows of %d words = %d." % (COUNT, stride, COUNT * stride * 4))
    say()
    if not args.parent:
        say("3. bench.py against the parent commit: NOT MEASURED in this run (no --parent)")
    else:
        say("3. bench.py --gpus 1 --steps 5 --warmup 2, parent and change alternately, parent first, MEASURED here")
        runs, ok = [], True
        for rnd in range(args.rounds):
            for name, cwd in (("parent", os.path.abspath(args.parent)), ("change", ROOT)):
                res = bench(cwd, args.bench_limit, say) if ok else None
                if res is None:
                    ok = False
                    continue
                runs.append((rnd, name, res))
                say("   round %d, %s: %.0f gates/s at %.4f GHz = %.0f per GHz" % (rnd + 1, name, res["gates_per_s"], res["ghz"], res["per_ghz"]))
        p = [r["per_ghz"] for _, nme, r in runs if nme == "parent"]
        c = [r["per_ghz"] for _, nme, r in runs if nme == "change"]
        if ok and p and len(p) == len(c):
            spread, mp, mc = max(p) - min(p), statistics.median(p), statistics.median(c)
            verdict = ("inside the parent's spread of the parent's median" if abs(mc - mp) <= spread else
                       "outside the parent's spread, on the FASTER side" if mc > mp else
                       "SLOWER than the parent's median by more than its spread")
            say("   parent median %.0f, spread (max - min) %.0f; change median %.0f; change - parent %+.0f (%+.2f %%): %s" % (mp, spread, mc, mc - mp, 100 * (mc - mp) / mp, verdict))
        else:
            say("   NOT COMPLETED: a step ended badly, nothing more was started")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
