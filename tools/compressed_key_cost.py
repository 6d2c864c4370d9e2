#!/usr/bin/env python3
"""What a seed-compressed cloud key costs and saves at P128 (profiles/compressed_keys.txt), in one process on one box,
the two paths alternately, `--rounds` times:

  time to a usable key   from the keyset's creation to the end of the first one-gate flush, minus a second one-gate flush:
                         the plain path (tfhe_hip_expand_cloud_key_host: masks on the CPU, the whole key uploaded) against
                         the device path (tfhe_hip_expand_cloud_key: bodies uploaded, masks made on the card)
  kernel time            the two expand kernels between two stream events (tfhe_hip_last_expand_ms, kernel timing on)
  bytes                  what travels, what is copied to the card, what the host holds per key before any tfhe_hip_key_* call

With --parent DIR (a built checkout of the commit before) it then runs bench.py of the parent and of this tree alternately,
parent first, `--rounds` times, each in a child process under a time limit of its own, and compares the headline per GHz of
shader clock with the parent's own spread, as tools/staging_ab.py does.  After a step that ends badly nothing more is
started on the card.  Writes the report to --out and prints it.

    python tools/compressed_key_cost.py [--parent DIR] [--rounds 3] [--out profiles/compressed_keys.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the counted estimate of the issue that asked for this: blocks of about a thousand VALU instructions a lane
EST_VALU_PER_BLOCK = 1000


def one_gate(api, L, pp, sk, cloud, a, b):
    r = api.CiphertextArray(pp, 1)
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], r.ptr, a.ptr, b.ptr, 1, cloud.cloud) == 0
    api.flush()
    bit = int(r.decrypt(sk)[0])
    r.close()
    return bit


def measure(rounds):
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    sk = api.SecretKeySet(pp, 0x5EBA2, device=False)
    ck = api.CompressedCloudKey.generate_seeded(sk, 7, np.arange(1, 11, dtype=np.uint32))
    api.set_deferred(True)
    L.tfhe_hip_set_kernel_timing(1)
    a, b = api.CiphertextArray(pp, 1).encrypt([1], sk), api.CiphertextArray(pp, 1).encrypt([1], sk)
    a.set_words(a.words())
    b.set_words(b.words())
    warm = ck.expand_host()                                  # the device, the pool and the scratch exist before anything is timed
    assert one_gate(api, L, pp, sk, warm, a, b) == 1
    warm.close()
    rows = []
    for rnd in range(rounds):
        for path in ("plain", "device"):
            t0 = time.perf_counter()
            cloud = ck.expand_host() if path == "plain" else ck.expand()
            t_made = time.perf_counter()
            assert one_gate(api, L, pp, sk, cloud, a, b) == 1
            t1 = time.perf_counter()
            assert one_gate(api, L, pp, sk, cloud, a, b) == 1
            t2 = time.perf_counter()
            rows.append({"round": rnd, "path": path, "create_ms": 1e3 * (t_made - t0), "first_ms": 1e3 * (t1 - t_made),
                         "second_ms": 1e3 * (t2 - t1), "usable_ms": 1e3 * ((t1 - t0) - (t2 - t1)),
                         "expand_kernels_ms": L.tfhe_hip_last_expand_ms() if path == "device" else None})
            cloud.close()
    n, N, k, l, t, base = pp.n, pp.N, pp.k, pp.l, pp.ks_t, 1 << pp.ks_basebit
    kpl, stride = (k + 1) * l, (n + 4) & ~3
    sizes = {"plain_file": 4 * (n * kpl * (k + 1) * N + k * N * t * base * (n + 1)), "compressed": ck.nbytes,
             "plain_to_card": 4 * (n * kpl * (k + 1) * N + (k * N * t * (base - 1) + 1) * stride),
             "device_to_card": ck.nbytes - 40,
             "plain_host": 4 * (n * kpl * (k + 1) * N + k * N * t * base * (n + 1)), "device_host": ck.nbytes,
             "blocks": (n * kpl * k * N + k * N * t * (base - 1) * n) // 8}
    ck.close()
    sk.close()
    return rows, sizes


def find(d, key):
    if isinstance(d, dict):
        if key in d and isinstance(d[key], (int, float)):
            return d[key]
        for v in d.values():
            got = find(v, key)
            if got is not None:
                return got
    return None


def bench(cwd, limit, say):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"]
    try:
        p = subprocess.run(cmd, cwd=cwd, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        say("   ended at its time limit of %d s: bench.py in %s" % (limit, cwd))
        return None
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        say("   exit code %d: bench.py in %s\n%s" % (p.returncode, cwd, p.stderr[-1500:]))
        return None
    res = json.loads(lines[-1])
    return {"gates_per_s": res.get("value"), "ghz": find(res, "shader_clock_ghz"), "per_ghz": find(res, "gates_per_s_per_shader_ghz")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressed_keys.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Seed-compressed cloud keys at P128: python tools/compressed_key_cost.py" + (" --parent <a built checkout of the commit before>" if args.parent else ""))
    say("=" * 100)
    rows, z = measure(args.rounds)
    say("1. Bytes (COUNTED from the parameter set: n = 630, N = 1,024, k = 1, l = 3, key switch (8, 2))")
    say("   what travels per client      plain cloud-key payload %11d    compressed %10d   (%.1f times smaller)" % (z["plain_file"], z["compressed"], z["plain_file"] / z["compressed"]))
    say("   copied to the card per key   plain path              %11d    device path %9d   (bodies; the masks never cross)" % (z["plain_to_card"], z["device_to_card"]))
    say("   held on the host per key     plain path              %11d    device path %9d   (before any tfhe_hip_key_* call)" % (z["plain_host"], z["device_host"]))
    say()
    say("2. Time to a usable key, MEASURED here, ms (wall; creation to the end of the first one-gate flush, minus a second one-gate flush)")
    for r in rows:
        say("   round %d  %-6s  create %8.2f  first gate %8.2f  second gate %6.2f  -> usable after %8.2f" % (r["round"] + 1, r["path"], r["create_ms"], r["first_ms"], r["second_ms"], r["usable_ms"]))
    med = {p: statistics.median(r["usable_ms"] for r in rows if r["path"] == p) for p in ("plain", "device")}
    say("   medians: plain %.2f ms, device %.2f ms: the device path is %s" % (med["plain"], med["device"], "FASTER by %.2f ms" % (med["plain"] - med["device"]) if med["device"] < med["plain"] else "NOT faster (by %.2f ms)" % (med["device"] - med["plain"])))
    say()
    ks = [r["expand_kernels_ms"] for r in rows if r["path"] == "device"]
    say("3. The two expand kernels between two stream events, MEASURED here, ms: " + ", ".join("%.4f" % x for x in ks))
    say("   a lane per ChaCha20 block: %d blocks.  The counted estimate beside it (NOT a measurement): %d blocks of about %d VALU" % (z["blocks"], z["blocks"], EST_VALU_PER_BLOCK))
    say("   instructions a lane = %.2e lane-instructions; on 256 CUs x 4 SIMDs x 16 lanes at 2.3 GHz that is %.3f ms of issue." % (z["blocks"] * EST_VALU_PER_BLOCK, 1e3 * z["blocks"] * EST_VALU_PER_BLOCK / (256 * 4 * 16 * 2.3e9)))
    say("   measured / estimate = %.1f" % (statistics.median(ks) / (1e3 * z["blocks"] * EST_VALU_PER_BLOCK / (256 * 4 * 16 * 2.3e9))))
    say()
    if not args.parent:
        say("4. bench.py against the parent commit: NOT MEASURED in this run (no --parent)")
    else:
        say("4. bench.py --gpus 1 --steps 5 --warmup 2, parent and change alternately, parent first, MEASURED here")
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
            verdict = ("PASS (within the parent's spread of the parent's median)" if abs(mc - mp) <= spread else
                       "outside the parent's spread, on the FASTER side" if mc > mp else
                       "FAIL (slower than the parent's median by more than its spread)")
            say("   parent median %.0f, spread (max - min) %.0f; change median %.0f; change - parent %+.0f (%+.2f %%): %s" % (mp, spread, mc, mc - mp, 100 * (mc - mp) / mp, verdict))
        else:
            say("   NOT COMPLETED: a step ended badly, nothing more was started")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
