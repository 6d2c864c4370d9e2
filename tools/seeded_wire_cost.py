#!/usr/bin/env python3
"""What seed-compressed packing keys and ring samples cost and save at P128 (profiles/seeded_wire.txt), in one process on
one box:

  bytes                  what travels and what is copied to the card, packing key and a 1,024-bit input, plain and compressed
  time to a first pack   from the key object's creation on the server (from the words it received) to the end of its first
                         pack, minus a second pack: the plain key's path (raw rows uploaded) against the device-expanded
                         key's (bodies uploaded, masks made on the card), alternately, `--rounds` times
  seeded unpack          1,024 samples from one compressed record in device memory between two stream events, beside the
                         plain unpack of the expanded sample in the same loop, with the counted ChaCha20 estimate

With --parent DIR (a built checkout of the commit before) it then runs bench.py of the parent and of this tree alternately,
parent first, `--rounds` times, each in a child process under a time limit of its own, and compares the headline per GHz of
shader clock with the parent's own spread, as tools/compressed_key_cost.py does.  After a step that ends badly nothing more
is started on the card.  Writes the report to --out and prints it.

    python tools/seeded_wire_cost.py [--parent DIR] [--rounds 3] [--out profiles/seeded_wire.txt]
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

from compressed_key_cost import bench   # noqa: E402  (the same child-process bench run and its JSON fields)

EST_VALU_PER_BLOCK = 1050               # 20 rounds of 4 quarter rounds of 12 VALU operations, the feed-forward, the LDS writes


def shader_ghz(api, L, pp, ks):
    """the shader clock of a 1,024-gate flush run now (kernel timing's cycle and reference counters)"""
    bits = np.arange(1024) & 1
    a, b, g = api.CiphertextArray(pp, 1024).encrypt(bits, ks), api.CiphertextArray(pp, 1024).encrypt(1 - bits, ks), api.CiphertextArray(pp, 1024)
    api.flush()
    L.tfhe_hip_set_kernel_timing(1)
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b.ptr, 1024, ks.cloud) == 0
    api.flush()
    st = api.stats()
    L.tfhe_hip_set_kernel_timing(0)
    for o in (a, b, g):
        o.close()
    return st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else float("nan")


def measure(rounds, reps):
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    api.set_deferred(True)
    N = pp.N
    out = {}
    # ---- the packing key ----
    ck = api.CompressedPackingKey.generate_seeded(ks, 7, np.arange(1, 11, dtype=np.uint32))
    seed, body = ck.seed(), np.array(ck.body())
    host = ck.expand_host()
    rows = host.words()
    arr = api.CiphertextArray(pp, 4).encrypt([1, 0, 1, 1], ks)
    api.flush()
    want = api.pack(host, arr, 4, ks)                         # the device, the scratch and the kernels' code exist before anything is timed
    warm = ck.expand()
    assert (api.pack(warm, arr, 4, ks) == want).all()          # ... and the pinned staging area has its size
    warm.close()
    timed = []
    for rnd in range(rounds):
        for path in ("plain", "device"):
            t0 = time.perf_counter()
            if path == "plain":
                key = api.PackingKey.from_words(pp, ck.t, ck.basebit, rows)
            else:
                c2 = api.CompressedPackingKey.from_words(pp, ck.t, ck.basebit, seed, body)
                key = c2.expand()
                c2.close()
            t_made = time.perf_counter()
            got = api.pack(key, arr, 4, ks)
            t1 = time.perf_counter()
            api.pack(key, arr, 4, ks)
            t2 = time.perf_counter()
            assert (got == want).all()
            timed.append({"round": rnd, "path": path, "create_ms": 1e3 * (t_made - t0), "first_ms": 1e3 * (t1 - t_made),
                          "second_ms": 1e3 * (t2 - t1), "usable_ms": 1e3 * ((t1 - t0) - (t2 - t1))})
            key.close()
    out["pack"] = timed
    out["pack_ghz"] = shader_ghz(api, L, pp, ks)
    out["sizes"] = {"rows": rows.size * 4, "compressed": ck.nbytes, "body": body.size * 4,
                    "ring_plain": 2 * N * 4, "ring_compressed": (10 + N) * 4}
    for o in (host, ck, arr):
        o.close()
    # ---- the unpack ----
    stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bits = np.random.default_rng(1).integers(0, 2, N)
    comp = api.ring_encrypt_bits(bits, ks, compressed=True)
    plain = api.ring_expand(comp, N)[0]
    dcomp, dplain = torch.from_numpy(comp).to("cuda:0"), torch.from_numpy(plain).to("cuda:0")
    torch.cuda.synchronize()
    r = api.CiphertextArray(pp, N)
    ms = {"plain": [], "seeded": []}
    for i in range(reps + 3):
        for form in ("plain", "seeded"):
            e0.record(stream)
            if form == "plain":
                api.unpack_device(dplain.data_ptr(), 1, ks, r, count=N)
            else:
                api.unpack_seeded_device(dcomp.data_ptr(), 1, ks, r, count=N)
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                ms[form].append(e0.elapsed_time(e1))
    assert L.tfhe_hip_stream_sync() == 0
    assert list(r.decrypt(ks)) == list(bits)
    # the extract kernels alone: the raw entries' launches between events would carry their transfers, so the difference of
    # the two whole unpacks above is the figure; what the key switch behind both takes is the common part
    out["unpack"] = {k: [float(np.median(v)), float(np.min(v))] for k, v in ms.items()}
    out["unpack_ghz"] = shader_ghz(api, L, pp, ks)
    r.close()
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bench-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_wire.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Seed-compressed packing keys and ring samples at P128: python tools/seeded_wire_cost.py" + (" --parent <a built checkout of the commit before>" if args.parent else ""))
    say("=" * 100)
    m = measure(args.rounds, args.reps)
    z = m["sizes"]
    say("1. Bytes (COUNTED from the parameter set: n = 630, N = 1,024, k = 1, packing decomposition (8, 2))")
    say("   packing key     travels: raw rows %10d   compressed %10d (seed + bodies)   copied to the card: plain %10d   device-expanded %10d" % (z["rows"], z["compressed"], z["rows"], z["body"]))
    say("   1,024-bit input travels: ring sample %7d   compressed %10d (seed + body)     copied to the card: plain %10d   seeded %19d" % (z["ring_plain"], z["ring_compressed"], z["ring_plain"], z["ring_compressed"]))
    say("   (1,024 LWE samples of n + 1 words, the form before ring inputs, are %d bytes)" % (1024 * 631 * 4))
    say()
    say("2. Time from key object to first completed pack, MEASURED here, ms (wall; from the words the server received to the end of")
    say("   the first pack of 4 samples, minus a second pack); shader clock of a 1,024-gate flush right after: %.4f GHz" % m["pack_ghz"])
    for r in m["pack"]:
        say("   round %d  %-6s  create %7.2f  first pack %7.2f  second pack %5.2f  -> first pack done after %7.2f" % (r["round"] + 1, r["path"], r["create_ms"], r["first_ms"], r["second_ms"], r["usable_ms"]))
    med = {p: statistics.median(r["usable_ms"] for r in m["pack"] if r["path"] == p) for p in ("plain", "device")}
    medf = {p: statistics.median(r["first_ms"] - r["second_ms"] for r in m["pack"] if r["path"] == p) for p in ("plain", "device")}
    say("   medians: plain %.2f ms, device-expanded %.2f ms (%s); the first pack alone, creation left out: plain %.2f, device-expanded %.2f" % (
        med["plain"], med["device"], "FASTER by %.2f ms" % (med["plain"] - med["device"]) if med["device"] < med["plain"] else "NOT faster, by %.2f ms" % (med["device"] - med["plain"]), medf["plain"], medf["device"]))
    say()
    u = m["unpack"]
    blocks = 1024 * 128
    est_ms = 1e3 * blocks * EST_VALU_PER_BLOCK / (256 * 4 * 16 * m["unpack_ghz"] * 1e9)
    added = u["seeded"][0] - u["plain"][0]
    say("3. Unpack of 1,024 samples from device memory between two stream events, MEASURED here, ms, median (min) of %d, the two forms" % args.reps)
    say("   alternately in one loop; shader clock of a 1,024-gate flush right after: %.4f GHz" % m["unpack_ghz"])
    say("   plain (8,192 bytes in) %.4f (%.4f)    seeded (4,136 bytes in) %.4f (%.4f)    seeded - plain %+.4f    seeded / plain %.3f" % (u["plain"][0], u["plain"][1], u["seeded"][0], u["seeded"][1], added, u["seeded"][0] / u["plain"][0]))
    say("   The counted estimate beside it (NOT a measurement): one row per workgroup = 1,024 x 128 = %d blocks of about %d VALU" % (blocks, EST_VALU_PER_BLOCK))
    say("   operations a lane = %.2e lane-operations; on 256 CUs x 4 SIMDs x 16 lanes at that clock %.4f ms of issue." % (blocks * EST_VALU_PER_BLOCK, est_ms))
    say("   added time / estimate = %.1f" % (added / est_ms))
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
