#!/usr/bin/env python3
"""What opening ring-encrypted inputs costs at P128 (profiles/unpack.txt).  Up to three steps on the GPU, each run at most
once, each in a child process under a time limit of its own.  After the first child that ends at its limit or with a
non-zero exit code nothing more is started on the card: the remaining steps are reported as NOT MEASURED.  The report goes
between the two marker lines of the output file; whatever else that file holds (the commentary) is kept.

  1. The time between two HIP events on the library's stream around ONE tfhe_hip_unpack_samples_device call of 1,024
     samples and of 1 sample.  Beside it, on the same box: a host import (tfhe_hip_import_samples) of the same 1,024
     samples, wall time; a key switch of 1,024 through tfhe_hip_kernel_keyswitch, wall time (it uploads its operands and
     downloads its results), and the key switch of one 1,024-gate level from the statistics with kernel timing on; and the
     counted estimate -- the bytes the extract writes at the memory's peak rate plus that key-switch time -- with the
     ratio of the measured unpack to it, as found.
  2. bench.py --gpus 1 of this tree and, with --parent DIR, of a built checkout of the parent commit in DIR: gates/s per
     GHz of shader clock, both numbers.

    python tools/unpack_cost.py [--reps 30] [--parent DIR] [--out profiles/unpack.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12            # HBM3E peak of the MI355X as specified
BEGIN = "---- report of tools/unpack_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/unpack_cost.py: end ----"


def measure(reps):
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bits = np.random.default_rng(1).integers(0, 2, N)
    ring = api.ring_encrypt_bits(bits, ks, seed=5)
    dev = torch.from_numpy(ring).to("cuda:0")
    torch.cuda.synchronize()
    out = {"n": pp.n, "N": N, "u_stride": N + 4, "reps": reps}
    for count in (1024, 1):
        r = api.CiphertextArray(pp, count)
        ms = []
        for i in range(reps + 3):
            e0.record(stream)
            api.unpack_device(dev.data_ptr(), 1, ks, r, count=count)
            e1.record(stream)
            e1.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        assert L.tfhe_hip_stream_sync() == 0
        assert list(r.decrypt(ks)) == list(bits[:count])
        out["unpack_%d" % count] = [float(np.median(ms)), float(np.min(ms))]
        if count == 1024:
            words = r.words()
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r.set_words(words)
                wall.append((time.perf_counter() - t0) * 1e3)
            out["import_1024_wall"] = [float(np.median(wall)), float(np.min(wall))]
        r.close()
    u = np.random.default_rng(2).integers(-2 ** 31, 2 ** 31, (1024, N + 1), dtype=np.int64).astype(np.int32)
    wall = []
    for _ in range(max(3, reps // 3)):
        t0 = time.perf_counter()
        api.kernel_keyswitch(ks, u)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["kernel_keyswitch_1024_wall"] = [float(np.median(wall)), float(np.min(wall))]
    L.tfhe_hip_set_kernel_timing(1)
    a, b, g = api.CiphertextArray(pp, N).encrypt(bits, ks), api.CiphertextArray(pp, N).encrypt(1 - bits, ks), api.CiphertextArray(pp, N)
    api.flush()
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b.ptr, N, ks.cloud) == 0
    api.flush()
    st = api.stats()
    out["level_keyswitch_1024"] = st["ms_keyswitch"]
    out["level_ghz"] = st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else None
    print(json.dumps(out))


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack.txt"))
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=2)
    args = ap.parse_args()
    if args.step == "unpack":
        measure(args.reps)
        return 0
    lines = ["tools/unpack_cost.py --reps %d: as measured, nothing fixed in advance" % args.reps, ""]
    stopped = None                   # why nothing more may be started on the card
    m, why = child([sys.executable, os.path.abspath(__file__), "--step", "unpack", "--reps", str(args.reps)], 240)
    if m is None:
        stopped = "the unpack step: " + why
        lines.append("1. unpack at P128: NOT MEASURED (%s)" % why)
    else:
        bytes_out = 1024 * m["u_stride"] * 4
        est = bytes_out / PEAK_BYTES_PER_S * 1e3 + m["level_keyswitch_1024"]
        lines += [
            "1. P128 (n = %d, N = %d), median (min) of %d, ms" % (m["n"], m["N"], m["reps"]),
            "   unpack of 1,024 samples, between two stream events:   %.4f (%.4f)" % tuple(m["unpack_1024"]),
            "   unpack of 1 sample, between two stream events:        %.4f (%.4f)" % tuple(m["unpack_1"]),
            "   host import of the same 1,024 samples, wall:          %.4f (%.4f)" % tuple(m["import_1024_wall"]),
            "   tfhe_hip_kernel_keyswitch of 1,024, wall (with its transfers): %.4f (%.4f)" % tuple(m["kernel_keyswitch_1024_wall"]),
            "   key switch of one 1,024-gate level, kernel timing:    %.4f%s" % (m["level_keyswitch_1024"], "  (shader clock %.3f GHz)" % m["level_ghz"] if m["level_ghz"] else ""),
            "   counted estimate: %d bytes written by the extract at %.1f TB/s (%.5f ms) + that key switch = %.4f ms"
            % (bytes_out, PEAK_BYTES_PER_S / 1e12, bytes_out / PEAK_BYTES_PER_S * 1e3, est),
            "   measured unpack of 1,024 / estimate: %.2f" % (m["unpack_1024"][0] / est),
            "   bytes in: %d as one ring sample, %d as 1,024 LWE samples" % (2 * m["N"] * 4, 1024 * (m["n"] + 1) * 4),
        ]
    lines.append("")
    bench = ["bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)]
    for name, cwd in (("this tree", ROOT), ("parent commit", args.parent)):
        if stopped:
            lines.append("2. bench.py, %s: NOT MEASURED, not started (an earlier step ended badly -- %s)" % (name, stopped))
            continue
        if not cwd:
            lines.append("2. bench.py, %s: NOT MEASURED (no --parent checkout given)" % name)
            continue
        res, why = child([sys.executable] + bench, 420, cwd=cwd)
        if res is None:
            stopped = "bench.py of %s: %s" % (name, why)
            lines.append("2. bench.py, %s: NOT MEASURED (%s)" % (name, why))
            continue
        gates, ghz, ratio = per_ghz(res)
        lines.append("2. bench.py --gpus 1 --steps %d --warmup %d, %s: %s gates/s at %s GHz = %s gates/s per GHz"
                     % (args.bench_steps, args.bench_warmup, name, "%.0f" % gates if gates else "n/a",
                        "%.4f" % ghz if ghz else "n/a", "%.0f" % ratio if ratio else "n/a"))
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
