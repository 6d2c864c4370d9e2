#!/usr/bin/env python3
"""This tree against a built checkout of its parent commit (profiles/engine_staging_ab.txt): the two alternately, parent
first, `--rounds` times -- the per-call times at P128 of a pack, an unpack and a stream-ordered export of 1,024 samples, then
bench.py's headline per GHz of shader clock.  Every step runs once, in a child process under a time limit of its own;
after the first that ends badly nothing more is started on the card.  Per-call times: three warm-up calls, then the median
of `--reps`; the device forms between two HIP events on the library's stream around ONE call (the procedures of
profiles/packing.txt and profiles/unpack.txt: the packed samples are bootsAND outputs on the device, the ring sample lies
in device memory), the host forms by wall clock around ONE call, which returns with its work complete.  The margin is the
parent's own spread over its runs; prints every run, the spread and the verdict.

    python tools/staging_ab.py --parent DIR [--rounds 3] [--reps 30]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (("bench.py headline, gates/s per GHz of shader clock (higher is better)", "bench", "gates_per_s_per_ghz", True, "%.0f"),
        ("pack of 1,024, device form, between two stream events, ms", "percall", "pack_device_events", False, "%.4f"),
        ("pack of 1,024, host form, wall, ms", "percall", "pack_host_wall", False, "%.4f"),
        ("unpack of 1,024, device form, between two stream events, ms", "percall", "unpack_device_events", False, "%.4f"),
        ("unpack of 1,024, host form, wall, ms", "percall", "unpack_host_wall", False, "%.4f"),
        ("export of 1,024, stream-ordered device form, between two stream events, ms", "percall", "export_async_events", False, "%.4f"))


def measure(reps):
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    pk = api.PackingKey(ks, seed=11)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def events(fn):
        for _ in range(3):
            fn()
        assert L.tfhe_hip_stream_sync() == 0
        ms = []
        for _ in range(reps):
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return [float(np.median(ms)), float(np.min(ms))]

    def wall(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return [float(np.median(ms)), float(np.min(ms))]

    rng = np.random.default_rng(1)
    xa, xb = rng.integers(0, 2, N), rng.integers(0, 2, N)
    a, b = api.CiphertextArray(pp, N).encrypt(xa, ks), api.CiphertextArray(pp, N).encrypt(xb, ks)
    r = api.CiphertextArray(pp, N)
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], r.ptr, a.ptr, b.ptr, N, ks.cloud) == 0
    api.flush()
    packed = torch.zeros(2 * N, dtype=torch.int32, device="cuda:0")
    flat = torch.zeros(N * pp.words, dtype=torch.int32, device="cuda:0")
    bits = rng.integers(0, 2, N)
    ring = api.ring_encrypt_bits(bits, ks, seed=5)
    dring = torch.from_numpy(ring).to("cuda:0")
    torch.cuda.synchronize()
    out = {}
    out["pack_device_events"] = events(lambda: api.pack_device(pk, r, N, ks, packed.data_ptr()))
    out["export_async_events"] = events(lambda: L.tfhe_hip_export_samples_device_async(r.ptr, N, pp.ptr, C.c_void_p(flat.data_ptr())))
    assert L.tfhe_hip_stream_sync() == 0
    assert list(api.packed_decrypt(packed.cpu().numpy(), N, ks)) == list(xa & xb)
    out["pack_host_wall"] = wall(lambda: api.pack(pk, r, N, ks))
    u = api.CiphertextArray(pp, N)
    out["unpack_device_events"] = events(lambda: api.unpack_device(dring.data_ptr(), 1, ks, u, count=N))
    assert L.tfhe_hip_stream_sync() == 0
    assert list(u.decrypt(ks)) == list(bits)
    out["unpack_host_wall"] = wall(lambda: api.unpack(ring, ks, u, count=N))
    assert list(u.decrypt(ks)) == list(bits)
    print(json.dumps(out))




def find(d, key):
    if isinstance(d, dict):
        if key in d and isinstance(d[key], (int, float)):
            return d[key]
        for v in d.values():
            got = find(v, key)
            if got is not None:
                return got
    return None


def child(cmd, cwd, limit):
    """the last JSON line a command printed, or None"""
    try:
        p = subprocess.run(cmd, cwd=cwd, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        print("ended at its time limit of %d s: %s" % (limit, " ".join(cmd)))
        return None
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        print("exit code %d: %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-2000:]))
        return None
    return json.loads(lines[-1])


def report(runs):
    def series(tree, what, key):
        vals = [r["result"][key] for r in runs if r["tree"] == tree and r["what"] == what]
        return [v[0] if isinstance(v, list) else v for v in vals]
    for title, what, key, higher, fmt in ROWS:
        p, c = series("parent", what, key), series("change", what, key)
        if not p or len(p) != len(c):
            print("   %s: NOT MEASURED" % title)
            continue
        spread, mp, mc = max(p) - min(p), statistics.median(p), statistics.median(c)
        worse = (mp - mc) if higher else (mc - mp)
        verdict = ("PASS (within the parent's spread of the parent's median)" if abs(mc - mp) <= spread else
                   "outside the parent's spread, on the FASTER side" if worse < 0 else
                   "FAIL (worse than the parent's median by more than its spread)")
        f = lambda xs: ", ".join(fmt % x for x in xs)
        print("   %s\n     parent: %s   median %s, spread (max - min) %s\n     change: %s   median %s\n     change - parent: %s (%+.2f %%): %s"
              % (title, f(p), fmt % mp, fmt % spread, f(c), fmt % mc, fmt % (mc - mp), 100 * (mc - mp) / mp, verdict))
    for r in runs:
        if r["what"] == "bench":
            print("   bench run: round %d, %s: %.0f gates/s at %.4f GHz" % (r["round"] + 1, r["tree"], r["result"]["gates_per_s"], r["result"]["shader_ghz"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default="")
    args = ap.parse_args()
    if args.step == "percall":
        sys.path.insert(0, os.getcwd())                  # the tree the step was started in, parent or change
        measure(args.reps)
        return 0
    if not args.parent:
        ap.error("--parent DIR: a built checkout of the parent commit")
    runs, ok = [], True
    steps = (("percall", [sys.executable, os.path.abspath(__file__), "--step", "percall", "--reps", str(args.reps)], 240),
             ("bench", [sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"], 420))
    for rnd in range(args.rounds):
        for what, cmd, limit in steps:
            for name, cwd in (("parent", os.path.abspath(args.parent)), ("change", ROOT)):
                res = child(cmd, cwd, limit) if ok else None
                if res is None:
                    ok = False
                    continue
                if what == "bench":
                    gates, ghz = res.get("value"), find(res, "shader_clock_ghz")
                    res = {"gates_per_s": gates, "shader_ghz": ghz, "gates_per_s_per_ghz": find(res, "gates_per_s_per_shader_ghz")}
                runs.append({"round": rnd, "tree": name, "what": what, "result": res})
    report(runs)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
