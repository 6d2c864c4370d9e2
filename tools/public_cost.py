#!/usr/bin/env python3
"""What a probe against a CLEAR gallery costs at P128 beside the encrypted inner products (profiles/ring_public.txt).  The
twin of tools/lookup_cost.py, whose child-process discipline and bench step (tools/select_cost.py) it uses: every step on the
GPU runs in a child under a time limit of its own, and after the first child that ends badly nothing more is started on
the card.  Nothing is fixed in advance; what could not be run is written down as NOT MEASURED.

  1. 1,024 templates of 128 bits (R = 128 polynomials / ring samples).  The product-and-extract launch of
     tfhe_hip_ring_inner_public beside that of tfhe_hip_ring_inner between two stream events (tfhe_hip_last_select_ms), in
     ONE alternating loop, three warm-up rounds, then three: the medians and the shader clock of the run.  Transform
     counts per workgroup are stated as counts (4 forward + 4 inverse against 4 l = 12 forward + 4 inverse), not promised.
  2. The whole match, wall time: identify.match_clear_gallery beside identify.match_by_inner, same loop.
  3. The probe on the wire in its three forms: TGSW, ring, seed-compressed ring.
  4. With --parent DIR: bench.py alternating parent and this tree, per shader GHz, both spreads.

    python tools/public_cost.py [--parent DIR] [--pairs 3] [--out profiles/ring_public.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from select_cost import child, per_ghz             # noqa: E402

BEGIN = "---- report of tools/public_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/public_cost.py: end ----"
M, WIDTH, TAU = 1024, 128, 40


def measure():
    import torch
    from peba1_amd import api, identify, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    rng = np.random.default_rng(1)
    probe = rng.integers(0, 2, WIDTH)
    entries = rng.integers(0, 2, (M, WIDTH))
    for i in range(0, M, 3):                                    # every third template near the probe
        entries[i] = probe
        entries[i, rng.choice(WIDTH, (5 * i) % 29, replace=False)] ^= 1
    dist = (entries ^ probe).sum(axis=1)
    band = identify.inner_decision_band(pp, WIDTH)
    outside = np.abs(dist - TAU) >= band
    # the TGSW route: an encrypted gallery, a TGSW probe; the new route: a clear gallery, a ring probe
    enc_gallery = identify.pack_gallery_inner(entries, WIDTH, ks, seed=11)
    tgsw, addend = identify.hamming_probe(probe, WIDTH, ks, seed=12)
    sel = api.Selector(pp, tgsw)
    clear = api.PublicGallery(pp, identify.clear_gallery_polys(entries, WIDTH, N))
    ring, addend2 = identify.hamming_probe_ring(probe, WIDTH, ks, seed=13)
    packed, addend3 = identify.hamming_probe_ring(probe, WIDTH, ks, compressed=True, seed=14)
    dgallery = torch.from_numpy(enc_gallery.reshape(-1)).to("cuda:0")
    dring = torch.from_numpy(ring.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    L.tfhe_hip_set_kernel_timing(1)
    public_ms, inner_ms = [], []
    for i in range(6):
        r = api.CiphertextArray(pp, M)
        api.ring_inner_public(clear, dring, M, WIDTH, ks, r, device=True)
        tp = api.last_select_ms()
        r2 = api.CiphertextArray(pp, M)
        api.ring_inner(sel, 0, dgallery, M, WIDTH, ks, r2, device=True)
        ti = api.last_select_ms()
        assert L.tfhe_hip_stream_sync() == 0
        r.close()
        r2.close()
        if i >= 3:
            public_ms.append(tp)
            inner_ms.append(ti)
    L.tfhe_hip_set_kernel_timing(0)
    clear_s, inner_s, right = [], [], {}
    for i in range(4):
        t0 = time.perf_counter()
        b1 = identify.match_clear_gallery(clear, dring, M, WIDTH, addend2, TAU, ks)
        t1 = time.perf_counter()
        b2 = identify.match_by_inner(sel, dgallery, M, WIDTH, addend, TAU, ks)
        t2 = time.perf_counter()
        if i >= 1:
            clear_s.append(t1 - t0)
            inner_s.append(t2 - t1)
        for name, b in (("clear", b1), ("inner", b2)):
            got = np.array([int(v) for v in b.decrypt(ks)])
            right[name] = bool((got[outside] == (dist[outside] <= TAU)).all())
            b.close()
    res = {"N": N, "l": pp.l, "public_ms": public_ms, "inner_ms": inner_ms, "clear_s": clear_s, "inner_s": inner_s, "right": right,
           "outside": int(outside.sum()), "band": band,
           "wire": {"tgsw": int(tgsw.nbytes), "ring": int(ring.nbytes), "seeded_ring": int(packed.nbytes)}}
    # the shader clock of this run: one 1,024-gate level with kernel timing on, as tools/select_cost.py takes it
    L.tfhe_hip_set_kernel_timing(1)
    bits = rng.integers(0, 2, (2, N))
    a, b, g = api.CiphertextArray(pp, N).encrypt(bits[0], ks), api.CiphertextArray(pp, N).encrypt(bits[1], ks), api.CiphertextArray(pp, N)
    api.flush()
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b.ptr, N, ks.cloud) == 0
    api.flush()
    st = api.stats()
    res["ghz"] = st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else None
    print(json.dumps(res))


def fmt(v, unit="%.4f"):
    return "%s; median %s" % (", ".join(unit % x for x in v), unit % float(np.median(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_public.txt"))
    args = ap.parse_args()
    if args.step == "public":
        measure()
        return 0
    lines = ["tools/public_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    m, why = child([sys.executable, os.path.abspath(__file__), "--step", "public"], 300)
    if m is None:
        stopped = "the product step: " + why
        lines.append("1.-3. probe against a clear gallery at P128: NOT MEASURED (%s)" % why)
    else:
        R = M // (m["N"] // WIDTH)
        lines += [
            "1. P128 (N = %d), %d templates of %d bits, R = %d workgroups, the product-and-extract launch between two stream events, ms"
            % (m["N"], M, WIDTH, R) + (" (shader clock %.3f GHz)" % m["ghz"] if m["ghz"] else ""),
            "   one alternating loop, three rounds after three warm-up rounds:",
            "   tfhe_hip_ring_inner_public (ring probe, clear gallery; 4 forward + 4 inverse wave transforms a workgroup):  %s" % fmt(m["public_ms"]),
            "   tfhe_hip_ring_inner (TGSW probe, encrypted gallery; %d forward + 4 inverse):                               %s"
            % (4 * m["l"], fmt(m["inner_ms"])),
            "   public / inner, medians: %.3f (by transform count %d / %d = %.2f was the expectation -- a count, not a promise)"
            % (float(np.median(m["public_ms"])) / float(np.median(m["inner_ms"])), 8, 4 * m["l"] + 4, 8.0 / (4 * m["l"] + 4)),
            "2. the whole match (product, key switch, %d linear combinations, one level of %d bootstraps, one flush), wall seconds," % (M, M),
            "   three rounds after one warm-up round, same alternating loop, tau = %d:" % TAU,
            "   identify.match_clear_gallery: %s" % fmt(m["clear_s"]),
            "   identify.match_by_inner:      %s" % fmt(m["inner_s"]),
            "   decisions right for the %d templates outside the band (g = %d): clear gallery %s, TGSW route %s"
            % (m["outside"], m["band"], m["right"]["clear"], m["right"]["inner"]),
            "3. the probe on the wire, bytes: TGSW sample %d, ring sample %d, seed-compressed ring sample %d"
            % (m["wire"]["tgsw"], m["wire"]["ring"], m["wire"]["seeded_ring"]),
        ]
    lines.append("")
    bench = ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = {"parent commit": [], "this tree": []}
    for pair in range(args.pairs if args.parent else 0):
        for name, cwd in (("parent commit", args.parent), ("this tree", ROOT)):
            if stopped:
                lines.append("4. bench.py, pair %d, %s: NOT MEASURED, not started (an earlier step ended badly -- %s)" % (pair + 1, name, stopped))
                continue
            res, why = child([sys.executable] + bench, 420, cwd=cwd)
            if res is None:
                stopped = "bench.py of %s: %s" % (name, why)
                lines.append("4. bench.py, pair %d, %s: NOT MEASURED (%s)" % (pair + 1, name, why))
                continue
            gates, ghz, ratio = per_ghz(res)
            runs[name].append(ratio)
            lines.append("4. bench.py --gpus 1 --steps 20 --warmup 5, pair %d, %s: %.0f gates/s at %.4f GHz = %.0f gates/s per GHz"
                         % (pair + 1, name, gates, ghz, ratio))
    if not args.parent:
        lines.append("4. bench.py against the parent commit: NOT MEASURED (no --parent checkout given)")
    elif runs["parent commit"] and runs["this tree"]:
        p, t = runs["parent commit"], runs["this tree"]
        lines.append("   per GHz, parent: median %.0f, spread %.0f .. %.0f (%.2f %%); this tree: median %.0f, spread %.0f .. %.0f (%.2f %%); "
                     "difference of the medians %+.2f %%"
                     % (np.median(p), min(p), max(p), (max(p) - min(p)) / np.median(p) * 100, np.median(t), min(t), max(t),
                        (max(t) - min(t)) / np.median(t) * 100, (np.median(t) - np.median(p)) / np.median(p) * 100))
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
