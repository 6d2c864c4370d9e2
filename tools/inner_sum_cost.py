#!/usr/bin/env python3
"""What a summed TGSW product costs at P128 (profiles/ring_inner_sum.txt).  The twin of tools/public_sum_cost.py, whose
child-process discipline and bench step (tools/select_cost.py) it uses: every step on the GPU runs in a child under a time
limit of its own, and after the first child that ends badly nothing more is started on the card.  Nothing is fixed in
advance; what could not be run is written down as NOT MEASURED.

  1. 1,024 entries of 2 x 128 bits (128 groups of two ring samples).  ONE terms = 2 launch of tfhe_hip_ring_inner_sum beside
     the TWO launches of tfhe_hip_ring_inner it replaces (term 0's samples under selector sample 0, term 1's under sample 1)
     between stream events (tfhe_hip_last_select_ms), in ONE alternating loop, three warm-up rounds, then three: the
     medians and the shader clock of the run.
  2. The whole identify.match_by_inner_long beside the K-call route -- two tfhe_hip_ring_inner calls, 2,048 key switches,
     one recorded linear op per entry that adds the two inner products and the addend, the same LUT bootstrap and flush --
     in wall time, same loop; both routes' decisions against the plaintext outside the band.
  3. identify.match_by_inner_masked (2,048-bit masked entries at 8/25, terms = 4) beside identify.match_by_inner (128-bit
     entries) on equally many entries: key switches, bootstraps and rotation launches from tfhe_hip_get_stats, and the wall
     time, which is reported only.
  4. With --parent DIR: bench.py alternating parent and this tree, per shader GHz, both spreads.

    python tools/inner_sum_cost.py [--parent DIR] [--pairs 3] [--out profiles/ring_inner_sum.txt]
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

BEGIN = "---- report of tools/inner_sum_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/inner_sum_cost.py: end ----"
M, WIDTH, TERMS, TAU = 1024, 128, 2, 82
MASKED_M, LENGTH, NUM, DEN = 256, 2048, 8, 25
COUNTED = ("keyswitches", "blind_rotates", "br_launches", "levels", "flushes", "lincomb_ops", "ks_pergate_launches", "ks_strip_launches",
           "ks_index_launches")


def measure():
    import torch
    from peba1_amd import api, identify, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    L.tfhe_hip_set_encrypt_seed(3)
    api.set_deferred(True)
    N = pp.N
    sw = 2 * N
    rng = np.random.default_rng(1)
    groups = M // (N // WIDTH)
    length = TERMS * WIDTH
    probe = rng.integers(0, 2, length)
    entries = rng.integers(0, 2, (M, length))
    entries[::2] = probe
    for i in range(0, M, 2):
        entries[i, rng.choice(length, (7 * i) % 61, replace=False)] ^= 1
    dist = (entries ^ probe).sum(axis=1)
    delta = identify.inner_delta(length)
    band = identify.inner_sum_decision_band(pp, delta, TERMS)
    outside = np.abs(dist - TAU) >= band
    gal = identify.pack_gallery_inner_long(entries, WIDTH, TERMS, ks, seed=100).reshape(groups, TERMS, sw)
    words, addend = identify.hamming_probe_long(probe, WIDTH, TERMS, ks, seed=7)
    sel = api.Selector(pp, words)
    dgal = torch.from_numpy(gal.reshape(-1).copy()).to("cuda:0")
    dterm = [torch.from_numpy(gal[:, t].reshape(-1).copy()).to("cuda:0") for t in range(TERMS)]     # the K-call route's galleries
    torch.cuda.synchronize()
    L.tfhe_hip_set_kernel_timing(1)
    lut = api.Lut.constant(pp, 1 << 29)
    c0 = (2 * TAU + 1) * delta // 2
    sum_ms, two_ms, sum_s, two_s = [], [], [], []
    right_sum = right_two = None
    for i in range(6):
        # launches alone, between stream events
        r = api.CiphertextArray(pp, M)
        api.ring_inner_sum(sel, 0, TERMS, dgal, M, WIDTH, ks, r, device=True)
        ts = api.last_select_ms()
        parts, tk = [api.CiphertextArray(pp, M) for _ in range(TERMS)], 0.0
        for t in range(TERMS):
            api.ring_inner(sel, t, dterm[t], M, WIDTH, ks, parts[t], device=True)
            tk += api.last_select_ms()
        assert L.tfhe_hip_stream_sync() == 0
        for o in [r] + parts:
            o.close()
        # the whole routes, wall time
        t0 = time.perf_counter()
        b1 = identify.match_by_inner_long(sel, dgal, TERMS, M, WIDTH, addend, TAU, ks)
        t1 = time.perf_counter()
        parts = [api.CiphertextArray(pp, M) for _ in range(TERMS)]
        for t in range(TERMS):
            api.ring_inner(sel, t, dterm[t], M, WIDTH, ks, parts[t], device=True)
        lin, b2 = api.CiphertextArray(pp, M), api.CiphertextArray(pp, M)
        for j in range(M):
            api.linear(lin.at(j), [p.at(j) for p in parts] + [addend.at(0)], [-1] * (TERMS + 1), c0, ks)
        api.lut_bootstrap_batch(lut, b2, [lin], [1], 0, ks)
        api.flush()
        t2 = time.perf_counter()
        if i == 0:
            want = (dist <= TAU)
            right_sum = bool((np.array([int(v) for v in b1.decrypt(ks)])[outside] == want[outside]).all())
            right_two = bool((np.array([int(v) for v in b2.decrypt(ks)])[outside] == want[outside]).all())
        for o in parts + [lin, b1, b2]:
            o.close()
        if i >= 3:
            sum_ms.append(ts)
            two_ms.append(tk)
            sum_s.append(t1 - t0)
            two_s.append(t2 - t1)
    L.tfhe_hip_set_kernel_timing(0)
    lut.close()
    sel.close()
    del dgal, dterm
    # 3. masked beside unmasked, equally many entries
    b, m = rng.integers(0, 2, LENGTH), (rng.random(LENGTH) < 0.9).astype(np.int64)
    codes = rng.integers(0, 2, (MASKED_M, LENGTH))
    codes[::2] = b
    for i in range(0, MASKED_M, 2):
        codes[i, rng.choice(LENGTH, (37 * i) % 400, replace=False)] ^= 1
    masks = (rng.random((MASKED_M, LENGTH)) < 0.85).astype(np.int64)
    width = N
    mgal = torch.from_numpy(identify.masked_gallery_inner(codes, masks, width, NUM, DEN, ks, seed=5000).reshape(-1).copy()).to("cuda:0")
    msel = api.Selector(pp, identify.masked_probe_tgsw(b, m, width, NUM, DEN, ks, seed=21))
    D = np.array([identify.masked_decision(b, codes[i], m, masks[i], NUM, DEN) for i in range(MASKED_M)])
    mband = identify.masked_inner_band(pp, LENGTH, width, DEN)
    moutside = np.abs(D) >= mband
    pb128 = rng.integers(0, 2, 128)
    e128 = rng.integers(0, 2, (MASKED_M, 128))
    pgal = torch.from_numpy(identify.pack_gallery_inner(e128, 128, ks, seed=9000).reshape(-1).copy()).to("cuda:0")
    pwords, paddend = identify.hamming_probe(pb128, 128, ks, seed=22)
    psel = api.Selector(pp, pwords)
    torch.cuda.synchronize()
    masked_s, plain_s, counts, right = [], [], {}, None
    for i in range(4):
        s0 = api.stats()
        t0 = time.perf_counter()
        b1 = identify.match_by_inner_masked(msel, mgal, MASKED_M, width, LENGTH, NUM, DEN, ks)
        t1 = time.perf_counter()
        s1 = api.stats()
        b2 = identify.match_by_inner(psel, pgal, MASKED_M, 128, paddend, 40, ks)
        t2 = time.perf_counter()
        s2 = api.stats()
        if i >= 1:
            masked_s.append(t1 - t0)
            plain_s.append(t2 - t1)
        counts = {"masked": {f: s1[f] - s0[f] for f in COUNTED}, "unmasked": {f: s2[f] - s1[f] for f in COUNTED}}
        got = np.array([int(v) for v in b1.decrypt(ks)])
        right = bool((got[moutside] == (D[moutside] <= 0)).all())
        b1.close()
        b2.close()
    res = {"N": N, "groups": groups, "sum_ms": sum_ms, "two_ms": two_ms, "sum_s": sum_s, "two_s": two_s, "right_sum": right_sum,
           "right_two": right_two, "outside_long": int(outside.sum()), "band_long": band, "masked_s": masked_s, "plain_s": plain_s,
           "counts": counts, "right": right, "outside": int(moutside.sum()), "band": mband}
    # the shader clock of this run: one 1,024-gate level with kernel timing on, as tools/select_cost.py takes it
    L.tfhe_hip_set_kernel_timing(1)
    bits = rng.integers(0, 2, (2, N))
    a, b2, g = api.CiphertextArray(pp, N).encrypt(bits[0], ks), api.CiphertextArray(pp, N).encrypt(bits[1], ks), api.CiphertextArray(pp, N)
    api.flush()
    api.reset_stats()
    assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], g.ptr, a.ptr, b2.ptr, N, ks.cloud) == 0
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_inner_sum.txt"))
    args = ap.parse_args()
    if args.step == "sum":
        measure()
        return 0
    lines = ["tools/inner_sum_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    m, why = child([sys.executable, os.path.abspath(__file__), "--step", "sum"], 400)
    if m is None:
        stopped = "the product step: " + why
        lines.append("1.-3. summed TGSW products at P128: NOT MEASURED (%s)" % why)
    else:
        med = lambda v: float(np.median(v))   # noqa: E731
        lines += [
            "1. P128 (N = %d), %d entries of %d x %d bits, %d groups = workgroups, launches between stream events, ms" % (m["N"], M, TERMS, WIDTH, m["groups"])
            + (" (shader clock %.3f GHz)" % m["ghz"] if m["ghz"] else ""),
            "   one alternating loop, three rounds after three warm-up rounds:",
            "   ONE tfhe_hip_ring_inner_sum launch, terms = 2 (12 forward + 2 inverse wave transforms a wave):         %s" % fmt(m["sum_ms"]),
            "   the TWO tfhe_hip_ring_inner launches it replaces, summed (2 x (6 forward + 2 inverse)):                %s" % fmt(m["two_ms"]),
            "   one launch / two launches, medians: %.3f" % (med(m["sum_ms"]) / med(m["two_ms"])),
            "2. the whole route, wall seconds, same loop -- identify.match_by_inner_long: one call, %d key switches of rows,"
            " %d linear ops of two samples, %d bootstraps, one flush:" % (M, M, M),
            "   %s" % fmt(m["sum_s"]),
            "   the K-call route: two calls, %d key switches of rows, %d linear ops of three samples, %d bootstraps, one flush:" % (2 * M, M, M),
            "   %s" % fmt(m["two_s"]),
            "   one route / the other, medians: %.3f; decisions right for the %d entries outside the band (|d - tau| >= %d): summed %s, K-call %s"
            % (med(m["sum_s"]) / med(m["two_s"]), m["outside_long"], m["band_long"], m["right_sum"], m["right_two"]),
            "3. the whole match on %d entries, wall seconds, three rounds after one warm-up round, one alternating loop:" % MASKED_M,
            "   identify.match_by_inner_masked (%d-bit masked entries at %d/%d, terms = 4): %s" % (LENGTH, NUM, DEN, fmt(m["masked_s"])),
            "   identify.match_by_inner (128-bit entries):                                 %s" % fmt(m["plain_s"]),
            "   tfhe_hip_get_stats, one match, masked:   %s" % json.dumps(m["counts"]["masked"]),
            "   tfhe_hip_get_stats, one match, unmasked: %s" % json.dumps(m["counts"]["unmasked"]),
            "   a masked match needs no more key switches, bootstraps or launches than an unmasked one: %s"
            % ("CONFIRMED" if all(m["counts"]["masked"][f] <= m["counts"]["unmasked"][f] for f in COUNTED) else "WITHDRAWN"),
            "   masked decisions right for the %d entries outside the band (|D| >= %d): %s" % (m["outside"], m["band"], m["right"]),
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
