#!/usr/bin/env python3
"""What a seed-compressed selector costs and saves at P128 (profiles/seeded_selector.txt).  The twin of
tools/public_cost.py, whose child-process discipline and bench step (tools/select_cost.py) it uses: every step on the GPU
runs in a child under a time limit of its own, and after the first child that ends badly nothing more is started on the
card.  Nothing is fixed in advance; what could not be run is written down as NOT MEASURED.

  1. The wire: a 10-bit selector and a one-sample TGSW probe, plain and compressed, in bytes -- counts, not measurements.
  2. The bytes copied to the card for the selector's image, from tfhe_hip_selector_upload_bytes.
  3. From words in hand to the first completed select: a 10-bit selector over 1,024 ring samples resident on the card; the
     constructor, the first tfhe_hip_ring_select_device (which makes the image: twiddles, upload, [expand,] transform, a
     stream wait) and a stream wait behind the tree, by the host clock; plain against compressed in ONE process,
     alternating, one warm-up round, then three: the medians.  The words of the two selects are compared once.
  4. With --parent DIR: bench.py alternating parent and this tree, per shader GHz, both spreads.

    python tools/seeded_select_cost.py [--parent DIR] [--pairs 3] [--out profiles/seeded_selector.txt]
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

BEGIN = "---- report of tools/seeded_select_cost.py: begin (this part is rewritten by the tool) ----"
END = "---- report of tools/seeded_select_cost.py: end ----"
NBITS, M = 10, 1024


def measure():
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=False)          # the client's key: the select needs no cloud key
    N = pp.N
    rng = np.random.default_rng(1)
    index = 0x2A5
    bits = [(index >> j) & 1 for j in range(NBITS)]
    record = api.tgsw_encrypt_bits_compressed(bits, ks, seed=21)
    plain = api.tgsw_expand(record, pp)                        # the same samples as plain words: the two selects must agree
    probe = api.tgsw_encrypt_polys_compressed(np.ones((1, N), dtype=np.int32), ks, seed=22)
    gallery = rng.integers(-2 ** 31, 2 ** 31, size=(M, 2 * N), dtype=np.int64).astype(np.int32)
    dgallery = torch.from_numpy(gallery.reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    make = {"plain": lambda: api.Selector(pp, plain), "compressed": lambda: api.Selector.from_compressed(pp, record)}
    first_s, again_s, upload, words = {"plain": [], "compressed": []}, {"plain": [], "compressed": []}, {}, {}
    for rnd in range(4):
        for kind in ("plain", "compressed"):
            t0 = time.perf_counter()
            sel = make[kind]()
            out = api.ring_select(sel, dgallery, device=True)
            assert L.tfhe_hip_stream_sync() == 0
            t1 = time.perf_counter()
            out2 = api.ring_select(sel, dgallery, device=True)     # the image is resident now
            assert L.tfhe_hip_stream_sync() == 0
            t2 = time.perf_counter()
            upload[kind] = sel.upload_bytes()
            words[kind] = out.cpu().numpy()
            assert np.array_equal(words[kind], out2.cpu().numpy())
            sel.close()
            if rnd >= 1:
                first_s[kind].append(t1 - t0)
                again_s[kind].append(t2 - t1)
    print(json.dumps({"N": N, "l": pp.l, "first_s": first_s, "again_s": again_s, "upload": upload,
                      "same_words": bool(np.array_equal(words["plain"], words["compressed"])),
                      "wire": {"selector_plain": int(plain.nbytes), "selector_compressed": int(record.nbytes),
                               "probe_plain": 4 * api.tgsw_words(pp), "probe_compressed": int(probe.nbytes)}}))
    ks.close()


def fmt(v, scale=1e3, unit="%.3f"):
    return "%s; median %s" % (", ".join(unit % (x * scale) for x in v), unit % (float(np.median(v)) * scale))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_selector.txt"))
    args = ap.parse_args()
    if args.step == "select":
        measure()
        return 0
    lines = ["tools/seeded_select_cost.py: as measured, nothing fixed in advance", ""]
    stopped = None                   # why nothing more may be started on the card
    m, why = child([sys.executable, os.path.abspath(__file__), "--step", "select"], 300)
    if m is None:
        stopped = "the select step: " + why
        lines.append("1.-3. compressed selector at P128: NOT MEASURED (%s)" % why)
    else:
        w, f, a = m["wire"], m["first_s"], m["again_s"]
        lines += [
            "1. on the wire, bytes (counts, not measurements): a %d-bit selector %d plain, %d compressed (%.4f); a one-sample TGSW probe "
            "%d plain, %d compressed" % (NBITS, w["selector_plain"], w["selector_compressed"], w["selector_compressed"] / w["selector_plain"],
                                         w["probe_plain"], w["probe_compressed"]),
            "2. copied to the card for the image of the %d-bit selector (tfhe_hip_selector_upload_bytes): %d plain, %d compressed"
            % (NBITS, m["upload"]["plain"], m["upload"]["compressed"]),
            "3. P128 (N = %d), %d-bit selector, %d ring samples resident on the card; words in hand -> constructor -> first"
            % (m["N"], NBITS, M),
            "   tfhe_hip_ring_select_device (makes the image) -> stream wait, host clock, ms; one process, alternating, three rounds after one warm-up round:",
            "   plain words:       %s" % fmt(f["plain"]),
            "   compressed record: %s" % fmt(f["compressed"]),
            "   compressed / plain, medians: %.3f" % (float(np.median(f["compressed"])) / float(np.median(f["plain"]))),
            "   a second select under the resident image, same loop, ms:",
            "   plain words:       %s" % fmt(a["plain"]),
            "   compressed record: %s" % fmt(a["compressed"]),
            "   the two selects give the same words: %s" % m["same_words"],
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
