#!/usr/bin/env python3
"""What a linear combination costs (profiles/linear_ops.txt), for information: a flush that holds nothing but `width`
16-term tfhe_hip_linear ops next to one that holds nothing but `width` bootsNOTs, and each next to the same flush of ONE
op (the host's share: plan, descriptor upload, launch, wait).  Times are the flush's wall time on the host
(TfheHipStats::ms_flush_wall): neither kernel is bracketed by events.  The shader clock of each round comes from a level
of 512 bootsANDs run with kernel timing just before it.  Usage: python tools/linear_cost.py [--rounds 3] [--width 4096]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peba1_amd import api, lib  # noqa: E402


def flush_wall(run):
    api.reset_stats()
    run()
    api.flush()
    s = api.stats()
    return s["ms_flush_wall"], s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=4096)
    args = ap.parse_args()
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 7, device=True)
    L.tfhe_hip_set_encrypt_seed(1)
    api.set_deferred(True)
    W = args.width
    rng = np.random.default_rng(0)
    words = rng.integers(-2 ** 31, 2 ** 31, (W + 15, pp.words), dtype=np.int64).astype(np.int32)
    src = api.CiphertextArray(pp, W + 15).set_words(words)
    out = api.CiphertextArray(pp, W)
    a = api.CiphertextArray(pp, 512).encrypt(rng.integers(0, 2, 512), ks)
    g = api.CiphertextArray(pp, 512)
    coefs = [int(c) for c in rng.integers(-2 ** 31, 2 ** 31, 16)]

    def lins(n):
        for i in range(n):
            api.linear(out.at(i), [src.at(i + t) for t in range(16)], coefs, 5, ks)

    def nots(n):
        for i in range(n):
            L.bootsNOT(out.at(i), src.at(i), ks.cloud)

    def clock():
        L.tfhe_hip_set_kernel_timing(1)
        _, s = flush_wall(lambda: api.gate_batch("AND", g, a, a, ks))
        L.tfhe_hip_set_kernel_timing(0)
        return 0.1 * s["clk_shader_cycles"] / s["clk_ref_ticks"] if s["clk_ref_ticks"] else float("nan")

    flush_wall(lambda: lins(W)), flush_wall(lambda: nots(W)), clock()           # warm-up
    for r in range(args.rounds):
        ghz = clock()
        for name, run in (("16-term linear", lins), ("NOT           ", nots)):
            one, _ = flush_wall(lambda: run(1))
            many, s = flush_wall(lambda: run(W))
            assert s["linear_ops"] == W and s["blind_rotates"] == 0
            print(f"round {r}: {W} x {name}: flush {many:7.3f} ms, of ONE op {one:6.3f} ms, difference {many - one:7.3f} ms "
                  f"({1e3 * (many - one) / W:6.3f} us per op)  launches {s['lincomb_launches'] or 1}  shader clock before it {ghz:.3f} GHz")
    want = np.zeros(pp.words, dtype=np.uint32)
    for t, c in enumerate(coefs):
        want += np.uint32(c & 0xFFFFFFFF) * words[t].view(np.uint32)
    lins(1)
    want[-1] += np.uint32(5)
    assert (out.words()[0].view(np.uint32) == want).all()
    ks.close()


if __name__ == "__main__":
    main()
