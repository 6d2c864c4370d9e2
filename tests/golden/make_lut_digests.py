#!/usr/bin/env python3
"""Writes tests/golden/lut_bootstrap_digests.json: the LUT bootstrap (tfhe_hip_lut_bootstrap) of fixed cases evaluated
on the CPU ORACLE's own pieces -- accumulator (0, X^-bbar v), the n CMUX steps, sample extract, key switch
(tests/lut_common.py) -- for the three parameter sets, and a chain of 2-bit re-encodings.  Per case: seeds, coefficients,
c0, the test polynomial's generator, SHA-256 and first four words of the output sample, SHA-256 of the extracted sample
and of the raw accumulator.  tests/test_lut_cpu.py recomputes some of them; tests/test_gpu_lut.py regenerates the same
keys and inputs and must reproduce all of them bit for bit on the GPU.  Takes a few minutes."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lut_common as T  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def main():
    O.build()
    out = {"key_seed": T.KEY_SEED, "sets": {}}
    for pname in T.CASES:
        oks = O.KeySet(O.params(pname), T.KEY_SEED)
        cases = []
        for spec in T.case_specs(pname, oks.N):
            inputs = T.case_inputs(O, oks, spec)
            if spec["force_bbar"] is not None:
                spec["c0"] = T.c0_for_bbar(spec["coefs"], inputs, oks.N, spec["force_bbar"])
            lin = T.linear(spec["coefs"], inputs, spec["c0"])
            if spec["force_bbar"] is not None:
                assert T.modswitch(lin[-1], oks.N) == spec["force_bbar"]
            ct, u, acc = T.oracle_lut_bootstrap(O, oks, lin, T.lut_words(spec["lut"], oks.N))
            spec.update(parameter_set=pname, seed=T.KEY_SEED, bbar=T.modswitch(lin[-1], oks.N), sha256=T.sha256_words(ct),
                        first_words=[int(x) for x in ct[:4]], sha256_extracted=T.sha256_words(u),
                        sha256_accumulator=T.sha256_words(acc))
            cases.append(spec)
            print(pname, spec["index"], spec["coefs"], spec["lut"]["kind"], spec["bbar"], spec["sha256"][:16], flush=True)
        out["sets"][pname] = {"cases": cases}
        if pname == T.CHAIN["parameter_set"]:
            out["chain"] = chain(oks)
        oks.close()
    with open(T.DIGESTS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def chain(oks):
    """16 messages x 4 hops of random permutation tables; every oracle output must stand more than 1/32 from a sector
    edge (the margin is 1/16: about twelve standard deviations by the noise analysis -- an estimate; the smallest distance
    seen is recorded, and that is the measurement)."""
    c = dict(T.CHAIN)
    perms = T.chain_perms(c["hops"])
    luts = [T.chain_lut(p, oks.N) for p in perms]
    msgs = [i % 4 for i in range(c["messages"])]
    cts = T.encode_messages(O, oks, msgs, c["enc_seed"])
    key = oks.lwe_key()
    smallest, hops = 1.0, []
    for h in range(c["hops"]):
        cts = np.stack([T.oracle_lut_bootstrap(O, oks, T.linear([1], ct[None, :], 0), luts[h])[0] for ct in cts])
        msgs = [perms[h][m] for m in msgs]
        ph = T.phases(cts, key)
        assert T.decode(ph).tolist() == msgs, (h, T.decode(ph).tolist(), msgs)
        d = float(T.edge_distance(ph).min())
        assert d > 1 / 32, f"hop {h}: an output stands {d:.4f} from a sector edge"
        smallest = min(smallest, d)
        hops.append({"sha256": [T.sha256_words(ct) for ct in cts], "messages": msgs})
        print("chain hop", h, msgs, f"{d:.4f}", flush=True)
    c.update(perms=perms, hops_out=hops, smallest_edge_distance=smallest)
    return c


if __name__ == "__main__":
    main()
