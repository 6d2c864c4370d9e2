#!/usr/bin/env python3
"""Writes tests/golden/gate3_circuit_digests.json: SHA-256 of the output ciphertexts of a 16-bit
peba1_hamming_match_csa and of a 2-slot peba1_function_f_fast3, recorded over the netlist provider
(tests/mock/netlist_tfhe.cpp, which has tfhe_hip_gate3) and evaluated gate by gate on the CPU ORACLE from fixed
seeds -- the three-input gates as the oracle's bootstrap and key switch of t = s (+-A +- B +- C)
(tests/gate3_common.py).  tests/test_gate3_cpu.py recomputes them; tests/test_gpu_gate3.py regenerates the same keys
and inputs with the product and must reproduce them bit for bit.  Takes about a minute."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gate3_common as G  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def main():
    O.build()
    oks = O.KeySet(O.params("P128"), G.KEY_SEED)
    out = {"key_seed": G.KEY_SEED, "encrypt_seed": G.ENC_SEED, "parameter_set": "P128"}
    with tempfile.TemporaryDirectory() as tmp:
        G.build_netlist_provider(tmp)
        jobs = {"hamming_match_csa_16": G.hamming_job("hamming_match_csa", G.HAMMING16["a"], G.HAMMING16["b"],
                                                      G.HAMMING16["bound"], G.HAMMING16["nbits"]),
                "function_f_fast3_2": G.function_f_job("function_f_fast3", G.FF3_2["probe"], G.FF3_2["template"],
                                                       G.FF3_2["bound"], G.FF3_2["bitsize"])}
        for name, job in jobs.items():
            rows, wires = G.record_netlist(tmp, **job)
            w = G.replay_oracle(oks, rows, O.Rng(G.ENC_SEED))
            words = np.stack([w[o] for o in wires])
            boots, depth = G.netlist_cost(rows)
            out[name] = {"inputs": job, "bootstraps": boots, "depth": depth, "decrypted": oks.decrypt(words).tolist(),
                         "sha256": G.sha256_words(words)}
            print(name, out[name])
    with open(G.DIGESTS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
