#!/usr/bin/env python3
"""Writes tests/golden/lut_multi_digests.json: the multi-output LUT bootstrap (tfhe_hip_lut_bootstrap_multi) of fixed
cases -- the accumulator from the CPU ORACLE's pieces (tests/lut_common.py), the outputs from the numpy restatement of
the definitions (tests/lut_multi_common.py), the oracle's key switch of each wanted output.  Per case: seeds,
coefficients, c0, the test polynomial's generator, the spec and which outputs are wanted; per output the SHA-256 and
first four words of the key-switched sample (null where not wanted) and the SHA-256 of the extracted sample; the
SHA-256 of the raw accumulator.  CPU only; takes seconds."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lut_common as T  # noqa: E402
import lut_multi_common as M  # noqa: E402
from oracle import pyoracle as O  # noqa: E402


def main():
    O.build()
    out = {"key_seed": M.KEY_SEED, "sets": {}}
    for pname in M.CASES:
        oks = O.KeySet(O.params(pname), M.KEY_SEED)
        cases = []
        for case in M.case_specs(pname):
            cts, us, acc = M.oracle_case(O, oks, case)
            case.update(sha256=[T.sha256_words(ct) if ct is not None else None for ct in cts],
                        first_words=[[int(x) for x in ct[:4]] if ct is not None else None for ct in cts],
                        sha256_extracted=[T.sha256_words(u) for u in us], sha256_accumulator=T.sha256_words(acc))
            cases.append(case)
            print(pname, case["index"], "template", case["template"], case["wanted"], case["sha256_accumulator"][:16], flush=True)
        out["sets"][pname] = {"cases": cases}
        oks.close()
    with open(M.DIGESTS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
