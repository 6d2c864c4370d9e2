#!/usr/bin/env python3
"""Writes tests/golden/ntt_bounds_inputs*.npz (file_of): per (pipeline, N, prime, direction, step) the input, out of everything the
admission predicates allow, that a seeded search (64 uniform random inputs, 64 more on the extremes, greedy moves) found
to push the largest |intermediate| after that step of the lazy wave NTT furthest toward its interval bound.  The search runs
on the emulation of tests/ntt_bounds_common.py; tests/test_ntt_bounds_cpu.py regenerates N = 1024 cases and compares the
bytes of the arrays, tests/test_gpu_ntt_bounds.py runs every entry through the kernels against the exact integer product.

Pipelines (ntt_bounds_common.pipeline_*):
  public       ring words (full 32-bit) and a gallery polynomial |q| <= T: directions fwd (the transform of the reduced
               words), inv (the inverse transform of the reduced product) and img (the transform of q itself)
  negacyclic   one digit polynomial |d| <= T and one key polynomial (negacyclic_kernel, negacyclic_split_kernel)
  gadget       (k+1) l rows of signed gadget digits and key rows at the most rows a selector is accepted with: l = 9,
               Bgbit = 3 at N = 1024 (18 rows, the MAC limit), l = 7, Bgbit = 4 at N = 2048 (14 rows: l = 8 passes the MAC
               bound of cmux.hpp but no blind-rotate form, so no parameter set carries it) (cmux_kernel, inner_kernel)
  pack1        t rows of 1-bit digits at the MAC limit, t = 18 / 16: the only digit width whose t reaches it (t basebit <= 32)
  pack4        t = 8 rows of 4-bit digits, 0 <= d <= 15: the most rows basebit 4 is accepted with (pack_kernel)
Key words are searched as WORDS, not as image words: they move over a palette (0, +-1, +-(P - 1), (P - 1) / 2, the ends of
int32 and eight seeded random words), the image follows through the model of bk_transform_kernel, and one key serves both
primes on the card.  Entry names: <pipeline>/<N>/p<prime>/<direction>/<step>/<array>; an entry stores only the arrays its
target depends on.

    python tests/golden/make_ntt_bounds_inputs.py            # a few minutes on 8 cores
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, os.pardir))
import ntt_bounds_common as B   # noqa: E402

PATH = os.path.join(HERE, "ntt_bounds_inputs.npz")


def file_of(name):
    """the file an array lives in: the one-row pipelines together, the many-row ones a file per pipeline and ring size (the
    keys and digits of 14 to 18 rows an entry: each file stays under the size a committed file may have)"""
    pipeline, N = name.split("/")[:2]
    return PATH if pipeline in ("public", "negacyclic") else PATH[:-4] + "_%s_%s.npz" % (pipeline, N)


def load():
    """every array of the fixture, {name: int32 array}"""
    import glob
    arrays = {}
    for path in sorted(glob.glob(PATH[:-4] + "*.npz")):
        with np.load(path) as z:
            arrays.update({k: z[k] for k in z.files})
    return arrays
SEED = 0x4E7742
RANDOM, RESTARTS, ROUNDS, CANDS = 64, 64, 120, 8
ROUNDS_ROWS, CANDS_ROWS = 40, 6                     # the many-row pipelines: a round costs rows times as much
PIPELINES = ("public", "negacyclic", "gadget", "pack1", "pack4")
# the digit pipelines: per log N (rows, least digit, largest digit) and what realises them on the card
GADGET = {10: (9, 3), 11: (7, 4)}                   # (l, Bgbit): rows = 2 l, digits in [-Bg/2, Bg/2)
PACK = {"pack1": {10: (18, 1), 11: (16, 1)}, "pack4": {10: (8, 4), 11: (8, 4)}}      # (t, basebit): digits in [0, 2^basebit)


def digit_shape(pipeline, logn):
    """(rows, least digit, largest digit)"""
    if pipeline == "negacyclic":
        T = B.max_coef(1 << logn)
        return 1, -T, T
    if pipeline == "gadget":
        l, bg = GADGET[logn]
        return 2 * l, -(1 << (bg - 1)), (1 << (bg - 1)) - 1
    t, bb = PACK[pipeline][logn]
    return t, 0, (1 << bb) - 1


def word_class(field):
    P = field.P
    return np.array([B.I32_MIN, B.I32_MAX, P - 1, -(P - 1), (P - 1) // 2, -((P - 1) // 2)], dtype=np.int64), B.I32_MIN, B.I32_MAX


def digit_class(D, lo=None):
    """digits between their extremes and 0"""
    lo = -D if lo is None else lo
    return np.unique(np.array([lo, 0, D], dtype=np.int64)), lo, D


def key_class(field):
    """the palette of key words (lo None: ntt_bounds_common.uniform_draw)"""
    P = field.P
    rnd = np.random.default_rng([SEED, 2, field.logn, field.prime]).integers(B.I32_MIN, B.I32_MAX + 1, size=8)
    return np.concatenate([[0, 1, -1, P - 1, -(P - 1), (P - 1) // 2, B.I32_MIN, B.I32_MAX], rnd]).astype(np.int64), None, None


def targets_of(pipeline, field):
    nf, ni = len(field.fwd_steps), len(field.inv_steps)
    t = [("fwd", k) for k in range(nf)] + [("inv", k) for k in range(ni)]
    return t + [("img", k) for k in range(nf)] if pipeline == "public" else t


def problem(pipeline, field):
    """(classes for ntt_bounds_common.search, evaluate) of one pipeline, ring size and prime"""
    N, T = field.N, B.max_coef(field.N)
    if pipeline == "public":
        classes = {"words": ((N,),) + word_class(field), "q": ((N,),) + digit_class(T)}

        def evaluate(x):
            r = B.pipeline_public(field, x["words"], x["q"])
            return np.stack(r["fwd"] + r["inv"] + r["img"], axis=1).astype(np.float64)
    else:
        rows, lo, hi = digit_shape(pipeline, field.logn)
        classes = {"digits": ((rows, N),) + digit_class(hi, lo), "key": ((rows, N),) + key_class(field)}

        def evaluate(x):
            r = B.pipeline_digits(field, x["digits"], field.image(x["key"]))
            return np.stack(r["fwd"] + r["inv"], axis=1).astype(np.float64)
    return classes, evaluate


# which arrays a target depends on, and under which name they are stored
STORED = {("public", "fwd"): {"words": "words"}, ("public", "inv"): {"words": "words", "q": "q"}, ("public", "img"): {"q": "q"},
          "fwd": {"digits": "digits"}, "inv": {"digits": "digits", "key": "key"}}


def stored(pipeline, direction):
    return STORED[pipeline, direction] if pipeline == "public" else STORED[direction]


def random_inputs(pipeline, field, classes):
    """the RANDOM uniform inputs of the admitted set that the search starts from and its result is compared with"""
    return B.uniform_inputs(classes, np.random.default_rng([SEED, 1, PIPELINES.index(pipeline), field.logn, field.prime]), RANDOM)


def find(pipeline, logn, prime, report=None):
    """{entry name: int32 array}, {target name: the value reached} of one (pipeline, N, prime)"""
    field = B.Field.get(prime, logn)
    classes, evaluate = problem(pipeline, field)
    targets = targets_of(pipeline, field)
    rng = np.random.default_rng([SEED, 0, PIPELINES.index(pipeline), logn, prime])
    many = digit_shape(pipeline, logn)[0] > 1 if pipeline != "public" else False
    best, value = B.search(evaluate, classes, len(targets), rng, random_inputs(pipeline, field, classes), RESTARTS,
                           ROUNDS_ROWS if many else ROUNDS, CANDS_ROWS if many else CANDS, report)
    out, reached = {}, {}
    for i, (direction, k) in enumerate(targets):
        base = "%s/%d/p%d/%s/%d" % (pipeline, field.N, prime, direction, k)
        reached[base] = float(value[i])
        for name, as_name in stored(pipeline, direction).items():
            out[base + "/" + as_name] = best[name][i].astype(np.int32)
    return out, reached


def entries_of(arrays):
    """the fixture's index: the entry names without the array part, sorted"""
    return sorted({name.rsplit("/", 1)[0] for name in arrays})


def main():
    from concurrent.futures import ProcessPoolExecutor
    arrays = {}
    jobs = [(pipeline, logn, prime) for pipeline in PIPELINES for logn in (11, 10) for prime in (0, 1)]
    with ProcessPoolExecutor(8) as ex:
        for (pipeline, logn, prime), (out, reached) in zip(jobs, ex.map(find, *zip(*jobs))):
            arrays.update(out)
            P = B.PRIMES[prime]
            print(pipeline, 1 << logn, "prime", prime, " ".join("%s%d=%.2fP" % (k.split("/")[3], int(k.split("/")[4]), v / P)
                                                               for k, v in reached.items()), flush=True)
    for path in sorted({file_of(name) for name in arrays}):
        np.savez_compressed(path, **{k: v for k, v in arrays.items() if file_of(k) == path})
        print("wrote", path, os.path.getsize(path), "bytes")
    print(len(entries_of(arrays)), "entries")


if __name__ == "__main__":
    main()
