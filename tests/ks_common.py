"""Shared by tests/test_ks_sweep_cpu.py and tests/test_gpu_ks_sweep.py: the accepted key-switch decompositions, the key
switch stated from its definition in numpy, and the input rows both files run.

unsupported_reason (engine.cpp) lets a key upload for every (ks_t, ks_basebit) with ks_t >= 1, 1 <= ks_basebit <= 8 and
ks_t * ks_basebit <= 31: 81 pairs.  The oracle's orc_keyswitch and the kernels were written from one specification with
the same shift expressions; keyswitch_ref below is written from the definition instead -- a rounding division, the digits
of an integer in base 2^basebit, a sum of key rows -- and shares no expression with either."""
import numpy as np

N_RING = 1024
N_LWE = 10                                   # the sweep's LWE width: the decomposition is what is under test
GADGET = (3, 7)                              # (l, Bgbit) of every key of the sweep
STDEVS = (2.0 ** -15, 2.0 ** -25, 0.012467)  # ks_stdev, bk_stdev, max_stdev (the oracle's custom_params defaults)
GRID = [(t, bb) for bb in range(1, 13) for t in range(1, 31 // bb + 1)]      # every pair a parameter set can be made of
ROW_WIDTHS = (1, 2, 3, 4, 255, 256, 511, 512, 767, 768, 1023)
PERGATE, STRIP, INDEX = 0, 1, 2              # launch_plan.hpp KsForm, as tfhe_hip_test_ks_plan reports it
KS_COUNTERS = ["ks_pergate_launches", "ks_strip_launches", "ks_index_launches"]
KS_DEFAULTS = {"ks_target_blocks": 32768, "ks_max_splits": 48, "ks_split_ties": 0, "ks_tile": 16, "ks_index": 1}


def accepted_by_rule(t, bb):
    """unsupported_reason's key-switch line, restated"""
    return t >= 1 and 1 <= bb <= 8 and t * bb <= 31


def accepted_grid():
    return [(t, bb) for t, bb in GRID if accepted_by_rule(t, bb)]


def threads(n):
    """lanes of a key-switch workgroup: one per four words of the padded row, rounded up to a wave"""
    stride = (n + 1 + 3) & ~3
    return -(-(stride // 4) // 64) * 64


def custom_tuple(n, t, bb, N=N_RING):
    return (n, N, 1) + GADGET + (t, bb) + STDEVS


def keyswitch_ref(ksk, u, n, N, t, bb):
    """The key switch of the rows u [rows][N + 1] under ksk [N][t][2^bb][n + 1], from the definition:
    r_i = round(u_i / 2^(32 - t bb)) mod 2^(t bb), ties up; digit j of r_i in base 2^bb, most significant first;
    out = (0, u_N) - sum_{i, j} ksk[i][j][digit_j(r_i)] in wrapping 32-bit words."""
    base = 2 ** bb
    K = np.asarray(ksk).reshape(N * t, base, n + 1).view(np.uint32)          # (no copy: the widest keys hold 2.4 GB)
    u = np.asarray(u).astype(np.int64).reshape(-1, N + 1) % 2 ** 32
    step = 2 ** (32 - t * bb)
    r = ((2 * u[:, :N] + step) // (2 * step)) % base ** t                    # round half up, as integers
    weight = np.array([base ** (t - 1 - j) for j in range(t)], dtype=np.int64)
    digits = (r[:, :, None] // weight[None, None, :]) % base                 # [rows][N][t]
    which = np.arange(N * t)
    out = np.zeros((len(u), n + 1), dtype=np.int64)
    for row in range(len(u)):
        out[row] = -(K[which, digits[row].reshape(-1)].sum(axis=0, dtype=np.uint64) % 2 ** 32).astype(np.int64)
    out[:, n] += u[:, N]
    out %= 2 ** 32
    return (out - ((out >> 31) << 32)).astype(np.int32)


def word_of_digits(digits, t, bb):
    """the torus word whose rounded value has these t digits (most significant first) and whose bits below are zero"""
    base = 2 ** bb
    r = 0
    for d in digits:
        r = r * base + int(d)
    return r * 2 ** (32 - t * bb)


def inputs(N, t, bb, seed, rows=0):
    """The rows [N + 1] of the sweep, as int32, and their names.  Uniformly random rows (six, or as many as bring the total
    to `rows`); all zero; all 0xFFFFFFFF (the rounding offset wraps every coefficient to digits 0); every digit base - 1;
    for each position j a row with digit 1 at j only and a row with base - 1 at j only; three tie rows at
    (2m + 1) 2^(31 - t bb) + {-1, 0, +1}, where the rounding carries into the lowest digit or does not."""
    base = 2 ** bb
    rng = np.random.default_rng(seed)
    named = [("zero", np.zeros(N + 1, dtype=np.int64)), ("ones", np.full(N + 1, 0xFFFFFFFF, dtype=np.int64)),
             ("top digits", np.full(N + 1, word_of_digits([base - 1] * t, t, bb), dtype=np.int64))]
    for j in range(t):
        for d in sorted({1, base - 1}):
            named.append(("digit %d at %d" % (d, j), np.full(N + 1, word_of_digits([d if q == j else 0 for q in range(t)], t, bb),
                                                             dtype=np.int64)))
    half = 2 ** (31 - t * bb)
    for shift in range(3):
        m = rng.integers(0, 2 ** 31 // half, N + 1)
        named.append(("tie %d" % shift, (2 * m + 1) * half + (np.arange(N + 1) + shift) % 3 - 1))
    nrandom = max(6, rows - len(named))
    rnd = [("random %d" % i, rng.integers(0, 2 ** 32, N + 1)) for i in range(nrandom)]
    named = rnd + named
    words = np.stack([w for _, w in named]) % 2 ** 32
    return (words - ((words >> 31) << 32)).astype(np.int32), [name for name, _ in named]


def check_inputs(u, names, N, t, bb):
    """The rows are what their names say, by the definition of the digits: checked where they are used."""
    base, step = 2 ** bb, 2 ** (32 - t * bb)
    w = u.astype(np.int64) % 2 ** 32
    r = ((2 * w + step) // (2 * step)) % base ** t
    by = {name: r[i] for i, name in enumerate(names)}
    assert (by["zero"] == 0).all() and (by["ones"] == 0).all() and (by["top digits"] == base ** t - 1).all()
    for j in range(t):
        assert (by["digit 1 at %d" % j] == base ** (t - 1 - j)).all()
        assert (by["digit %d at %d" % (base - 1, j)] == (base - 1) * base ** (t - 1 - j)).all()
    for shift in range(3):
        x = w[names.index("tie %d" % shift)]
        frac = x % step                        # the bits below the lowest digit: half a step -1, +0, +1
        assert set(np.unique(frac - step // 2)) <= {-1, 0, 1} and len(np.unique(frac)) >= (2 if step > 2 else 1)


def ks_plan(lib, n, t, bb, tunings, cu_count, count, N=N_RING):
    """(tiled, tile, chunk, ranges of the first chunk, of the last chunk, partial bytes, form) from the library's planner"""
    import ctypes as C
    tn = dict(KS_DEFAULTS, **tunings)
    t5 = (C.c_int32 * 5)(*(tn[k] for k in KS_DEFAULTS))
    out = (C.c_int64 * 7)()
    assert lib.tfhe_hip_test_ks_plan_form(n, N, 1, t, bb, t5, cu_count, count, out) == 0
    return tuple(out)
