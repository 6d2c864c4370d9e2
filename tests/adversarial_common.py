"""Shared by tests/test_adversarial_cpu.py and tests/test_gpu_adversarial.py: cloud keys whose bootstrapping-key words are
CHOSEN, so that the production blind rotation multiplies a chosen accumulator by chosen key rows.

A blind rotation skips the mask words whose modulus switch is 0, so a row of `lin` with two or three non-zero mask words
runs two or three CMUX steps under the key entries BK_i of those words:

* one-step load (mask word i_a, abar = 1, bbar = 0): (X - 1) testvec = -2 mu X^0 in the body and 0 in the mask, whose
  decomposition is the single digit d0 = -2^(Bgbit-2) at coefficient 0 of row l (p = 1, j = 0).  Hence
  ACC = testvec + d0 BK_ia[row l]: any accumulator whose words are = testvec modulo |d0|;
* two-step load (mask word 0 with abar = 1, then mask word i_a with abar = N): BK_0 loads -2^(31-Bgbit) X^0 in the mask,
  whose rotated difference by X^N is +2^(32-Bgbit) X^0: the single digit +1 at coefficient 0 of row 0.  Hence
  ACC = that + BK_ia[row 0]: any accumulator at all;
* the step under test (mask word i_k, abar = a): ACC += BK_ik (.) decompose((X^a - 1) ACC), with the accumulator solved
  from the wanted digits (solve_accumulator) and BK_ik one of the key patterns.

Every other row of a loading BK_i meets zero digits only and holds random words.  exact_step is the reference of the
step under test in unreduced integers; build_set checks with it and with the oracle's decomposition that every case
is what it was meant to be."""
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

P0, P1 = 134111233, 134176769
CRT_EXACT_LIMIT = P0 * P1 // 100 * 36            # ntt_field.hpp
MU = 1 << 29

# name -> (N, l, Bgbit, n).  n (the LWE dimension, here the number of key entries) is one no other test module uses.
SETS = {
    "P128": (1024, 3, 7, 57), "P80": (1024, 2, 10, 58), "P2048": (2048, 3, 6, 59),
    "l4_Bg8": (1024, 4, 8, 60), "N2048_l6_Bg4": (2048, 6, 4, 61), "l8_Bg4": (1024, 8, 4, 62),
    "N2048_l2_Bg9": (2048, 2, 9, 63),
    # the frontier of every kernel form's admissible range (br_forms.hpp) and the digit-field edges:
    "l9_Bg3": (1024, 9, 3, 65),             # the 2-wave form only
    "l7_Bg4": (1024, 7, 4, 66),             # the last l of the 4-wave form (model: 3.95 of < 4), tables usable
    "l5_Bg5": (1024, 5, 5, 67),             # the last l of the 8-wave form (3.88), which takes it only without tables
    "l5_Bg6": (1024, 5, 6, 68),             # lowest digit field at bit 2: tables off by DIGIT_TAB_MIN_SHIFT, Bgbit <= 7
    "l1_Bg11": (1024, 1, 11, 69),           # l = 1 (one gadget row, no 8-wave form), the widest digits the CRT range takes
    "N2048_l7_Bg4": (2048, 7, 4, 70),       # the last l of the split form (3.98), table mode 1 excluded
    "N2048_l4_Bg6": (2048, 4, 6, 71),       # the largest l with the split form's eleven-table first step
    "N2048_l1_Bg10": (2048, 1, 10, 72),     # l = 1 at N = 2048, at the CRT magnitude 2^52
}
# the sets' seeds: the first seven keep the ones they were first checked with (their rank by name among themselves)
_SEED_RANK = {name: i for i, name in enumerate(sorted(list(SETS)[:7]) + list(SETS)[7:])}
KS_T, KS_BASEBIT = 8, 2
WIDE4, SPLIT, WAVE8, WAVE2 = range(4)
FORM_NAMES = ["4-wave", "split", "8-wave", "2-wave"]
FORM_COUNTERS = ["br_wide4_launches", "br_split_launches", "br_wave8_launches", "br_wave2_launches"]
TABLE_COUNTERS = ["br_tables0_launches", "br_tables1_launches", "br_tables2_launches"]


def crt_bound(N, l, Bgbit, k=1):
    """(k+1) l N (Bg/2) 2^31: what unsupported_reason compares with CRT_EXACT_LIMIT."""
    return (k + 1) * l * N * (1 << (Bgbit - 1)) * (1 << 31)


def w32(x):
    """int64 values -> their centred representatives modulo 2^32 (still int64)."""
    return ((np.asarray(x, dtype=np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def i32(x):
    return w32(x).astype(np.int32)


# ---- ring arithmetic from the definitions ---------------------------------------------------------------------------
def mul_xa(p, a):
    """X^a p modulo X^N + 1, a in [0, 2N)."""
    N = len(p)
    r = a % N
    out = np.roll(p, r)
    out[:r] = -out[:r]
    return -out if a >= N else out


def rot_diff(p, a):
    return w32(mul_xa(p, a) - p)


def sigma(p, a):
    """The ring automorphism X -> X^a (a odd)."""
    N = len(p)
    e = (a * np.arange(N)) % (2 * N)
    out = np.zeros_like(p)
    out[e % N] = np.where(e < N, p, -p)
    return out


def decomp_offset(l, Bgbit):
    return sum((1 << (Bgbit - 1)) << (32 - j * Bgbit) for j in range(1, l + 1)) & 0xFFFFFFFF


def decompose(p, l, Bgbit):
    """Gadget digits from the definition: offset, bit fields, - Bg/2 -> [l][N]."""
    u = (np.asarray(p, dtype=np.int64) + decomp_offset(l, Bgbit)) & 0xFFFFFFFF
    return np.stack([((u >> (32 - (j + 1) * Bgbit)) & ((1 << Bgbit) - 1)) - (1 << (Bgbit - 1)) for j in range(l)])


def recompose(digits, Bgbit):
    """The word whose digits are `digits` [l][N] and whose bits below the lowest digit field are zero."""
    l = digits.shape[0]
    return w32(sum(digits[j].astype(np.int64) << (32 - (j + 1) * Bgbit) for j in range(l)))


def solve_accumulator(D, a):
    """T with (X^a - 1) T = D modulo 2^32, for a = N (D even) or a odd (the words of D sum to an even number)."""
    N = len(D)
    D = w32(D)
    if a == N:
        assert not (D & 1).any(), "X^N - 1 = -2: the rotated difference must be even"
        T = w32(-(D // 2))
    else:
        assert a & 1
        D1 = sigma(D, pow(a, -1, 2 * N))
        S = int(D1[1:].sum())
        assert (S - int(D1[0])) % 2 == 0, "(X - 1) T has an even coefficient sum"
        T1 = np.empty(N, dtype=np.int64)
        T1[0] = (S - int(D1[0])) // 2
        T1[1:] = T1[0] - np.cumsum(D1[1:])
        T = w32(sigma(w32(T1), a))
    assert (rot_diff(T, a) == D).all()
    return T


def negacyclic_exact(d, key):
    c = np.convolve(d.astype(np.int64), key.astype(np.int64))
    out = c[:len(d)].copy()
    out[:len(d) - 1] -= c[len(d):]
    return out


def exact_step(acc, a, bk_i, l, Bgbit):
    """One CMUX step in integers: acc [2][N], bk_i [2l][2][N] -> (new accumulator words [2][N] int32, the digits
    [2l][N], the largest |coefficient| of the UNREDUCED sums over the 2 l rows)."""
    acc = np.asarray(acc, dtype=np.int64)
    dig = np.concatenate([decompose(rot_diff(acc[u], a), l, Bgbit) for u in range(2)])
    out, most = [], 0
    for w in range(2):
        s = np.zeros(acc.shape[1], dtype=np.int64)
        for q in range(2 * l):
            if dig[q].any():
                s += negacyclic_exact(dig[q], bk_i[q, w])
        most = max(most, int(np.abs(s).max()))
        out.append(i32(acc[w] + s))
    return np.stack(out), dig, most


# ---- the patterns -----------------------------------------------------------------------------------------------------
def spectral_signs(N, m):
    """+1 / -1 by the sign of Re psi^((2m+1) i), psi = exp(i pi / N): all the weight in transform bin m."""
    return np.where(np.cos(np.pi * ((2 * m + 1) * np.arange(N) % (2 * N)) / N) >= 0, 1, -1)


def spectral_bins(N):
    return [0, 1, N // 2 - 1, N - 1]


def digit_patterns(N, l, Bgbit, seed):
    """name -> digits [2l][N], every one -Bg/2 or Bg/2 - 1."""
    half = 1 << (Bgbit - 1)
    lo, hi = -half, half - 1
    rng = np.random.default_rng(seed)
    rows = np.arange(2 * l)[:, None]
    idx = np.arange(N)[None, :]
    pats = {"min": np.full((2 * l, N), lo), "max": np.full((2 * l, N), hi),
            "alt": np.where((rows + idx) & 1, hi, lo), "rnd": np.where(rng.integers(0, 2, (2 * l, N)), hi, lo)}
    for m in spectral_bins(N):
        pats["bin%d" % m] = np.broadcast_to(np.where(spectral_signs(N, m) > 0, hi, lo), (2 * l, N)).copy()
    return {k: v.astype(np.int64) for k, v in pats.items()}


def key_patterns(N, l, seed):
    """name -> BK_i [2l][2][N] int32."""
    lo, hi = -(1 << 31), (1 << 31) - 1
    rng = np.random.default_rng(seed)
    shape = (2 * l, 2, N)
    rows = np.arange(2 * l)[:, None, None]
    idx = np.arange(N)[None, None, :]
    one_sign = np.full(shape, lo)
    one_sign[:, :, 0] = hi
    pats = {"lo": np.full(shape, lo), "hi": np.full(shape, hi), "one_sign": one_sign,
            "alt": np.where((rows + idx) & 1, hi, lo) + np.zeros(shape, dtype=np.int64),
            "rnd": np.where(rng.integers(0, 2, shape), hi, lo)}
    for m in spectral_bins(N):
        pats["bin%d" % m] = np.broadcast_to(np.where(spectral_signs(N, m) > 0, hi, lo), shape).copy()
    return {k: v.astype(np.int32) for k, v in pats.items()}


def realisable(dig, a, l, Bgbit):
    """The nearest digits some accumulator can give under rotation a.  Only gadgets that use all 32 bits are touched:
    X^N - 1 = -2 makes every word even (lowest digits Bg/2 - 1 become Bg/2 - 2), and for odd a the words sum to an even
    number (the lowest digit of the last coefficient of the body changes sides if need be)."""
    dig = dig.copy()
    if l * Bgbit < 32:
        return dig
    if a == len(dig[0]):
        for u in range(2):
            dig[u * l + l - 1] -= dig[u * l + l - 1] & 1
    else:
        half = 1 << (Bgbit - 1)
        for u in range(2):
            if int(dig[u * l + l - 1].sum()) & 1:
                dig[u * l + l - 1, -1] = -half if dig[u * l + l - 1, -1] == half - 1 else half - 1
    return dig


def tie_words(N, l, Bgbit, kind, seed):
    """Rotated differences [2][N] placed on the decisions of the decomposition.  "trunc": 2^(32 - l Bgbit) m + {-1, 0, +1},
    the step of the lowest digit (a rounding decomposition moves the digit at - 1).  "field": words whose offset sum is
    on a boundary of digit field j, + {-1, 0, +1}.  The last word is moved by one where the sum would be odd."""
    rng = np.random.default_rng(seed)
    g = 1 << (32 - l * Bgbit)
    delta = (np.arange(N) % 3) - 1
    out = []
    for u in range(2):
        if kind == "trunc":
            w = g * rng.integers(0, (1 << 32) // g, N) + delta
        else:
            j = (np.arange(N) + u) % l
            w = (rng.integers(0, 1 << 31, N) >> (32 - (j + 1) * Bgbit) << (32 - (j + 1) * Bgbit)) - decomp_offset(l, Bgbit) + delta
        w = w32(w)
        if int(w.sum()) & 1:
            w[-1] = w32(w[-1] + 1)
        out.append(w)
    return np.stack(out)


# ---- one crafted key and its cases ------------------------------------------------------------------------------------
class CraftedSet:
    """bk [n][2l][2][N], ksk, and the cases: dicts of name, lin row [n + 1], bara [n], target accumulator, wanted
    digits, key entry, rotation, expected accumulator (integer reference) and its largest exact coefficient."""


def _rand_words(rng, shape):
    return rng.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32)


def build_set(name, key_variant=0, with_cases=True):
    """The crafted key of parameter set `name`.  key_variant > 0: other random fillers, sign patterns and key-switching
    words (the multi-key test's second and third key), same case list."""
    N, l, Bgbit, n = SETS[name]
    half = 1 << (Bgbit - 1)
    assert Bgbit >= 2, "the loads need the digit 2^(Bgbit-2)"
    seed = 1000 * _SEED_RANK[name] + key_variant
    rng = np.random.default_rng(seed)
    cs = CraftedSet()
    cs.name, cs.N, cs.l, cs.Bgbit, cs.n = name, N, l, Bgbit, n
    cs.params_tuple = (n, N, 1, l, Bgbit, KS_T, KS_BASEBIT, 2.0 ** -15, 2.0 ** -25, 0.012467)
    bk = _rand_words(rng, (n, 2 * l, 2, N))
    tv = np.stack([np.zeros(N, dtype=np.int64), np.full(N, MU, dtype=np.int64)])
    unit = 1 << (32 - (N.bit_length()))                       # the torus word whose modulus switch to 2N is 1
    rotations = [1, N - 1, N, N + 1, 2 * N - 1]

    # entry 0: the first half of the two-step load
    TA = np.zeros((2, N), dtype=np.int64)
    TA[0, 0] = -(1 << (31 - Bgbit))
    d0 = 1 << (Bgbit - 2)                                     # |d0|
    bk[0, l] = i32(-(w32(TA - tv) >> (Bgbit - 2)))
    assert (w32(TA - tv) % d0 == 0).all()

    dpats = digit_patterns(N, l, Bgbit, seed + 1)
    kpats = key_patterns(N, l, seed + 2)
    knames = list(kpats)
    loaders = []                                              # (label, target accumulator, wanted digits or None, rotation)
    for pname, dig in dpats.items():
        for a in rotations:
            dig_a = realisable(dig, a, l, Bgbit)
            T = np.stack([solve_accumulator(recompose(dig_a[u * l:(u + 1) * l], Bgbit), a) for u in range(2)])
            loaders.append(("%s/a%d" % (pname, a), T, dig_a, a))
    for kind in ("trunc", "field"):
        D = tie_words(N, l, Bgbit, kind, seed + 3)
        loaders.append(("tie_%s/a1" % kind, np.stack([solve_accumulator(D[u], 1) for u in range(2)]), None, 1))
    first_key = 1 + len(loaders)
    assert first_key + len(knames) <= n, "SETS: n too small for the case list"
    for q, kn in enumerate(knames):
        bk[first_key + q] = kpats[kn]

    cs.cases = []
    for q, (label, T, dig, a) in enumerate(loaders):
        ia = 1 + q
        one_step = bool((w32(T - tv) % d0 == 0).all())
        if one_step:
            bk[ia, l] = i32(-(w32(T - tv) >> (Bgbit - 2)))
        else:
            bk[ia, 0] = i32(T - TA)
        if label.startswith("tie"):
            keys = ["rnd", "hi"]
        elif a == N:
            keys = knames
        else:
            keys = [knames[q % len(knames)]]
        for kn in keys:
            ik = first_key + knames.index(kn)
            bara = np.zeros(n, dtype=np.int64)
            bara[ia], bara[ik] = (1 if one_step else N), a
            if not one_step:
                bara[0] = 1
            lin = np.zeros(n + 1, dtype=np.int64)
            lin[:n] = bara * unit
            cs.cases.append(dict(name="%s x %s" % (label, kn), lin=i32(lin), bara=bara.astype(np.int32), target=i32(T),
                                 digits=dig, ia=ia, ik=ik, a=a, one_step=one_step, key=kn, pattern=label.split("/")[0]))
    cs.bk = np.ascontiguousarray(bk)
    # key-switching key: extreme words of a seeded sign pattern (arithmetic modulo 2^32, but no generated key holds them)
    ksk_words = N * KS_T * (1 << KS_BASEBIT) * (n + 1)
    cs.ksk = np.where(rng.integers(0, 2, ksk_words), (1 << 31) - 1, -(1 << 31)).astype(np.int32)
    cs.lin = np.stack([c["lin"] for c in cs.cases])
    if with_cases:
        _reference(cs)
    return cs


def _reference(cs):
    """Fills expected / digits_seen / most of every case with the integer reference, and checks the construction."""
    l, Bgbit = cs.l, cs.Bgbit

    def one(c):
        acc, dig, most = exact_step(c["target"], c["a"], cs.bk[c["ik"]], l, Bgbit)
        return acc, dig, most
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(one, cs.cases))
    for c, (acc, dig, most) in zip(cs.cases, res):
        c["expected"], c["digits_seen"], c["most"] = acc, dig, most
        if c["digits"] is not None:
            assert (dig == c["digits"]).all(), "%s %s: the loaded accumulator does not give the intended digits" % (cs.name, c["name"])


def reach_cases(cs):
    """(the case whose digits are all -Bg/2 against the constant key word -2^31, the case with digits Bg/2 - 1 against
    2^31 - 1), both under rotation N."""
    by = {c["name"]: c for c in cs.cases}
    return by["min/a%d x lo" % cs.N], by["max/a%d x hi" % cs.N]


# ---- the file and the oracle twin -------------------------------------------------------------------------------------
def cloud_key_bytes(params_tuple, bk, ksk):
    """The container of peba1_amd/csrc/io.cpp: header {"TFHP", version 1, kind 2 (cloud), 0, payload bytes}, the parameter
    record {n, N, k, l, Bgbit, ks_t, ks_basebit, pad; ks_stdev, bk_stdev, max_stdev}, bk, ksk; little endian."""
    n, N, k, l, Bgbit, ks_t, ks_basebit, ks_stdev, bk_stdev, max_stdev = params_tuple
    rec = struct.pack("<8i3d", n, N, k, l, Bgbit, ks_t, ks_basebit, 0, ks_stdev, bk_stdev, max_stdev)
    bk = np.ascontiguousarray(bk, dtype="<i4").reshape(-1)
    ksk = np.ascontiguousarray(ksk, dtype="<i4").reshape(-1)
    payload = len(rec) + 4 * (bk.size + ksk.size)
    return b"TFHP" + struct.pack("<3IQ", 1, 2, 0, payload), rec, bk, ksk


def write_cloud_key(path, params_tuple, bk, ksk):
    hdr, rec, bk, ksk = cloud_key_bytes(params_tuple, bk, ksk)
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(rec)
        bk.tofile(f)
        ksk.tofile(f)


def oracle_twin(oracle, cs):
    """An oracle keyset with the crafted words written over its own.  Only the schoolbook evaluator (use_ntt = False) is
    valid afterwards: the transformed images still belong to the generated key."""
    n, N, k, l, Bgbit = cs.params_tuple[:5]
    oks = oracle.KeySet(oracle.custom_params(n=n, N=N, l=l, Bgbit=Bgbit, ks_t=KS_T, ks_basebit=KS_BASEBIT), 1)
    assert oks.bk().size == cs.bk.size and oks.ksk().size == cs.ksk.size
    oks.bk()[:] = cs.bk.reshape(-1)
    oks.ksk()[:] = cs.ksk
    return oks


def oracle_accumulators(oks, cs, threads=16):
    """The oracle's schoolbook blind rotation of every case -> [cases][2 N]."""
    with ThreadPoolExecutor(threads) as ex:
        return np.stack(list(ex.map(lambda c: oks.blind_rotate(c["bara"], 0, use_ntt=False), cs.cases)))


# ---- which kernel form a launch runs: launch_plan.hpp plan_br restated over tfhe_hip_test_form_admissible -------------
def predicted_form(ok, N, l, Bgbit, count, cu_count, br_variant, br_digit_table, br8_max):
    if br_variant == 4 and N == 1024:
        form = WAVE2
    elif br_variant == 2 or N == 2048:
        form = SPLIT
    elif br8_max > 0 and count <= min(br8_max, cu_count) and l >= 2:
        form = WAVE8
    else:
        form = WIDE4
    tables = br_digit_table
    if not ok(form, N, l, Bgbit, tables):
        for f in (form, WIDE4, SPLIT, WAVE2, WAVE8):
            if f == WAVE8 and count > cu_count:
                continue
            hit = [t for t in (tables, 2, 0) if ok(f, N, l, Bgbit, t)]
            if hit:
                return f, hit[0]
        return None
    return form, tables


def tables_run(form, l, Bgbit, tables):
    """br_forms.hpp br_tables_run restated: the digit-table mode a launch planned with `tables` really runs, which is what
    the br_tables*_launches counters count.  The launchers (kernels.hip digit_table_usable) multiply where the digits do
    not index the LDS tables: wider than 7 bits, or a lowest field below bit 3; the 2-wave form has no tables."""
    return 0 if form == WAVE2 or Bgbit > 7 or 32 - l * Bgbit < 3 else tables
