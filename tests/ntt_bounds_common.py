"""Shared by tests/test_ntt_bounds_cpu.py, tests/golden/make_ntt_bounds_inputs.py and tests/test_gpu_ntt_bounds.py: the signed
lazy radix-4 wave NTT of peba1_amd/csrc/ntt_wave.hpp emulated on numpy int64 arrays, a batch of transforms at a time, with
every 32-bit intermediate checked against [-2^31, 2^31) and every 64-bit sum against 2^63; the interval recurrences of the
magnitudes, step by step; and the kernels' pipelines from what a kernel is given to what enters the CRT.

The scalar statement of the same butterflies is tools/ntt_model_r4.py (Python integers, one element at a time);
tests/test_ntt_bounds_cpu.py holds this file to it element by element and step by step.  Shares no code with the library.

Order of the values: the model's -- natural order into the forward transform, bit-reversed out of it, and back.  A word of
a key image multiplies the forward output at the same index, so the order never matters to a pipeline."""
import os
import sys

import numpy as np

PRIMES = (134111233, 134176769)                    # peba1_amd/csrc/ntt_field.hpp NTT_P
GENERATORS = (10, 3)                               # NTT_GEN
R = 1 << 32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
CRT_EXACT_LIMIT = PRIMES[0] * PRIMES[1] // 100 * 36
TOOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tools")


def scalar_model():
    """tools/ntt_model_r4.py as a module"""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import ntt_model_r4
    return ntt_model_r4


class BoundsViolation(AssertionError):
    """an intermediate of the emulated arithmetic left int32, or a 64-bit sum left int64"""


def chk32(v, what):
    if v.size and (v.min() < I32_MIN or v.max() > I32_MAX):
        raise BoundsViolation("%s leaves int32: [%d, %d]" % (what, v.min(), v.max()))
    return v


def sum64(what, *terms):
    """the int64 sum of the terms, checked against 2^63 (in float64 on the magnitudes, with 2^40 to spare for its rounding)"""
    mag = sum(np.abs(t).astype(np.float64) for t in terms)
    if mag.size and mag.max() >= 2.0 ** 63 - 2.0 ** 40:
        raise BoundsViolation("%s leaves int64: %.4g" % (what, mag.max()))
    out = terms[0]
    for t in terms[1:]:
        out = out + t
    return out


def max_coef(N):
    """ring_public.hpp public_max_coef: the largest power of two T with N T 2^31 < CRT_EXACT_LIMIT"""
    T = 1
    while N * (2 * T) * 2 ** 31 < CRT_EXACT_LIMIT:
        T *= 2
    return T


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


class Field:
    """one prime and one ring size: the plain twiddle tables as engine.cpp make_twiddles makes them, per step the
    Montgomery-form twiddles of every block, and the constants of the reductions"""
    _made = {}

    @classmethod
    def get(cls, prime, logn):
        if (prime, logn) not in cls._made:
            cls._made[prime, logn] = cls(prime, logn)
        return cls._made[prime, logn]

    def __init__(self, prime, logn):
        P = self.P = PRIMES[prime]
        self.prime, self.logn, self.N = prime, logn, 1 << logn
        N = self.N
        self.pinv = (-pow(P, -1, R)) % R
        self.rmod = R % P
        self.ninv = pow(N, P - 2, P)
        self.scale = self.ninv * R % P                           # engine.cpp: the image scale N^-1 R
        psi = pow(GENERATORS[prime], (P - 1) // (2 * N), P)
        assert pow(psi, N, P) == P - 1
        ipsi = pow(psi, P - 2, P)
        self.W, self.IW = [0] * N, [0] * N
        a = b = 1
        for i in range(N):
            j = bitrev(i, logn)
            self.W[j], self.IW[j] = a, b
            a, b = a * psi % P, b * ipsi % P
        rb = logn - 6
        self.passes = [list(range(0, rb)), list(range(rb, 2 * rb)), list(range(2 * rb, logn))]
        self.fwd_steps, self.inv_steps = [], []
        for p in self.passes:
            i = 0
            while i < len(p):
                self.fwd_steps.append(tuple(p[i:i + 2]))
                i += 2
        for p in reversed(self.passes):
            i = len(p)
            while i > 0:
                self.inv_steps.append(tuple(p[max(i - 2, 0):i]))
                i -= 2
        self.fwd_tw = [self._tw(self.W, st, False) for st in self.fwd_steps]
        self.inv_tw = [self._tw(self.IW, st, True) for st in self.inv_steps]

    def _tw(self, W, step, inverse):
        P, s = self.P, step[0]
        m = lambda v: v * R % P                                   # noqa: E731
        col = lambda vals: np.array(vals, dtype=np.int64).reshape(-1, 1)   # noqa: E731
        if len(step) == 1:
            return (col([m(W[(1 << s) + t]) for t in range(1 << s)]),)
        w1 = [W[(1 << s) + t] for t in range(1 << s)]
        w2 = [W[(2 << s) + 2 * t] for t in range(1 << s)]
        w3 = [W[(2 << s) + 2 * t + 1] for t in range(1 << s)]
        # the quads of make_twiddles: {w2, w3, w1 w2, P - w1 w3}
        return (col([m(v) for v in w1]), col([m(v) for v in w2]), col([m(v) for v in w3]),
                col([m(a * b % P) for a, b in zip(w1, w2)]), col([m((P - a * b % P) % P) for a, b in zip(w1, w3)]),
                col([m(a * b % P) for a, b in zip(w1, w3)]))

    # ---- the reductions ----
    def redc(self, T, what="redc"):
        """ntt_wave.hpp mont_redc on an int64 array (|T| + 2^31 P must stay inside int64: checked)"""
        if T.size and np.abs(T).astype(np.float64).max() >= 2.0 ** 63 - 2.0 ** 59:
            raise BoundsViolation("%s: the 64-bit operand leaves int64" % what)
        m = ((T.astype(np.uint64) & np.uint64(0xFFFFFFFF)) * np.uint64(self.pinv)) & np.uint64(0xFFFFFFFF)
        m = m.astype(np.int64)
        m = m - ((m >> 31) << 32)
        U = T + m * self.P
        assert not (U & 0xFFFFFFFF).any()
        return chk32(U >> 32, what)

    def mont_mul(self, b, w, what="mont_mul"):
        return self.redc(chk32(b, what) * w, what)

    # ---- the transforms ----
    def forward(self, x, track=None, first=0, kernel_form=True):
        """x int64 [..., N] -> the lazy forward transform, every intermediate checked; track gets max |x| per transform
        after every step.  first: the index of the first step to run (1: the caller made the first step's outputs).
        kernel_form: S' = redc(x1 w3 + x3 (P - w1 w3)), the kernel's quads; False: redc(x1 w3 - x3 w1 w3), as the scalar
        model writes it -- the same residue, now and then another representative of it (the two operands differ by x3 P)"""
        x = chk32(np.array(x, dtype=np.int64), "forward input")
        lead = x.shape[:-1]
        for k, (step, tw) in enumerate(zip(self.fwd_steps, self.fwd_tw)):
            if k < first:
                continue
            s = step[0]
            if len(step) == 1:
                v = x.reshape(lead + (1 << s, 2, -1))
                a, b = v[..., 0, :], v[..., 1, :]
                r = self.mont_mul(b, tw[0], "forward radix-2 product")
                x = np.stack([chk32(a + r, "a + t"), chk32(a - r, "a - t")], axis=-2).reshape(lead + (-1,))
            else:
                v = x.reshape(lead + (1 << s, 4, -1))
                x0, x1, x2, x3 = v[..., 0, :], v[..., 1, :], v[..., 2, :], v[..., 3, :]
                m1, m2, m3, m12, m13n, m13 = tw
                A = self.mont_mul(x2, m1, "A")
                S = self.redc(sum64("x1 w2 + x3 w1w2", x1 * m2, x3 * m12), "S")
                T = self.redc(sum64("x1 w3 + x3 (P - w1w3)", x1 * m3, x3 * m13n if kernel_form else -(x3 * m13)), "S'")
                u, w = chk32(x0 + A, "x0 + A"), chk32(x0 - A, "x0 - A")
                x = np.stack([chk32(u + S, "u + S"), chk32(u - S, "u - S"), chk32(w + T, "v + S'"), chk32(w - T, "v - S'")],
                             axis=-2).reshape(lead + (-1,))
            if track is not None:
                track.append(np.abs(x).max(axis=-1))
        return x

    def inverse(self, x, renorm, track=None):
        """the unscaled lazy inverse transform; renorm[k]: step k renormalises its plain sums"""
        x = chk32(np.array(x, dtype=np.int64), "inverse input")
        lead = x.shape[:-1]
        for k, (step, tw) in enumerate(zip(self.inv_steps, self.inv_tw)):
            s = step[0]
            if len(step) == 1:
                v = x.reshape(lead + (1 << s, 2, -1))
                a, b = v[..., 0, :], v[..., 1, :]
                sm = chk32(a + b, "a + b")
                y0 = self.mont_mul(sm, self.rmod, "renormalised a + b") if renorm[k] else sm
                y1 = self.mont_mul(chk32(a - b, "a - b"), tw[0], "(a - b) w")
                x = np.stack([y0, y1], axis=-2).reshape(lead + (-1,))
            else:
                v = x.reshape(lead + (1 << s, 4, -1))
                x0, x1, x2, x3 = v[..., 0, :], v[..., 1, :], v[..., 2, :], v[..., 3, :]
                m1, m2, m3, m12, m13n = tw[:5]
                s0, s1 = chk32(x0 + x1, "s0"), chk32(x2 + x3, "s1")
                d0, d1 = chk32(x0 - x1, "d0"), chk32(x2 - x3, "d1")
                y0 = chk32(s0 + s1, "s0 + s1")
                if renorm[k]:
                    y0 = self.mont_mul(y0, self.rmod, "renormalised s0 + s1")
                y2 = self.mont_mul(chk32(s0 - s1, "s0 - s1"), m1, "(s0 - s1) w1")
                y1 = self.redc(sum64("d0 w2 + d1 w3", d0 * m2, d1 * m3), "y1")
                y3 = self.redc(sum64("d0 w1w2 + d1 (P - w1w3)", d0 * m12, d1 * m13n), "y3")
                x = np.stack([y0, y1, y2, y3], axis=-2).reshape(lead + (-1,))
            if track is not None:
                track.append(np.abs(x).max(axis=-1))
        return x

    # ---- images and the key words that have a given image ----
    def image(self, words):
        """the canonical, scaled image of polynomials of signed words, as bk_transform_kernel and public_image_kernel leave
        it (the word reduced below P first; for |word| <= 2^11 that changes nothing)"""
        w = np.asarray(words, dtype=np.int64)
        x = self.forward(np.fmod(w, self.P))
        return (x % self.P) * self.scale % self.P

    def words_of_image(self, img):
        """the polynomial with 0 <= word < P whose image modulo this prime is img (any canonical img has one)"""
        unscaled = np.asarray(img, dtype=np.int64) * pow(self.scale, self.P - 2, self.P) % self.P
        plan = Plan.python(self.logn, 4.0)
        return (self.inverse(unscaled, plan.renorm) % self.P) * self.ninv % self.P


# ---- the interval recurrences, step by step (tools/ntt_model_r4.py fwd_bound / inv_schedule; P the larger prime) ----
Q = PRIMES[1] / R


def fwd_bounds(field, b_in, first=0):
    """|value| / P after every forward step from inputs |x| <= b_in P (units of the LARGER prime, as the library's)"""
    b, out = b_in, []
    for k, step in enumerate(field.fwd_steps):
        if k >= first:
            b = b + (b * Q + 0.5) if len(step) == 1 else b + (b * Q + 0.5) + (2 * b * Q + 0.5)
        out.append(b)
    return out


def inv_bounds(field, b_in, renorm):
    """|value| / P after every inverse step under the given renormalisation flags"""
    b, out = b_in, []
    for step, r in zip(field.inv_steps, renorm):
        fan = 2 * len(step)
        small = fan * b * Q + 0.5
        b = small if r else max(small, fan * b)
        out.append(b)
    return out


class Plan:
    """an inverse plan: nsteps, fan, renorm, out_bound"""

    def __init__(self, nsteps, fan, renorm, out_bound):
        self.nsteps, self.fan, self.renorm, self.out_bound = nsteps, list(fan), [bool(r) for r in renorm], out_bound

    @classmethod
    def python(cls, logn, b_in):
        """inv_schedule of the scalar model's rule, restated (units of the larger prime)"""
        f = Field.get(1, logn)
        limit = (2 ** 31 - 1) / PRIMES[1]
        b, renorm = b_in, []
        fans = [2 * len(s) for s in f.inv_steps]
        for k, fan in enumerate(fans):
            small, big = fan * b * Q + 0.5, fan * b
            assert big <= limit
            last = k == len(fans) - 1
            r = last or fans[k + 1] * max(big, small) > limit
            renorm.append(r)
            b = small if r else max(big, small)
        return cls(len(fans), fans, renorm, b)

    @classmethod
    def library(cls, L, logn):
        """make_inv_plan(logn) through tfhe_hip_test_ntt_bounds"""
        import ctypes as C
        fwd, plan, out = (C.c_double * 2)(), (C.c_int32 * 25)(), C.c_double()
        assert L.tfhe_hip_test_ntt_bounds(logn, 1.0, fwd, plan, C.byref(out)) == 0
        n = plan[0]
        return cls(n, plan[1:1 + n], plan[13:13 + n], out.value)


# the flags of make_inv_plan (ntt_wave.hpp), for the files that must not load the library to know them: the GPU-free
# generator of the fixture.  tests/test_ntt_bounds_cpu.py holds them to the library's.
RENORM = {10: (True, False, True, False, True), 11: (True, False, True, False, True, False, True)}


# ---- the pipelines: from what a kernel is given to what enters the CRT ----
def pipeline_public(field, words, q):
    """ring_public.hip public_kernel for one prime, with the gallery polynomial's own transform (public_image_kernel):
    word -> mont_mul(word, R mod P) -> forward -> one product with the canonical image word of q -> redc -> inverse.
    words, q: int64 [B][N].  -> {"fwd": [steps][B], "inv": [steps][B], "img": [steps][B], "into_inverse": [B]}, |values|"""
    t_img, t_fwd, t_inv = [], [], []
    x = field.forward(np.asarray(q, dtype=np.int64), t_img)
    img = (x % field.P) * field.scale % field.P
    x = field.mont_mul(np.asarray(words, dtype=np.int64), field.rmod, "the word's reduction")
    x = field.forward(x, t_fwd)
    y = field.redc(x * img, "the product's reduction")
    field.inverse(y, RENORM[field.logn], t_inv)
    return {"fwd": t_fwd, "inv": t_inv, "img": t_img, "into_inverse": np.abs(y).max(axis=-1)}


def pipeline_digits(field, digits, img):
    """pack.hip / cmux.hip / kernels.hip negacyclic_kernel for one prime and one output polynomial: per row one forward
    transform of the digit polynomial, the products with the row's canonical image words summed in 64 bits, ONE reduction,
    one inverse.  digits, img: int64 [B][rows][N]"""
    t_fwd, t_inv = [], []
    x = field.forward(np.asarray(digits, dtype=np.int64), t_fwd)
    img = np.asarray(img, dtype=np.int64)
    acc = sum64("the row sum", *[x[:, r] * img[:, r] for r in range(x.shape[1])])
    y = field.redc(acc, "the row sum's reduction")
    field.inverse(y, RENORM[field.logn], t_inv)
    return {"fwd": [t.max(axis=-1) for t in t_fwd], "inv": t_inv, "into_inverse": np.abs(y).max(axis=-1)}


def table_first_step(field, width):
    """ntt_wave.hpp forward_digits<TABLE>: the first radix-4 step of a transform of `width`-bit digits from the digit
    table.  -> (the table rows [5][2^width] as build_digit_table fills them, for digit fields 0 .. 2^width - 1,
    a function digits [B][N] -> the step's outputs)"""
    fields = 1 << width
    d = np.arange(fields, dtype=np.int64)
    d = np.where(d < fields // 2, d, d - fields)
    m1, m2, m3, m12, m13n = [int(t[0, 0]) for t in field.fwd_tw[0][:5]]
    rows = np.stack([field.mont_mul(d, w, "table entry") for w in (m1, m2, m12, m3, m13n)])

    def step(digits):
        x = np.asarray(digits, dtype=np.int64)
        v = x.reshape(x.shape[:-1] + (4, -1))
        f = v & (fields - 1)
        x0 = v[..., 0, :]
        A = rows[0][f[..., 2, :]]
        S = chk32(rows[1][f[..., 1, :]] + rows[2][f[..., 3, :]], "table S")
        T = chk32(rows[3][f[..., 1, :]] + rows[4][f[..., 3, :]], "table S'")
        u, w = chk32(x0 + A, "x0 + A"), chk32(x0 - A, "x0 - A")
        return np.stack([chk32(u + S, "u + S"), chk32(u - S, "u - S"), chk32(w + T, "v + S'"), chk32(w - T, "v - S'")],
                        axis=-2).reshape(x.shape)
    return rows, step


# ---- the seeded search ----
def uniform_draw(cls, rng, size):
    """uniform over the admitted set of one array: the integers of [lo, hi], or, lo None, the values of the palette"""
    shape, ext, lo, hi = cls
    if lo is None:
        return np.asarray(ext, dtype=np.int64)[rng.integers(0, len(ext), size=size)]
    return rng.integers(lo, hi + 1, size=size)


def uniform_inputs(classes, rng, count):
    """`count` inputs drawn uniformly from the admitted set of every array"""
    return {name: uniform_draw(cls, rng, (count,) + cls[0]) for name, cls in sorted(classes.items())}


def search(evaluate, classes, ntargets, rng, first, restarts, rounds, cands, report=None):
    """Random restarts, then greedy coordinate moves, for all targets at once.
    evaluate(inputs: {name: int64 [B][...]}) -> float [B][ntargets], larger is worse for the kernel.
    classes: {name: (shape of one input, extremes (1-d int64), lo, hi)}: a coordinate moves among the extremes and the
    uniform values of [lo, hi]; lo None: the extremes are a palette and the array takes no other value.
    first: restarts the caller drew (uniform_inputs: the random inputs the searched ones are compared with); `restarts` more
    are drawn here, on the extremes.  report: a dict that receives per target the value of the best restart ("restart") and
    the number of accepted greedy moves ("moves").
    -> (inputs {name: int64 [ntargets][...]}, value [ntargets]): per target its worst input."""
    names = sorted(classes)

    def draw(name, size, uniform_share):
        ext = classes[name][1]
        pick = np.asarray(ext, dtype=np.int64)[rng.integers(0, len(ext), size=size)]
        return np.where(rng.random(size) < uniform_share, uniform_draw(classes[name], rng, size), pick)

    pool = {name: np.concatenate([first[name], draw(name, (restarts,) + classes[name][0], 0.05)]) for name in names}
    val = evaluate(pool)
    best_of = val.argmax(axis=0)
    cur = {name: pool[name][best_of].copy() for name in names}
    cur_val = val[best_of, np.arange(ntargets)]
    restart_val, moves = cur_val.copy(), np.zeros(ntargets, dtype=np.int64)
    # greedy: per round and target `cands` candidates, each the current input with a few coordinates moved
    for _ in range(rounds):
        cand = {name: np.repeat(cur[name], cands, axis=0) for name in names}
        for name in names:
            flat = cand[name].reshape(ntargets * cands, -1)
            nmove = 1 << rng.integers(0, 4, size=flat.shape[0])
            for i in range(flat.shape[0]):
                at = rng.integers(0, flat.shape[1], size=nmove[i])
                flat[i, at] = draw(name, nmove[i], 0.1)
        val = evaluate(cand).reshape(ntargets, cands, ntargets)
        own = val[np.arange(ntargets), :, np.arange(ntargets)]              # [target][cand]: the target's own column
        pick = own.argmax(axis=1)
        better = own[np.arange(ntargets), pick] > cur_val
        for name in names:
            c = cand[name].reshape((ntargets, cands) + cur[name].shape[1:])
            cur[name][better] = c[np.arange(ntargets), pick][better]
        cur_val = np.where(better, own[np.arange(ntargets), pick], cur_val)
        moves += better
    if report is not None:
        report["restart"], report["moves"] = restart_val, moves
    return cur, cur_val
