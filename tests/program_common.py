"""Shared by tests/test_plan_model_cpu.py and tests/test_gpu_recorded_programs.py: the gates as a literal table of
integers (include/tfhe_hip.h and tfhe's boot-gates restated; nothing here is read from the library), their truth tables,
the decrypt rule of the plain +-1/8 encoding that ties the two together, and the constant-folding rule of the recorder
written out from truth tables."""
import itertools

M32 = 0xFFFFFFFF
EIGHTH = 1 << 29
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# name -> (code, c0 in eighths, sa, sb, truth table [f(0,0), f(0,1), f(1,0), f(1,1)]): t = c0/8 + sa A + sb B
GATE2 = {
    "NAND": (0, 1, -1, -1, (1, 1, 1, 0)),
    "OR": (1, 1, 1, 1, (0, 1, 1, 1)),
    "AND": (2, -1, 1, 1, (0, 0, 0, 1)),
    "NOR": (3, -1, -1, -1, (1, 0, 0, 0)),
    "XOR": (4, 2, 2, 2, (0, 1, 1, 0)),
    "XNOR": (5, -2, -2, -2, (1, 0, 0, 1)),
    "ANDNY": (6, -1, -1, 1, (0, 1, 0, 0)),
    "ANDYN": (7, -1, 1, -1, (0, 0, 1, 0)),
    "ORNY": (8, 1, -1, 1, (1, 1, 0, 1)),
    "ORYN": (9, 1, 1, -1, (1, 0, 1, 1)),
}
GATE2_BY_CODE = {v[0]: (name,) + v[1:] for name, v in GATE2.items()}
# the two-input gates whose result does not depend on the operand order
SYMMETRIC = {"NAND", "OR", "AND", "NOR", "XOR", "XNOR"}
# MUX(a, b, c) = KS(Boot(prelude of MUX_FIRST on a, b) + Boot(prelude of MUX_SECOND on a, c) + MUX_ADD eighths)
MUX_FIRST, MUX_SECOND, MUX_ADD = "AND", "ANDNY", 1
# name -> (enum TfheHipGate3, s): t = s (+-A +- B +- C), bit i of the mask flips the sign of operand i
GATE3 = {"MAJ3": (0, 1), "XOR3": (1, -2), "XNOR3": (2, 2)}
GATE3_BY_CODE = {v[0]: name for name, v in GATE3.items()}
KIND_MUX, KIND_NOT, KIND_GATE3, KIND_LUT, KIND_LUTM, KIND_LIN = 16, 17, 32, 64, 65, 66


def w32(x):
    return x & M32


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def plain(bit):
    """The noiseless encoding of a bit: +1/8 or -1/8 of the torus."""
    return EIGHTH if bit else -EIGHTH


def boot_bit(t):
    """What a gate bootstrap decrypts to from phase t: 1 on the upper half of the torus (0, 1/2), else 0."""
    return 1 if 0 < s32(t) else 0


def gate3_coefs(name, mask):
    s = GATE3[name][1]
    return [-s if (mask >> i) & 1 else s for i in range(3)]


def gate3_truth(name, mask, a, b, c):
    a, b, c = a ^ (mask & 1), b ^ ((mask >> 1) & 1), c ^ ((mask >> 2) & 1)
    if name == "MAJ3":
        return 1 if a + b + c >= 2 else 0
    return (a ^ b ^ c) if name == "XOR3" else 1 - (a ^ b ^ c)


def mux_truth(a, b, c):
    return b if a else c


def check_tables_against_truth():
    """The literal table decrypts, on the plain encoding, to the truth tables: every two-input gate, MUX as the sum of
    its two bootstraps, the three-input gates under every mask."""
    for name, (code, c8, sa, sb, tt) in GATE2.items():
        for a, b in itertools.product((0, 1), repeat=2):
            assert boot_bit(c8 * EIGHTH + sa * plain(a) + sb * plain(b)) == tt[2 * a + b], (name, a, b)
        assert (name in SYMMETRIC) == (tt[1] == tt[2]) == (sa == sb), name
    assert sorted(v[0] for v in GATE2.values()) == list(range(10))
    f, s = GATE2[MUX_FIRST], GATE2[MUX_SECOND]
    for a, b, c in itertools.product((0, 1), repeat=3):
        u1 = plain(boot_bit(f[1] * EIGHTH + f[2] * plain(a) + f[3] * plain(b)))
        u2 = plain(boot_bit(s[1] * EIGHTH + s[2] * plain(a) + s[3] * plain(c)))
        assert boot_bit(u1 + u2 + MUX_ADD * EIGHTH) == mux_truth(a, b, c), (a, b, c)
    assert [GATE3[n][1] for n in ("MAJ3", "XOR3", "XNOR3")] == [1, -2, 2]
    for name in GATE3:
        for mask in range(8):
            sa, sb, sc = gate3_coefs(name, mask)
            for a, b, c in itertools.product((0, 1), repeat=3):
                assert boot_bit(sa * plain(a) + sb * plain(b) + sc * plain(c)) == gate3_truth(name, mask, a, b, c), (name, mask)


# ---- constant folding ("fold_constants", include/tfhe_hip.h): a trivial sample is a public constant ---------------------
# A folded call gives ("const", bit), ("copy", operand index), ("not", operand index), ("gate", name, operand indices) or
# None (not folded: evaluated as recorded).  `consts`: per operand, 0 / 1 for a public constant, None for a ciphertext.
def fold_gate2(name, consts):
    ka, kb = consts
    if ka is None and kb is None:
        return None
    tt = GATE2[name][4]
    x = 1 if ka is not None else 0                      # the operand that is not (known to be) constant
    if ka is not None and kb is not None:
        return ("const", tt[2 * ka + kb])
    f = [tt[2 * ka + v] if ka is not None else tt[2 * v + kb] for v in (0, 1)]
    if f[0] == f[1]:
        return ("const", f[0])
    return ("copy", x) if f[0] == 0 else ("not", x)


def fold_mux(consts, same_data):
    """same_data: operands b and c are the same sample."""
    ka, kb, kc = consts
    if ka is None and kb is None and kc is None and not same_data:
        return None
    if ka is not None:
        return ("copy", 1 if ka else 2)
    if same_data:
        return ("copy", 1)
    if kb is not None and kc is not None:                # kb != kc: equal constants are one shared sample
        return ("copy", 0) if kb == 1 else ("not", 0)
    if kc is not None:
        return ("gate", "AND" if kc == 0 else "ORNY", (0, 1))
    return ("gate", "ANDNY" if kb == 0 else "OR", (0, 2))


def fold_gate3(name, mask, consts):
    """One constant operand: the two-input gate of the other two with the same truth table (which folds again by its
    own rule when another operand is constant)."""
    which = [i for i in range(3) if consts[i] is not None]
    if not which:
        return None
    k = which[-1]
    x, y = [i for i in range(3) if i != k]
    for g2, v in GATE2.items():
        tt = v[4]
        if all(tt[2 * a + b] == gate3_truth(name, mask, *[consts[k] if i == k else (a if i == x else b) for i in range(3)])
               for a in (0, 1) for b in (0, 1)):
            return ("gate", g2, (x, y))
    raise AssertionError("a three-input gate with a constant operand is a two-input gate")
