"""Shared by tests/test_plan_model_cpu.py and tests/test_gpu_recorded_programs.py: the gates as a literal table of
integers (include/tfhe_hip.h and tfhe's boot-gates restated; nothing here is read from the library), their truth tables,
the decrypt rule of the plain +-1/8 encoding that ties the two together, and the constant-folding rule of the recorder
written out from truth tables.  For tests/test_gpu_recorded_programs.py and tests/test_program_moves_cpu.py also the
movement calls of a recorded program: the splice, the census of the hazards from a call list, three wrong models."""
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


# ---- movement calls: imports, exports, unpacks and packs spliced into a recorded program -------------------------------------
# A call list of tests/test_gpu_recorded_programs.py over handles (array, index).  The movement calls, beside the base calls
# of random_program there (T = the handles written or covered, in call order):
#   ("import", form, T, src)              T a run of one array; src ("random", seed) or ("observed", k, first): the words of
#                                         samples first .. of the k-th observation of the same program
#   ("export", form, T)                   T a run of one array; an observation
#   ("unpack", form, index, T, key)       from the two plain ring samples; index None: 0 .. len(T) - 1; T a run of one array,
#                                         for the scattered form any handles, repeats allowed
#   ("unpack_seeded", form, index, T, key)   the same from the one compressed ring sample
#   ("import_seeded", form, index, T)     from the seeded record of RECORD samples
#   ("pack", form, T)                     T a run of one array; an observation
MOVE_FORMS = {"import": ("host", "device", "device_async"), "export": ("device", "device_async"),
              "unpack": ("host", "scattered", "device"), "unpack_seeded": ("host", "scattered", "device"),
              "import_seeded": ("host", "scattered", "device"), "pack": ("host", "device")}
WRITER_MOVES = ("import", "unpack", "unpack_seeded", "import_seeded")
OBSERVER_MOVES = ("export", "pack")
RECORDED_OPS = ("gate", "mux", "not", "gate3", "lut", "lutm", "lin")       # what stays pending until a flush
FLUSH_POINTS = ("flush", "flush_async", "observe", "export", "pack")       # where the census takes the recording as run
RECORD = 64                                                                # samples of the seeded LWE record
CLASSES = ("i", "ii", "iii", "iv", "v", "vi", "vii")


def reads_of(call):
    """the handles whose value the call reads"""
    k = call[0]
    if k == "gate":
        return [call[3], call[4]]
    if k == "mux":
        return [call[2], call[3], call[4]]
    if k in ("not", "copy"):
        return [call[2]]
    if k == "gate3":
        return [call[4], call[5], call[6]]
    if k == "lut":
        return list(call[3])
    if k == "lutm":
        return list(call[2])
    if k == "lin":
        return list(call[2])
    if k == "observe":
        return [call[1]]
    if k in OBSERVER_MOVES:
        return list(call[2])
    return []


def writes_of(call):
    """the handles the call gives a new value, in the order it writes them"""
    k = call[0]
    if k in ("mux", "not", "copy", "const", "lin"):
        return [call[1]]
    if k == "gate":
        return [call[2]]
    if k == "gate3":
        return [call[3]]
    if k == "lut":
        return [call[2]]
    if k == "lutm":
        return [r for r in call[1] if r is not None]
    if k == "import":
        return list(call[2])
    if k in ("unpack", "unpack_seeded", "import_seeded"):
        return list(call[3])
    return []


def base_of(calls):
    return [c for c in calls if c[0] not in MOVE_FORMS]


def with_moves(calls, seed, nmoves, nkeys=1, N=1024, narr=6, per=4):
    """The base program `calls`, unchanged and in its order, with about `nmoves` movement calls spliced in from a generator
    of its own.  A position is drawn at random; most draws choose it among the places where the base program has what a
    hazard needs -- behind a flush_async, in front of a re-allocation, around a recorded operation whose operand or result
    the move then renames, covers or supplies -- and the rest anywhere.  Whether the hazards did come about is counted from
    the finished list (census)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    ri = lambda n: int(rng.integers(n))
    handles = [(a, i) for a in range(narr) for i in range(per)]
    at = {p: [] for p in range(len(calls) + 1)}                 # position -> the moves in front of base call `position`
    ops = [p for p, c in enumerate(calls) if c[0] in RECORDED_OPS]
    asyncs = [p for p, c in enumerate(calls) if c[0] == "flush_async"]
    reallocs = [p for p, c in enumerate(calls) if c[0] == "realloc"]

    def run(h=None):
        """a run of 1 to 4 handles of one array, through h if one is given"""
        a, i = h if h is not None else handles[ri(len(handles))]
        cnt = 1 + ri(per)
        i0 = max(0, i - cnt + 1) + ri(min(i, per - cnt) - max(0, i - cnt + 1) + 1)
        return [(a, j) for j in range(i0, i0 + cnt)]

    def scattered(h=None):
        t = [handles[ri(len(handles))] for _ in range(1 + ri(per))]
        if h is not None:
            t[ri(len(t))] = h
        if len(t) > 1 and rng.random() < 0.3:                    # a handle given twice ends with its last value
            t[-1] = t[0]
        return t

    def index(count, top, special):
        out = []
        for _ in range(count):
            if out and rng.random() < 0.25:
                out.append(out[-1])
            else:
                out.append(int(special[ri(len(special))]) if rng.random() < 0.5 else ri(top))
        return out

    def deck(cards):
        """the cards in a random order, again and again: every form comes up once before one comes up twice"""
        while True:
            for j in rng.permutation(len(cards)):
                yield cards[int(j)]

    writers = deck(sorted(f for f in all_forms() if f[0] in WRITER_MOVES))
    observers = deck(sorted(f for f in all_forms() if f[0] in OBSERVER_MOVES))

    def writer(h=None, card=None):
        card = card or next(writers)
        kind, form = card[:2]
        if kind == "import":
            return ("import", form, run(h), ("random", ri(1 << 30)))
        t = scattered(h) if form == "scattered" else run(h)
        if kind == "import_seeded":
            return (kind, form, index(len(t), RECORD, (0, RECORD - 1)), t)
        top, special = (2 * N, (0, N - 1, N, 2 * N - 1)) if kind == "unpack" else (N, (0, N - 1))
        return (kind, form, None if card[2] == "null" else index(len(t), top, special), t, ri(nkeys))

    def observer(h=None):
        kind, form = next(observers)
        return (kind, form, run(h))

    def any_move(h=None):
        return writer(h) if rng.random() < 0.7 else observer(h)

    pick = lambda seq: seq[ri(len(seq))]
    made = 0
    while made < nmoves:
        x = rng.random()
        made += 1
        if x < 0.12 and asyncs:                                  # a move right behind a flush_async
            at[pick(asyncs) + 1].insert(0, any_move())
        elif x < 0.24 and reallocs:                              # samples moved into an array that is then re-allocated
            p = pick(reallocs)
            at[p].append(writer((calls[p][1], ri(per))))
        elif x < 0.38 and ops:                                   # the operand of a pending operation is renamed
            p = pick(ops)
            at[p + 1].append(writer(pick(reads_of(calls[p]))))
        elif x < 0.52 and ops:                                   # the result of a pending operation is renamed
            p = pick(ops)
            at[p + 1].append(writer(pick(writes_of(calls[p]))))
        elif x < 0.64 and ops:                                   # a pending result is packed or exported
            p = pick(ops)
            at[p + 1].append(observer(pick(writes_of(calls[p]))))
        elif x < 0.76 and ops:                                   # a moved sample is the operand of the next operation
            p = pick(ops)
            at[p].append(writer(pick(reads_of(calls[p]))))
        elif x < 0.88 and ops:                                   # stream-ordered import, a gate on it, an observation
            p = pick(ops)
            at[p].append(writer(pick(reads_of(calls[p])), ("import", "device_async")))
            at[p + 1].insert(0, observer(pick(writes_of(calls[p]))))
            made += 1
        else:
            at[ri(len(calls) + 1)].append(any_move())
    out = []
    for p in range(len(calls) + 1):
        out.extend(at[p])
        if p < len(calls):
            out.append(calls[p])
    # now and then an import brings back words that the program exported earlier
    seen, nobs = [], 0                                           # (observation number, samples) of the sample observations
    for q, c in enumerate(out):
        if c[0] == "import" and seen and rng.random() < 0.35:
            fits = [(k, cnt) for k, cnt in seen if cnt >= len(c[2])]
            if fits:
                k, cnt = pick(fits)
                out[q] = c[:3] + (("observed", k, ri(cnt - len(c[2]) + 1)),)
        if c[0] in ("observe", "export"):
            seen.append((nobs, 1 if c[0] == "observe" else len(c[2])))
        nobs += c[0] in ("observe",) + OBSERVER_MOVES
    return out


def pending_walk(calls):
    """Per call, from the call list alone: (position, call, state before the call).  state: `reads` / `writes`, the
    handles that an operation recorded since the last flush point reads / has as its result and that still name that
    sample; `moved`, the handles holding a moved sample since the last flush point; `held`, the same whatever was flushed;
    `start`, the position behind the last flush point.  A flush point is a flush, a flush_async or an observation."""
    reads, writes, moved, held, start = set(), set(), set(), set(), 0
    for q, c in enumerate(calls):
        yield q, c, dict(reads=reads, writes=writes, moved=moved, held=held, start=start)
        k, R, W = c[0], reads_of(c), writes_of(c)
        if k in FLUSH_POINTS:
            reads, writes, moved, start = set(), set(), set(), q + 1
        else:
            reads, writes, moved = set(reads), set(writes), set(moved)
        held = set(held)
        gone = W if k != "realloc" else [h for h in reads | writes | moved | held if h[0] == c[1]]
        src = [c[2] in s for s in (writes, moved, held)] if k == "copy" and c[1] != c[2] else None
        if src is not None or k != "copy":
            for s in (reads, writes, moved, held):
                s.difference_update(gone)
        if k in RECORDED_OPS:
            reads.update(set(R) - set(W))                        # (r = AND(r, x): r names the result from here on)
            writes.update(W)
        elif k in WRITER_MOVES:
            moved.update(W)
            held.update(W)
        elif src is not None:                                    # a copy names its operand's sample
            for s, had in zip((writes, moved, held), src):
                if had:
                    s.add(c[1])


def census(calls):
    """-> (classes, forms): how often each hazard class of a program with moves occurs, counted from the call list alone,
    and the forms of the movement calls that occur (an unpack's index list or NULL is part of its form).
    (i) a move writes a handle a pending operation reads; (ii) ... a pending operation writes; (iii) a move directly
    behind a flush_async; (iv) a pack or export covers a pending result; (v) a moved sample is read by a recorded operation
    before any flush point; (vi) an array holding moved samples is re-allocated; (vii) a device-async import, an operation
    recorded on it with no flush point between, then an observation with no flush between."""
    n = dict.fromkeys(CLASSES, 0)
    forms, chains, prev = set(), [], None
    for q, c, st in pending_walk(calls):
        k, R, W = c[0], set(reads_of(c)), set(writes_of(c))
        if k in MOVE_FORMS:
            forms.add((k, c[1]) + (("listed" if c[2] is not None else "null",) if k.startswith("unpack") else ()))
            n["iii"] += prev == "flush_async"
        if k in WRITER_MOVES:
            n["i"] += bool(W & st["reads"])
            n["ii"] += bool(W & st["writes"])
        if k in OBSERVER_MOVES:
            n["iv"] += bool(R & st["writes"])
        if k in RECORDED_OPS:
            n["v"] += bool(R & st["moved"])
            for ch in chains:
                ch[1] = ch[1] or bool(R & ch[0])
        if k == "realloc":
            n["vi"] += any(h[0] == c[1] for h in st["held"])
        if k in FLUSH_POINTS:
            if k not in ("flush", "flush_async"):
                n["vii"] += sum(ch[1] for ch in chains)
            chains = []
        for ch in chains:                                        # an overwritten handle no longer holds the imported words
            if not ch[1]:
                ch[0] -= W | ({h for h in ch[0] if h[0] == c[1]} if k == "realloc" else set())
        if k == "import" and c[1] == "device_async":
            chains.append([set(W), False])
        prev = k
    return n, forms


def all_forms():
    out = set()
    for k, fs in MOVE_FORMS.items():
        for f in fs:
            out |= {(k, f, x) for x in ("listed", "null")} if k.startswith("unpack") else {(k, f)}
    return out


# ---- three wrong models of the moves, as rewritten call lists: the sequential replay of each must differ from the true one ----
def wrong_import_without_rename(calls):
    """an import that wrote into the handle's old slot: the pending operation that reads the handle sees the new words --
    every plain import moves in front of the earliest still-pending operation that reads one of its handles"""
    out = list(calls)
    for q, c, st in list(pending_walk(calls)):
        if c[0] == "import" and set(c[2]) & st["reads"]:
            first = min(p for p in range(st["start"], q) if out[p][0] in RECORDED_OPS and set(reads_of(out[p])) & set(c[2]) & st["reads"])
            out[first + 1:q + 1] = out[first:q]
            out[first] = c
    return out


def wrong_pack_before_pending(calls):
    """a pack that did not run the pending operations first: it sees the samples as they were at the last flush point"""
    out = list(calls)
    for q, c, st in list(pending_walk(calls)):
        if c[0] == "pack" and st["start"] < q:
            out[st["start"] + 1:q + 1] = out[st["start"]:q]
            out[st["start"]] = c
    return out


def wrong_unpack_lost_to_pending_result(calls):
    """an unpack into the result handle of a pending operation, which then ran and wrote over the unpacked sample: those
    handles drop out of the unpack"""
    out = []
    for q, c, st in pending_walk(calls):
        if c[0] in ("unpack", "unpack_seeded") and set(c[3]) & st["writes"]:
            index = c[2] if c[2] is not None else list(range(len(c[3])))
            keep = [j for j, h in enumerate(c[3]) if h not in st["writes"]]
            if not keep:
                continue
            c = (c[0], "scattered", [index[j] for j in keep], [c[3][j] for j in keep], c[4])
        out.append(c)
    return out
