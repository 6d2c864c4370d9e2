"""Model-based test of the recording layer on the CPU: random programs go through tfhe_hip_test_level_plan_full (the
recorder's own graph, elimination, levelling and plan code over a plain slot table), and the plan that comes back is
EXECUTED here on a scalar model and compared with the records taken one at a time in recording order.

The model.  A sample is one 32-bit word (the LWE body alone, n = 0), arithmetic wraps mod 2^32, a blind rotation is a
fixed hash of (key, phase word, test polynomial, extract spec, output number) and a key switch a hash of (key, word): a
wrong coefficient, operand, key, LUT, spec or output number changes the word.  The gates' integers are the literal table
of tests/program_common.py; nothing is computed by an expression taken from the library.

What the entry accepts decides what is generated here.  It takes each destination id once (a second write of an id is
refused: the renaming of an overwritten sample is the recorder's, not the graph's) and hands a NOT of a pending NOT to
the graph as it stands (the alias NOT(NOT x) = x is made in recorder.cpp before the graph is asked).  So records of the
form r = AND(r, x) and NOT-of-NOT are left to tests/test_gpu_recorded_programs.py, which drives the real recorder."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import program_common as PC
from program_common import INT32_MAX, INT32_MIN, KIND_GATE3, KIND_LIN, KIND_LUT, KIND_LUTM, KIND_MUX, KIND_NOT, M32

I32 = np.int32
P32 = C.POINTER(C.c_int32)
SPEC_NOUT = (1, 2, 3, 4)                 # extract spec s has SPEC_NOUT[s] outputs
WANTED_SHIFT, ENTRY_MASK = 24, (1 << 24) - 1
NINPUTS = 6
COEFS = (0, 1, -1, 2, -2, 3, -5, INT32_MIN, INT32_MAX, 1 << 30, 7)
MUTATIONS = ("negate_sa", "rot_key", "swap_u0", "rank_to_zero", "drop_not", "clear_wanted", "negate_rewritten")


@pytest.fixture(scope="module")
def L():
    from peba1_amd import lib
    return lib.load()


class PlanError(AssertionError):
    pass


def need(cond, *what):
    if not cond:
        raise PlanError(what)


# ---- the scalar model --------------------------------------------------------------------------------------------------
def boot(key, t, lut, spec, m):
    return int.from_bytes(hashlib.blake2b(struct.pack("<iIiii", key, t & M32, lut, spec, m), digest_size=4).digest(), "little")


def keyswitch(key, word):
    return int.from_bytes(hashlib.blake2b(struct.pack("<iI", key, word & M32), digest_size=4, person=b"ks").digest(), "little")


class Rec:
    """One record: kind as the entry numbers it, dsts (-1: an output nobody asks for), operand ids (-1: absent)."""

    def __init__(self, kind, dsts, a=-1, b=-1, c=-1, key=0, lut=-1, coefs=(0, 0, 0), c0=0, spec=-1, terms=()):
        self.kind, self.dsts, self.a, self.b, self.c, self.key = kind, list(dsts), a, b, c, key
        self.lut, self.coefs, self.c0, self.spec, self.terms = lut, tuple(coefs), c0, spec, [tuple(t) for t in terms]

    def operands(self):
        return [x for x in (self.a, self.b, self.c) if x >= 0]

    def copy(self, dsts, **changes):
        r = Rec(self.kind, dsts, self.a, self.b, self.c, self.key, self.lut, self.coefs, self.c0, self.spec, self.terms)
        for k, v in changes.items():
            setattr(r, k, v)
        return r


def phase_of(r, val):
    """The word a bootstrapped record rotates by (MUX: its two), from the literal table."""
    if r.kind < 10:
        _, c8, sa, sb, _ = PC.GATE2_BY_CODE[r.kind]
        return (c8 * PC.EIGHTH + sa * val[r.a] + sb * val[r.b]) & M32
    if KIND_GATE3 <= r.kind < KIND_GATE3 + 24:
        sa, sb, sc = PC.gate3_coefs(PC.GATE3_BY_CODE[(r.kind - KIND_GATE3) >> 3], (r.kind - KIND_GATE3) & 7)
        return (sa * val[r.a] + sb * val[r.b] + sc * val[r.c]) & M32
    assert r.kind in (KIND_LUT, KIND_LUTM)
    return (r.c0 + sum(s * val[x] for s, x in zip(r.coefs, (r.a, r.b, r.c)) if x >= 0)) & M32


def direct(recs, inputs):
    """The records one by one, in recording order, on id -> word; a destination written again is overwritten."""
    val = dict(inputs)
    for r in recs:
        if r.kind == KIND_NOT:
            out = [(-val[r.a]) & M32]
        elif r.kind == KIND_LIN:
            out = [(r.c0 + sum(c * val[x] for x, c in r.terms)) & M32]
        elif r.kind == KIND_MUX:
            f, s = PC.GATE2[PC.MUX_FIRST], PC.GATE2[PC.MUX_SECOND]
            u1 = boot(r.key, f[1] * PC.EIGHTH + f[2] * val[r.a] + f[3] * val[r.b], -1, -1, 0)
            u2 = boot(r.key, s[1] * PC.EIGHTH + s[2] * val[r.a] + s[3] * val[r.c], -1, -1, 0)
            out = [keyswitch(r.key, u1 + u2 + PC.MUX_ADD * PC.EIGHTH)]
        elif r.kind == KIND_LUTM:
            t = phase_of(r, val)
            out = [keyswitch(r.key, boot(r.key, t, r.lut, r.spec, m)) for m in range(len(r.dsts))]
        else:
            out = [keyswitch(r.key, boot(r.key, phase_of(r, val), r.lut if r.kind == KIND_LUT else -1, -1, 0))]
        for d, w in zip(r.dsts, out):
            if d >= 0:
                val[d] = w
    return val


class Recording:
    """The model of what the recorder makes of the records (written from the rules in DESIGN.md and the headers' comments,
    no code shared): sharing, widening, the two NOT rewrites, and the reverse-liveness pass."""

    def __init__(self, recs, reuse, dead):
        self.canon, self.shared, self.ops, self.op_of = {}, [], [], []
        index, not_origin, lin_out = {}, {}, set()
        slot = lambda x: self.canon.get(x, x)
        for i, r in enumerate(recs):
            kind, srcs, rewritten = r.kind, [slot(x) for x in r.operands()], []
            if kind == KIND_NOT and srcs[0] in lin_out:
                kind, terms = KIND_LIN, [(srcs[0], -1)]
            elif kind == KIND_LIN:
                terms = []
                for x, c in r.terms:
                    s = slot(x)
                    rewritten.append(s in not_origin)
                    terms.append((not_origin[s], (-c) & M32) if s in not_origin else (s, c & M32))
            if kind == KIND_LIN:
                op = dict(rec=i, kind=kind, key=r.key, srcs=[s for s, _ in terms], terms=terms, rewritten=rewritten, dsts=list(r.dsts))
                lin_out.add(r.dsts[0])
                self.shared.append(-1)
                self.op_of.append(len(self.ops))
                self.ops.append(op)
                continue
            a_b = sorted(srcs) if kind < 10 and PC.GATE2_BY_CODE[kind][0] in PC.SYMMETRIC else srcs
            key = (kind, tuple(a_b), r.key) + ((r.lut, r.coefs, r.c0 & M32, r.spec) if kind in (KIND_LUT, KIND_LUTM) else ())
            at = index.get(key) if reuse else None
            if at is None:
                op = dict(rec=i, kind=kind, key=r.key, srcs=srcs, dsts=list(r.dsts))
                if reuse:
                    index[key] = len(self.ops)
                if kind == KIND_NOT:
                    not_origin[r.dsts[0]] = srcs[0]
                self.shared.append(-1)
                self.op_of.append(len(self.ops))
                self.ops.append(op)
                continue
            have = self.ops[at]
            self.shared.append(have["rec"])
            self.op_of.append(at)
            for m, d in enumerate(r.dsts):
                if d < 0:
                    continue
                if have["dsts"][m] >= 0:
                    self.canon[d] = have["dsts"][m]          # served by the pending op
                else:
                    have["dsts"][m] = d                      # widened
        # reverse liveness: a result is alive if a handle that is not dead names it or a surviving record reads it
        held = {slot(d) for r in recs for d in r.dsts if d >= 0 and d not in dead}
        needed = set()
        for op in reversed(self.ops):
            op["dsts"] = [d if d >= 0 and (d in held or d in needed) else -1 for d in op["dsts"]]
            op["alive"] = any(d >= 0 for d in op["dsts"])
            if op["alive"]:
                needed.update(op["srcs"])
        self.eliminated = {i for i in range(len(recs)) if not self.ops[self.op_of[i]]["alive"]}
        alive = [op for op in self.ops if op["alive"]]
        boots = [op for op in alive if op["kind"] not in (KIND_NOT, KIND_LIN)]
        self.rotations = sum(2 if op["kind"] == KIND_MUX else 1 for op in boots)
        self.keyswitches = sum(sum(d >= 0 for d in op["dsts"]) for op in boots)
        self.producer = {d: op for op in alive for d in op["dsts"] if d >= 0}


# ---- the entry ----------------------------------------------------------------------------------------------------------
def p(a):
    return a.ctypes.data_as(P32)


def level_plan(L, recs, nkeys, unit, balance, reuse, dead):
    count = len(recs)
    ops, terms = np.zeros((count, 16), I32), []
    for i, r in enumerate(recs):
        if r.kind == KIND_LIN:
            ops[i, :10] = [KIND_LIN, r.dsts[0], -1, -1, -1, len(terms), len(r.terms), 0, 0, PC.s32(r.c0)]
            terms += [[x, PC.s32(c)] for x, c in r.terms]
            continue
        dst = r.dsts[0] if r.kind != KIND_LUTM else -1
        ops[i, :10] = [r.kind, dst, r.a, r.b, r.c, r.lut] + [PC.s32(c) for c in r.coefs] + [PC.s32(r.c0)]
        if r.kind == KIND_LUTM:
            ops[i, 10:12] = [r.spec, len(r.dsts)]
            ops[i, 12:16] = r.dsts + [-1] * (4 - len(r.dsts))
    nterms = len(terms)
    terms = np.ascontiguousarray(terms + [[0, 0]], dtype=I32)
    keys = np.ascontiguousarray([r.key for r in recs], dtype=I32)
    deadv = np.ascontiguousarray(sorted(dead) + [0], dtype=I32)
    z = lambda *shape: np.zeros(shape, I32)
    levels, ranks, shared, sizes = z(count), z(count), z(count), z(6)
    rot_off, ks_off, rot_koff, ks_koff = z(count + 1), z(count + 1), z(count * nkeys + 1), z(count * nkeys + 1)
    rot_key, rots, kss = z(2 * count), z(2 * count, 10), z(4 * count, 4)
    lin_sizes, level_off, launch_off, launch_rank, descs = z(2), z(count + 2), z(count + 1), z(count), z(count, 35)
    not_off, nots = z(count + 2), z(count, 2)
    depth = L.tfhe_hip_test_level_plan_full(p(ops), p(keys), count, nkeys, unit, balance, reuse, p(deadv), len(dead), p(terms),
                                            nterms, p(levels), p(ranks), p(shared), p(sizes), p(rot_off), p(ks_off), p(rot_koff),
                                            p(ks_koff), p(rot_key), p(rots), p(kss), p(lin_sizes), p(level_off), p(launch_off),
                                            p(launch_rank), p(descs), p(not_off), p(nots))
    assert depth >= 0, L.tfhe_hip_last_error().decode()
    assert sizes[0] == depth
    nrot, nks, nlaunch = int(sizes[1]), int(sizes[2]), int(lin_sizes[0])
    assert sizes[5] == (nrot if nkeys > 1 else 0) and sizes[3] == sizes[4] == (depth * nkeys + 1 if nkeys > 1 else 0)
    lins = [dict(dst=int(d[0]), c0=int(d[2]), terms=[(int(d[3 + t]), int(d[19 + t])) for t in range(d[1])]) for d in descs[:lin_sizes[1]]]
    return dict(levels=depth, nkeys=nkeys, level_of=levels.tolist(), rank_of=ranks.tolist(), shared=shared.tolist(),
                rot_off=rot_off[:depth + 1].tolist(), ks_off=ks_off[:depth + 1].tolist(),
                rot_koff=rot_koff[:sizes[3]].tolist(), ks_koff=ks_koff[:sizes[4]].tolist(), rot_key=rot_key[:sizes[5]].tolist(),
                rots=[[int(w) for w in rd] for rd in rots[:nrot]], kss=[[int(w) for w in kd] for kd in kss[:nks]],
                not_off=not_off[:depth + 2].tolist(), nots=[[int(w) for w in nd] for nd in nots[:not_off[depth + 1]]],
                lin_level_off=level_off[:depth + 2].tolist(), lin_launch_off=launch_off[:nlaunch + 1].tolist() if nlaunch else [0],
                lin_launch_rank=launch_rank[:nlaunch].tolist(), lins=lins)


# ---- the plan, executed as Engine::run_level runs it -----------------------------------------------------------------------
def rot_outputs(rd):
    """(output number, sample of the level's extract buffer) of every output a rotation writes."""
    if rd[9] < 0:
        return [(0, rd[5])]
    return [(m, rd[5] + m) for m in range(4) if rd[9] >> (WANTED_SHIFT + m) & 1]


def execute(plan, inputs):
    """-> (pool, trace).  Level 0: NOTs, then the linear launches; level L >= 1: the rotations from the pool as it stood,
    the key switches, the NOT launch, the linear launches in order.  A launch reads the pool as it was before it."""
    pool, nkeys = dict(inputs), plan["nkeys"]
    trace = dict(u=[], rot_reads=[])

    def read(s):
        need(s in pool, "a slot is read before anything wrote it", s)
        return pool[s]

    def launch(descs, what):
        """descs: (destination, slots read, value function)"""
        writes = [d for d, _, _ in descs]
        need(len(set(writes)) == len(writes), what, "writes a slot twice")
        for d, reads, _ in descs:
            need(not set(reads) & set(writes), what, "reads a slot the same launch writes", d)
        done = [(d, f()) for d, _, f in descs]
        for d, w in done:
            need(d not in pool, what, "writes a slot that holds a value already", d)
            pool[d] = w

    for lvl in range(plan["levels"] + 1):
        if lvl >= 1:
            g, u, reads = lvl - 1, {}, set()
            for r in range(plan["rot_off"][g], plan["rot_off"][g + 1]):
                a, b, sa, sb, c0, _, c, sc, lut, spec = plan["rots"][r]
                t = c0 + sa * read(a) + sb * read(b) + (sc * read(c) if c >= 0 else 0)
                reads.update(x for x in (a, b, c) if x >= 0)
                key = plan["rot_key"][r] if nkeys > 1 else 0
                for m, at in rot_outputs(plan["rots"][r]):
                    need(at not in u, "two rotations write one extracted sample", lvl, at)
                    u[at] = boot(key, t, lut, spec & ENTRY_MASK if spec >= 0 else -1, m)
            trace["u"].append(u)
            ks = []
            for j in range(plan["ks_off"][g], plan["ks_off"][g + 1]):
                u0, u1, add_b, dst = plan["kss"][j]
                key = 0
                if nkeys > 1:
                    key = next((k for k in range(nkeys) if plan["ks_koff"][g * nkeys + k] <= j < plan["ks_koff"][g * nkeys + k + 1]), None)
                    need(key is not None, "a key switch outside every key's run", j)
                need(u0 in u and (u1 < 0 or u1 in u), "a key switch reads an extracted sample no rotation wrote", lvl, j)
                ks.append((dst, (), lambda key=key, w=u[u0] + (u[u1] if u1 >= 0 else 0) + add_b: keyswitch(key, w)))
            need(not reads & {d for d, _, _ in ks}, "a rotation reads a slot its level's key switches write", lvl)
            launch(ks, "key switches")
        nots = plan["nots"][plan["not_off"][lvl]:plan["not_off"][lvl + 1]]
        launch([(d, (s,), lambda s=s: (-read(s)) & M32) for s, d in nots], "NOT launch")
        for j in range(plan["lin_level_off"][lvl], plan["lin_level_off"][lvl + 1]):
            descs = plan["lins"][plan["lin_launch_off"][j]:plan["lin_launch_off"][j + 1]]
            launch([(d["dst"], [s for s, _ in d["terms"]], lambda d=d: (d["c0"] + sum(c * read(s) for s, c in d["terms"])) & M32)
                    for d in descs], "linear launch")
    return pool, trace


def compare(recs, model, pool, want, dead):
    """Every slot the plan wrote and every destination id that still has a handle holds its direct value."""
    for r in recs:
        for d in r.dsts:
            if d < 0:
                continue
            s = model.canon.get(d, d)
            if s in pool:
                need(pool[s] == want[d], "a result differs from the record's direct value", d)
            need(d in dead or s in pool, "a live result was never written", d)


def check_structure(recs, model, plan, dead):
    nkeys, levels = plan["nkeys"], plan["levels"]
    need(plan["shared"] == model.shared, "shared_with", plan["shared"], model.shared)
    need({i for i, lv in enumerate(plan["level_of"]) if lv < 0} == model.eliminated, "the eliminated set")
    need(len(plan["rots"]) == model.rotations and len(plan["kss"]) == model.keyswitches, "rotation / key-switch counts",
         len(plan["rots"]), model.rotations, len(plan["kss"]), model.keyswitches)
    # each destination written exactly once, and exactly the surviving ones
    written = [kd[3] for kd in plan["kss"]] + [nd[1] for nd in plan["nots"]] + [d["dst"] for d in plan["lins"]]
    need(sorted(written) == sorted(model.producer), "the destinations written", sorted(written), sorted(model.producer))
    need(plan["rot_off"][0] == 0 == plan["ks_off"][0] and plan["rot_off"][-1] == len(plan["rots"]) and plan["ks_off"][-1] == len(plan["kss"]),
         "level offsets")
    for g in range(levels):
        r0, r1, k0, k1 = plan["rot_off"][g], plan["rot_off"][g + 1], plan["ks_off"][g], plan["ks_off"][g + 1]
        need(r0 <= r1 and k0 <= k1, "level offsets")
        # the rotations' ranges of the extract buffer: disjoint, inside what the level extracts
        owner, total = {}, 0
        for r in range(r0, r1):
            rd = plan["rots"][r]
            width = SPEC_NOUT[rd[9] & ENTRY_MASK] if rd[9] >= 0 else 1
            total += width
            for at in range(rd[5], rd[5] + width):
                need(at not in owner, "u_index ranges overlap", g, at)
                owner[at] = r
        need(all(0 <= at < total for at in owner), "a u_index outside the level's extract count", g)
        if nkeys > 1:
            for k in range(nkeys):
                need(plan["rot_koff"][g * nkeys + k] <= plan["rot_koff"][g * nkeys + k + 1] and
                     plan["ks_koff"][g * nkeys + k] <= plan["ks_koff"][g * nkeys + k + 1], "key runs")
            need(plan["rot_koff"][g * nkeys] == r0 and plan["rot_koff"][(g + 1) * nkeys] == r1 and
                 plan["ks_koff"][g * nkeys] == k0 and plan["ks_koff"][(g + 1) * nkeys] == k1, "the key runs partition the level")
            for r in range(r0, r1):
                k = plan["rot_key"][r]
                need(plan["rot_koff"][g * nkeys + k] <= r < plan["rot_koff"][g * nkeys + k + 1], "a rotation outside its key's run", r)
        switched = {}
        for j in range(k0, k1):
            u0, u1, add_b, dst = plan["kss"][j]
            op = model.producer[dst]
            need(plan["level_of"][op["rec"]] == g + 1, "a key switch on another level than its record", dst)
            for at in (u0, u1) if u1 >= 0 else (u0,):
                need(at in owner, "a key switch names a sample outside every rotation's range", g, at)
                r = owner[at]
                switched.setdefault(r, set()).add(at - plan["rots"][r][5])
                if nkeys > 1:
                    need(plan["rot_key"][r] == op["key"], "rot_key is not the record's key", r)
                    need(plan["ks_koff"][g * nkeys + op["key"]] <= j < plan["ks_koff"][g * nkeys + op["key"] + 1],
                         "a key switch outside its key's run", j)
        for r in range(r0, r1):
            rd = plan["rots"][r]
            wanted = {m for m in range(4) if rd[9] >> (WANTED_SHIFT + m) & 1} if rd[9] >= 0 else {0}
            need(switched.get(r) == wanted, "the wanted mask is not the set of outputs with a key switch", r)


def check(recs, model, plan, inputs, want, dead, structure=True):
    if structure:
        check_structure(recs, model, plan, dead)
    pool, trace = execute(plan, inputs)
    compare(recs, model, pool, want, dead)
    return pool, trace


# ---- mutations: each returns the list of mutated plans it can make of this plan (at most one) ---------------------------------
def clone(plan):
    out = dict(plan)
    for k in ("rots", "kss", "nots"):
        out[k] = [list(x) for x in plan[k]]
    out["lins"] = [dict(d, terms=list(d["terms"])) for d in plan["lins"]]
    for k in ("rot_key", "not_off", "lin_launch_off", "lin_level_off"):
        out[k] = list(plan[k])
    return out


def mutate(name, plan, model, pool, trace, rng):
    m = clone(plan)
    if name == "negate_sa":
        # where the negation changes the phase word: 2 sa A != 0 mod 2^32
        hits = [r for r, rd in enumerate(plan["rots"]) if (2 * rd[2] * pool[rd[0]]) & M32]
        if not hits:
            return None
        r = hits[rng.integers(len(hits))]
        m["rots"][r][2] = PC.s32(-m["rots"][r][2])
    elif name == "rot_key":
        if plan["nkeys"] < 2 or not plan["rot_key"]:
            return None
        r = int(rng.integers(len(plan["rot_key"])))
        m["rot_key"][r] = (m["rot_key"][r] + 1 + int(rng.integers(plan["nkeys"] - 1))) % plan["nkeys"]
    elif name == "swap_u0":
        pairs = []
        for g in range(plan["levels"]):
            js, u = range(plan["ks_off"][g], plan["ks_off"][g + 1]), trace["u"][g]
            pairs += [(i, j) for i in js for j in js if i < j and u[plan["kss"][i][0]] != u[plan["kss"][j][0]]][:8]
        if not pairs:
            return None
        i, j = pairs[rng.integers(len(pairs))]
        m["kss"][i][0], m["kss"][j][0] = plan["kss"][j][0], plan["kss"][i][0]
    elif name == "rank_to_zero":
        # a descriptor of a rank >= 1 launch goes to the end of the rank-0 launch of its level
        hits = [(lvl, j) for lvl in range(plan["levels"] + 1) for j in range(plan["lin_level_off"][lvl] + 1, plan["lin_level_off"][lvl + 1])]
        if not hits:
            return None
        lvl, j = hits[rng.integers(len(hits))]
        first = plan["lin_level_off"][lvl]
        assert plan["lin_launch_rank"][first] == 0 and plan["lin_launch_rank"][j] >= 1
        at = plan["lin_launch_off"][j]
        d = m["lins"].pop(at)
        m["lins"].insert(plan["lin_launch_off"][first + 1], d)
        for k in range(first + 1, j + 1):
            m["lin_launch_off"][k] += 1
    elif name == "drop_not":
        if not plan["nots"]:
            return None
        at = int(rng.integers(len(plan["nots"])))
        del m["nots"][at]
        m["not_off"] = [o - (o > at) for o in plan["not_off"]]
    elif name == "clear_wanted":
        hits = [r for r, rd in enumerate(plan["rots"]) if rd[9] >= 0]
        if not hits:
            return None
        r = hits[rng.integers(len(hits))]
        bits = [b for b in range(4) if plan["rots"][r][9] >> (WANTED_SHIFT + b) & 1]
        m["rots"][r][9] &= ~(1 << (WANTED_SHIFT + bits[rng.integers(len(bits))]))
    elif name == "negate_rewritten":
        # a term the recorder moved from a pending NOT's result onto the NOT's operand, where the sign matters
        hits = []
        for at, d in enumerate(plan["lins"]):
            op = model.producer[d["dst"]]
            for t, (s, c) in enumerate(d["terms"]):
                if op.get("rewritten") and op["rewritten"][t] and (2 * c * pool[s]) & M32:
                    hits.append((at, t))
        if not hits:
            return None
        at, t = hits[rng.integers(len(hits))]
        s, c = m["lins"][at]["terms"][t]
        m["lins"][at]["terms"][t] = (s, PC.s32(-c))
    return m


# ---- random programs ------------------------------------------------------------------------------------------------------
def random_program(rng, nkeys, size):
    """-> (records, dead ids).  Built to meet the recorder's rules: duplicates (same order, swapped, another key), multi
    output records and later equal ones that want a further output, linear terms on pending NOTs and on pending linear
    results, chains of dependent linear records, NOTs of linear results, random dead sets."""
    recs, avail, kind_of = [], list(range(NINPUTS)), {i: "in" for i in range(NINPUTS)}
    nxt = [100]

    def fresh():
        nxt[0] += 1
        return nxt[0]

    def pick(kinds=None):
        pool = avail if kinds is None else [x for x in avail if kind_of[x] in kinds]
        if not pool:
            pool = avail
        return int(pool[-1 - int(rng.integers(min(len(pool), 6)))] if rng.random() < 0.5 else pool[rng.integers(len(pool))])

    def key():
        return int(rng.integers(nkeys))

    def coef():
        return int(COEFS[rng.integers(len(COEFS))]) if rng.random() < 0.7 else int(rng.integers(INT32_MIN, INT32_MAX + 1))

    def add(r, kind):
        recs.append(r)
        for d in r.dsts:
            if d >= 0:
                avail.append(d)
                kind_of[d] = kind

    def lut_fields():
        nin = int(rng.integers(1, 4))
        ops = [pick() for _ in range(nin)] + [-1] * (3 - nin)
        return dict(a=ops[0], b=ops[1], c=ops[2], key=key(), lut=int(rng.integers(3)),
                    coefs=[coef() for _ in range(nin)] + [0] * (3 - nin), c0=coef())

    def linear(first=None):
        n = int(rng.integers(1, 17)) if rng.random() < 0.25 else int(rng.integers(1, 5))
        terms = []
        for _ in range(n):
            x = rng.random()
            src = pick(("not",)) if x < 0.3 else pick(("lin",)) if x < 0.6 else terms[-1][0] if x < 0.7 and terms else pick()
            terms.append((src, coef()))
        if first is not None:
            terms[int(rng.integers(n))] = (first, coef() | 1)
        add(Rec(KIND_LIN, [fresh()], key=key(), c0=coef(), terms=terms), "lin")

    while len(recs) < size:
        x = rng.random()
        if x < 0.26:
            add(Rec(int(rng.integers(10)), [fresh()], pick(), pick(), key=key()), "boot")
        elif x < 0.32:
            add(Rec(KIND_MUX, [fresh()], pick(), pick(), pick(), key=key()), "boot")
        elif x < 0.44:
            # (a NOT of a pending NOT's result is aliased by recorder.cpp before the graph sees it: not generated here)
            src = pick(("in", "boot", "lin"))
            if kind_of[src] != "not":
                add(Rec(KIND_NOT, [fresh()], src, key=key()), "lin" if kind_of[src] == "lin" else "not")
        elif x < 0.51:
            add(Rec(KIND_GATE3 + int(rng.integers(24)), [fresh()], pick(), pick(), pick(), key=key()), "boot")
        elif x < 0.59:
            add(Rec(KIND_LUT, [fresh()], **lut_fields()), "boot")
        elif x < 0.67:
            spec = int(rng.integers(4))
            want = [rng.random() < 0.6 for _ in range(SPEC_NOUT[spec])]
            if not any(want):
                want[int(rng.integers(len(want)))] = True
            add(Rec(KIND_LUTM, [fresh() if w else -1 for w in want], spec=spec, **lut_fields()), "boot")
        elif x < 0.80:
            linear()
        elif x < 0.84:
            for _ in range(int(rng.integers(3, 5))):                 # a chain: each reads the one before
                linear(first=avail[-1] if kind_of[avail[-1]] == "lin" else None)
        elif recs:
            # a record again: as it was, with the first two operands swapped, under another key, or (multi-output) wanting
            # another set of outputs
            old = recs[int(rng.integers(len(recs)))]
            if old.kind == KIND_LIN or (old.kind == KIND_NOT and kind_of[old.dsts[0]] == "lin"):
                continue
            how = rng.random()
            change = {}
            if how < 0.3 and old.b >= 0:
                change = dict(a=old.b, b=old.a)
                if old.kind in (KIND_LUT, KIND_LUTM):
                    change["coefs"] = (old.coefs[1], old.coefs[0], old.coefs[2])    # the same function, keyed as given
            elif how < 0.5 and nkeys > 1:
                change = dict(key=(old.key + 1 + int(rng.integers(nkeys - 1))) % nkeys)
            dsts = [fresh() if rng.random() < 0.6 else -1 for _ in old.dsts]
            if not any(d >= 0 for d in dsts):
                dsts[int(rng.integers(len(dsts)))] = fresh()
            add(old.copy(dsts, **change), "not" if old.kind == KIND_NOT else "boot")
    made = [d for r in recs for d in r.dsts if d >= 0]
    frac = (0.0, 0.2, 0.5)[int(rng.integers(3))]
    dead = {d for d in made if rng.random() < frac}
    if rng.random() < 0.5:                                           # the NOTs that only linear records read lose their handles
        dead |= {d for d in made if kind_of[d] == "not" and rng.random() < 0.7}
    return recs, dead


PARAMS = [(nkeys, unit, balance, reuse) for nkeys in (1, 2, 3, 16) for unit in (1, 4, 256) for balance in (0, 1) for reuse in (0, 1)]
SEEDS_PER_PARAM = 42
SIZES = (5, 8, 13, 21, 34, 55, 89, 120)


def run_program(L, seed, nkeys, unit, balance, reuse, counts=None):
    rng = np.random.default_rng(seed)
    recs, dead = random_program(rng, nkeys, int(SIZES[rng.integers(len(SIZES))]))
    inputs = {i: int(rng.integers(1, 1 << 32)) | 1 for i in range(NINPUTS)}
    want = direct(recs, inputs)
    model = Recording(recs, reuse, dead)
    plan = level_plan(L, recs, nkeys, unit, balance, reuse, dead)
    pool, trace = check(recs, model, plan, inputs, want, dead)
    if counts is not None:
        for name in MUTATIONS:
            bad = mutate(name, plan, model, pool, trace, rng)
            if bad is None:
                continue
            counts[name][0] += 1
            try:
                check(recs, model, bad, inputs, want, dead, structure=False)
            except PlanError:
                counts[name][1] += 1
    return recs, model, plan


def test_the_literal_gate_table_decrypts_to_the_truth_tables():
    PC.check_tables_against_truth()


def test_the_model_tells_a_wrong_argument_apart():
    base = (1, 0x12345678, 2, 3, 1)
    words = {boot(*base)} | {boot(*(base[:i] + (base[i] + 1,) + base[i + 1:])) for i in range(5)}
    assert len(words) == 6 and keyswitch(0, 5) != keyswitch(1, 5) != keyswitch(1, 6)


def test_random_programs_run_as_their_records_say_and_mutated_plans_do_not(L):
    """About two thousand programs over nkeys x unit x balance x reuse; every plan is checked for structure, executed and
    compared, then mutated in each way that applies to it, and every mutated plan must fail the execution or comparison
    (the structural checks are left out there: the words alone must tell)."""
    counts = {name: [0, 0] for name in MUTATIONS}
    programs = records = 0
    seen = set()
    for pi, (nkeys, unit, balance, reuse) in enumerate(PARAMS):
        for s in range(SEEDS_PER_PARAM):
            recs, model, plan = run_program(L, 1000 * pi + s, nkeys, unit, balance, reuse, counts)
            programs += 1
            records += len(recs)
            seen.update(r.kind for r in recs)
    print(f"programs {programs}, records {records}, mutations applicable / detected: " +
          ", ".join(f"{k} {a}/{d}" for k, (a, d) in counts.items()))
    assert seen == set(range(10)) | {KIND_MUX, KIND_NOT, KIND_LUT, KIND_LUTM, KIND_LIN} | set(range(KIND_GATE3, KIND_GATE3 + 24))
    for name, (applicable, detected) in counts.items():
        assert applicable >= 50, (name, applicable)
        assert detected == applicable, (name, applicable, detected)


def test_the_generator_meets_the_rules_it_is_built_for(L):
    """Over a slice of the run: shared records in the same and in swapped order, an asymmetric swap and another key that
    must not share, widened multi-output records, rewritten terms, NOTs that became linear, ranks of at least 2 on a
    level, eliminated records, balanced levels that differ from the as-soon-as-possible ones."""
    met = dict(shared=0, swapped_shared=0, asym_swap_apart=0, other_key_apart=0, widened=0, rewritten=0, not_as_lin=0,
               rank2=0, eliminated=0, multi_level_lins=0)
    for pi, (nkeys, unit, balance, reuse) in enumerate(PARAMS):
        for s in range(6):
            recs, model, plan = run_program(L, 1000 * pi + s, nkeys, unit, balance, reuse)
            first = {}
            for i, r in enumerate(recs):
                if r.kind < 10:
                    j = first.setdefault((r.kind, frozenset((model.canon.get(r.a, r.a), model.canon.get(r.b, r.b))), r.key), i)
                    old = recs[j]
                    same = (model.canon.get(old.a, old.a), model.canon.get(old.b, old.b)) == (model.canon.get(r.a, r.a), model.canon.get(r.b, r.b))
                    if j != i and reuse and old.a != old.b:
                        sym = PC.GATE2_BY_CODE[r.kind][0] in PC.SYMMETRIC
                        if same or sym:
                            assert plan["shared"][i] == (j if plan["shared"][j] < 0 else plan["shared"][j])
                            met["swapped_shared" if not same else "shared"] += 1
                        else:
                            assert plan["shared"][i] != j
                            met["asym_swap_apart"] += 1
                if plan["shared"][i] >= 0:
                    assert recs[plan["shared"][i]].key == r.key
                    if r.kind == KIND_LUTM and any(d >= 0 and d not in model.canon for d in r.dsts):
                        met["widened"] += 1
            by_what = {}
            for i, r in enumerate(recs):
                if r.kind < 10 or r.kind == KIND_MUX:
                    what = (r.kind, model.canon.get(r.a, r.a), model.canon.get(r.b, r.b), model.canon.get(r.c, r.c))
                    if reuse and any(recs[j].key != r.key for j in by_what.get(what, [])) and plan["shared"][i] < 0:
                        met["other_key_apart"] += 1
                    by_what.setdefault(what, []).append(i)
            met["rewritten"] += sum(any(op.get("rewritten", ())) for op in model.ops)
            met["not_as_lin"] += sum(op["kind"] == KIND_LIN and recs[op["rec"]].kind == KIND_NOT for op in model.ops)
            met["rank2"] += max(plan["rank_of"]) >= 2
            met["eliminated"] += bool(model.eliminated)
            met["multi_level_lins"] += sum(plan["lin_level_off"][lv + 1] > plan["lin_level_off"][lv] for lv in range(1, plan["levels"] + 1)) >= 2
    assert all(v >= 10 for v in met.values()), met
