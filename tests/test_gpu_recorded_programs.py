"""Random recorded programs through the real C API -- the recorder, the slot pool, the flush and the kernels -- word for
word against a sequential replay: a Python interpreter that applies the CPU oracle call by call, in call order, on a
table handle -> words.  The parameter set is P128's ring, gadget and key switch with a 16-step blind rotation (custom
set n = 16, N = 1024, k = 1, l = 3, Bgbit = 7, ks 8 x 2), so the recorder is what is under test and a replay costs
milliseconds.  A program overwrites and aliases its ~24 handles all the time: r = AND(r, x), NOT of a pending NOT,
copies, constants, never-written samples, freed arrays with pending results -- what tests/test_plan_model_cpu.py cannot
reach through the plan entry.  LUT and linear results are compared as words only; no decrypt claim is made for them.

Programs with moves (with_moves of tests/program_common.py splices them into a base program) also move samples from
outside the recording: imports of caller words (host, device and stream-ordered), exports into device memory, unpacks of
plain and of seed-compressed ring samples (a run of one array or the scattered form, an index list or NULL, under any of
the recording's keys), imports from a seeded LWE record, and packs under a packing key.  The contracts of
include/tfhe_hip.h they exercise: every imported or unpacked result is RENAMED INTO A FRESH SLOT -- a pending operation
that reads the handle still reads the old sample, one that writes it does not write the new one; A FLUSH IN FLIGHT IS
COMPLETED FIRST by the unpacks and the seeded import; RECORDED OPERATIONS STAY RECORDED across all of them (and all of
them run, whatever became of their result handles, unless eliminate_dead drops them); and THE PACK IS AN OBSERVATION
POINT like the exports -- what is pending runs first, a flush in flight included.  Expected words come from the numpy
restatements (unpack_common, pack_common, seeded_lwe_common, seeded_wire_common); every tensor of a device form stays
alive to the final tfhe_hip_stream_sync, and the stream-ordered observations are compared behind it.
tests/test_program_moves_cpu.py counts, from the call lists, that the hazards do occur in these programs."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import gate3_common as G3
import ks_common as K
import lut_common as T
import lut_multi_common as M
import pack_common as PK
import program_common as PC
import seeded_lwe_common as SL
import seeded_wire_common as SW
import unpack_common as U

pytestmark = pytest.mark.gpu
I32 = np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LWE, NARR, PER = 16, 6, 4
KEY_SEEDS = (0x51A7, 0x51A8, 0x51A9)
GATES = list(PC.GATE2)
DEFAULTS = {"reuse_gates": 1, "eliminate_dead": 1, "balance_levels": 1, "fold_constants": 0, "batch_keys": 0}
COEFS = (0, 1, -1, 2, -2, 3, PC.INT32_MIN, PC.INT32_MAX, 1 << 29)
# mode (e): the pool's two shared constants hold two slots, so with 4,098 in all "fewer than 4,096 free slots" holds from the
# first materialised operand on, and every call that finds an op pending runs it first (a program's live samples are a few
# dozen slots at the most: the pool itself never runs dry)
POOL_SLOTS = 4096 + 2
# the programs with moves: mode -> (base seed, base calls, keys, splice seed, moves), chosen so that every hazard class of
# program_common.census occurs at least three times and every form of every movement call at least once
# (tests/test_program_moves_cpu.py checks that)
MOVES_PROGRAMS = {"a": (1001, 180, 1, 4, 60), "b": (1003, 70, 1, 5, 40), "c": (1003, 180, 3, 1, 60), "e": (1000, 170, 1, 4, 60)}


# ---- programs ---------------------------------------------------------------------------------------------------------------
def random_program(seed, ncalls, nkeys=1):
    """Calls over handles (array, index).  Every handle is operand and result alike, so overwriting is the norm.  The
    LUT and linear calls write arrays 3 to 5 only and the gates mostly read and write the others, so that some handles
    hold Boolean functions of the inputs to the end (mode (d) decrypts those)."""
    rng = np.random.default_rng(seed)
    handles = [(a, i) for a in range(NARR) for i in range(PER)]
    words_side = [x for x in handles if x[0] >= 3]
    bool_side = [x for x in handles if x[0] < 3]
    any_h = lambda: handles[int(rng.integers(len(handles)))]
    hw = lambda: words_side[int(rng.integers(len(words_side)))]
    h = lambda: bool_side[int(rng.integers(len(bool_side)))] if rng.random() < 0.85 else any_h()
    key = lambda: int(rng.integers(nkeys))
    coef = lambda: int(COEFS[rng.integers(len(COEFS))]) if rng.random() < 0.6 else int(rng.integers(PC.INT32_MIN, PC.INT32_MAX + 1))
    calls = []
    while len(calls) < ncalls:
        x = rng.random()
        if x < 0.24:
            calls.append(("gate", GATES[int(rng.integers(10))], h(), h(), h(), key()))
        elif x < 0.30:
            calls.append(("mux", h(), h(), h(), h(), key()))
        elif x < 0.40:
            r, a = h(), h()
            calls.append(("not", r, a, key()))
            if rng.random() < 0.5:                          # NOT of the pending NOT, into a third handle or back
                calls.append(("not", h() if rng.random() < 0.5 else a, r, key()))
        elif x < 0.44:
            calls.append(("copy", h(), h(), key()))
        elif x < 0.48:
            calls.append(("const", h(), int(rng.integers(2)), key()))
        elif x < 0.56:
            calls.append(("gate3", list(PC.GATE3)[int(rng.integers(3))], int(rng.integers(8)), h(), h(), h(), h(), key()))
        elif x < 0.63:
            nin = int(rng.integers(1, 4))
            calls.append(("lut", int(rng.integers(2)), hw(), [any_h() for _ in range(nin)], [coef() for _ in range(nin)], coef(), key()))
        elif x < 0.70:
            nin = int(rng.integers(1, 4))
            ins, coefs, c0, k = [any_h() for _ in range(nin)], [coef() for _ in range(nin)], coef(), key()
            free = [x for x in words_side if x not in ins]
            for _ in range(2 if rng.random() < 0.6 else 1):     # an equal call again that wants another set of outputs
                res = [free[i] for i in rng.choice(len(free), 4, replace=False)]
                want = rng.random(4) < 0.5
                want[int(rng.integers(4))] = True
                calls.append(("lutm", [r if w else None for r, w in zip(res, want)], ins, coefs, c0, k))
                free = [x for x in free if x not in res]
        elif x < 0.84:
            nin = int(rng.integers(1, 17)) if rng.random() < 0.3 else int(rng.integers(1, 5))
            calls.append(("lin", hw(), [any_h() for _ in range(nin)], [coef() for _ in range(nin)], coef(), key()))
        elif x < 0.88:
            calls.append(("flush",))
        elif x < 0.92:
            calls.append(("flush_async",))
        elif x < 0.98:
            calls.append(("observe", any_h(), "export" if rng.random() < 0.5 else "sync"))
        else:
            calls.append(("realloc", int(rng.integers(NARR))))
    return calls


def moves_program(mode):
    base_seed, ncalls, nkeys, seed, nmoves = MOVES_PROGRAMS[mode]
    return PC.with_moves(random_program(base_seed, ncalls, nkeys), seed, nmoves, nkeys=nkeys)


def results_of(call):
    if call[0] in ("gate", "mux", "not", "copy", "const", "lin"):
        return [call[1]] if call[0] != "gate" else [call[2]]
    if call[0] == "gate3":
        return [call[3]]
    if call[0] == "lut":
        return [call[2]]
    if call[0] == "lutm":
        return [r for r in call[1] if r is not None]
    return PC.writes_of(call) if call[0] in PC.WRITER_MOVES else []


# ---- the replay ---------------------------------------------------------------------------------------------------------------
class Fixture:
    """Keys on both sides from one seed each, the inputs, the two test polynomials and the four-output spec; for the
    moves two plain ring samples of random words, one compressed ring sample and one seeded LWE record of 64 samples under
    key 0 (mask words by the numpy restatements over the ChaCha known-answer hook), and a packing key of key 0."""

    def __init__(self, oracle, nkeys=1, device=True):
        from peba1_amd import api
        self.O, self.api = oracle, api
        self.pp = api.ParameterSet(custom=K.custom_tuple(N_LWE, 8, 2))
        n, N = self.pp.n, self.pp.N
        op = oracle.custom_params(n=n, N=N, l=K.GADGET[0], Bgbit=K.GADGET[1], ks_t=8, ks_basebit=2, ks_stdev=K.STDEVS[0],
                                  bk_stdev=K.STDEVS[1])
        self.ks = [api.SecretKeySet(self.pp, s, device=device) for s in KEY_SEEDS[:nkeys]]
        self.oks = [oracle.KeySet(op, s) for s in KEY_SEEDS[:nkeys]]
        self.lut_words = [T.lut_words({"kind": "sectors", "seed": 31, "slots": 8}, N), T.lut_words({"kind": "random", "seed": 32}, N)]
        self.spec = M.spec_templates(N, 1100)[4][0]                       # four outputs
        M.check_limits(N, self.spec)
        rng, bits = oracle.Rng(0xC0FFEE), np.random.default_rng(9).integers(0, 2, (NARR, PER))
        # arrays 0..3 hold fresh encryptions (array j under key j mod nkeys); 4 and 5 are never written
        self.inputs = {a: self.oks[a % nkeys].encrypt(rng, bits[a]) for a in range(4)}
        from peba1_amd import lib
        L, mrng = lib.load(), np.random.default_rng(0x30FE5)
        self.ring = U.random_ring(mrng, 2, N)
        mu = [int(x) for x in mrng.integers(PC.INT32_MIN, PC.INT32_MAX + 1, N)]
        self.cring = api.ring_encrypt(mu, self.ks[0], compressed=True, seed=0x5EED, mask_seed=SW.seed_of(0)).reshape(1, 10 + N)
        self.cring_plain = SW.ring_expand_ref(L, self.cring, N)
        self.record = api.encrypt_bits_compressed(mrng.integers(0, 2, PC.RECORD), self.ks[0], seed=0x5EEE, mask_seed=SL.MASK_SEED)
        self.record_plain = SL.expand_ref(L, self.record, n, np.arange(PC.RECORD))
        self.pk = api.PackingKey(self.ks[0], seed=0x9ACC)
        self.pk_rows = PK.KeyRows(self.pk.words())
        self.unpacked = {}

    def unpack_words(self, seeded, index, key):
        """what an unpack of these indices under key `key` writes, [len(index)][n + 1] (kept: the modes share programs)"""
        at = (seeded, tuple(index), key)
        if at not in self.unpacked:
            pp, ring = self.pp, self.cring_plain if seeded else self.ring
            self.unpacked[at] = U.keyswitch_ref(self.ks[key].ksk(), U.extract_ref(ring, index, pp.N), pp.n, pp.N, pp.ks_t, pp.ks_basebit)
        return self.unpacked[at]

    def open_device(self):
        self.luts = [self.api.Lut(self.pp, w) for w in self.lut_words]
        self.multi = self.api.LutMulti(self.luts[1], self.spec)
        import torch
        self.dring, self.dcring, self.drecord = (torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to("cuda:0")
                                                 for x in (self.ring, self.cring, self.record))
        torch.cuda.synchronize()

    def close(self):
        for x in getattr(self, "luts", []) + ([self.multi] if hasattr(self, "multi") else []):
            x.close()
        self.pk.close()
        for ks in self.ks:
            ks.close()


def replay(fx, calls, fold=False):
    """-> dict(final, observed, steps, clean, rotations, keyswitches, recorded, moves).  final: handle -> words; observed: per
    observation its words (an observe call: n + 1; an export: [count][n + 1]; a pack: (k+1) N); steps: per call the words of its results on return; clean: the handles whose value is a Boolean
    function of Boolean inputs (a decrypt claim holds).  fold: by the rule of "fold_constants" (program_common.py), for
    which the replay keeps what the rule reads -- which handles name a public constant, and which name one sample (sid:
    a new one per result, the operand's for a copy).  A moved sample is never a constant and always a sample of its own;
    an unpack's key switches run at once, one per index, and are never eliminated or shared."""
    O, oks = fx.O, fx.oks
    zero = oks[0].constant(0)
    val, const, clean, sid, steps, aliased = {}, {}, {}, {}, [], {}
    fresh_sid = iter(range(1, 1 << 30))
    for a in range(NARR):
        for i in range(PER):
            val[(a, i)] = fx.inputs[a][i].copy() if a in fx.inputs else zero.copy()
            const[(a, i)] = None if a in fx.inputs else 0              # a never-written sample is the public constant 0
            clean[(a, i)] = True
            sid[(a, i)] = next(fresh_sid) if a in fx.inputs else ("const", 0)
    observed, rot, ksw, recorded, moves = [], 0, 0, 0, dict.fromkeys(PC.MOVE_FORMS, 0)

    def gate2(name, r, a, b, k):
        nonlocal rot, ksw
        f = PC.fold_gate2(name, (const[a], const[b])) if fold else None
        ok = clean[a] and clean[b]
        if f is None:
            val[r], const[r] = oks[k].gate(name, val[a], val[b], use_ntt=2), None
            rot, ksw = rot + 1, ksw + 1
        elif f[0] == "const":
            val[r], const[r] = oks[k].constant(f[1]), f[1]
        elif f[0] == "copy":
            src = (a, b)[f[1]]
            val[r], const[r], aliased[r] = val[src].copy(), const[src], sid[src]
        else:
            bool_not(r, (a, b)[f[1]], k)
        clean[r] = ok

    def bool_not(r, a, k):
        if fold and const[a] is not None:
            val[r], const[r] = oks[k].constant(1 - const[a]), 1 - const[a]
        else:
            val[r], const[r] = oks[k].gate_not(val[a]), None

    for call in calls:
        what = call[0]
        recorded += what not in ("flush", "flush_async", "observe", "realloc") + tuple(PC.MOVE_FORMS)
        if what in PC.MOVE_FORMS:
            moves[what] += 1
        before = dict(sid)
        if what == "gate":
            gate2(*call[1:])
        elif what == "mux":
            _, r, a, b, c, k = call
            ok = clean[a] and clean[b] and clean[c]
            f = PC.fold_mux((const[a], const[b], const[c]), same_data=sid[b] == sid[c]) if fold else None
            if f is None:
                val[r], const[r] = oks[k].mux(val[a], val[b], val[c], use_ntt=2), None
                rot, ksw = rot + 2, ksw + 1
            elif f[0] == "copy":
                src = (a, b, c)[f[1]]
                val[r], const[r], aliased[r] = val[src].copy(), const[src], sid[src]
            elif f[0] == "not":
                bool_not(r, (a, b, c)[f[1]], k)
            else:
                gate2(f[1], r, (a, b, c)[f[2][0]], (a, b, c)[f[2][1]], k)
            clean[r] = ok
        elif what == "not":
            _, r, a, k = call
            ok = clean[a]
            bool_not(r, a, k)
            clean[r] = ok
        elif what == "copy":
            _, r, a, k = call
            val[r], const[r], clean[r] = val[a].copy(), const[a], clean[a]
        elif what == "const":
            _, r, v, k = call
            val[r], const[r], clean[r] = oks[k].constant(v), v, True
        elif what == "gate3":
            _, name, mask, r, a, b, c, k = call
            ok = clean[a] and clean[b] and clean[c]
            f = PC.fold_gate3(name, mask, (const[a], const[b], const[c])) if fold else None
            if f is None:
                val[r], const[r] = G3.oracle_gate3(oks[k], name, mask, val[a], val[b], val[c]), None
                rot, ksw = rot + 1, ksw + 1
            else:
                gate2(f[1], r, (a, b, c)[f[2][0]], (a, b, c)[f[2][1]], k)
            clean[r] = ok
        elif what == "lut":
            _, li, r, ins, coefs, c0, k = call
            lin = T.linear(coefs, np.stack([val[x] for x in ins]), c0)
            val[r], const[r], clean[r] = T.oracle_lut_bootstrap(O, oks[k], lin, fx.lut_words[li])[0], None, False
            rot, ksw = rot + 1, ksw + 1
        elif what == "lutm":
            _, res, ins, coefs, c0, k = call
            lin = T.linear(coefs, np.stack([val[x] for x in ins]), c0)
            acc = T.oracle_lut_bootstrap(O, oks[k], lin, fx.lut_words[1])[2]
            us = M.outputs(acc, fx.spec)
            for r, u in zip(res, us):
                if r is not None:
                    val[r], const[r], clean[r] = oks[k].keyswitch(u), None, False
                    ksw += 1
            rot += 1
        elif what == "lin":
            _, r, ins, coefs, c0, k = call
            val[r], const[r], clean[r] = T.linear(coefs, np.stack([val[x] for x in ins]), c0), None, False
        elif what == "observe":
            observed.append(val[call[1]].copy())
        elif what == "realloc":
            for i in range(PER):
                val[(call[1], i)], const[(call[1], i)], clean[(call[1], i)] = zero.copy(), 0, True
        elif what in PC.WRITER_MOVES:
            for r, w in zip(PC.writes_of(call), moved_words(fx, call, observed)):
                val[r], const[r], clean[r] = w.copy(), None, False
                sid[r] = next(fresh_sid)                         # (a handle given twice: its last value)
            ksw += len(call[3]) if what.startswith("unpack") else 0
        elif what == "export":
            observed.append(np.stack([val[x] for x in call[2]]))
        elif what == "pack":
            observed.append(PK.pack_ref(fx.pk_rows, np.stack([val[x] for x in call[2]]), fx.pk.basebit))
        # one sample per result; a copy (a folded one too) names its operand's sample, a constant the shared constant
        for r in results_of(call) if what not in PC.WRITER_MOVES else []:
            sid[r] = ("const", const[r]) if const[r] is not None else next(fresh_sid)
        if what == "copy":
            sid[call[1]] = before[call[2]]
        for r in list(aliased):                                 # a call folded to a copy
            sid[r] = aliased.pop(r)
        steps.append({r: val[r].copy() for r in results_of(call)})
    return dict(final=val, observed=observed, steps=steps, clean=clean, rotations=rot, keyswitches=ksw, recorded=recorded,
                moves=moves)


def moved_words(fx, call, observed):
    """the words a movement call writes, one row per handle it names, from the restatements alone"""
    what = call[0]
    if what == "import":
        src, count = call[3], len(call[2])
        if src[0] == "random":
            return np.random.default_rng(src[1]).integers(PC.INT32_MIN, PC.INT32_MAX + 1, (count, fx.pp.words)).astype(I32)
        return observed[src[1]].reshape(-1, fx.pp.words)[src[2]:src[2] + count]
    if what == "import_seeded":
        return fx.record_plain[call[2]]
    index = call[2] if call[2] is not None else list(range(len(call[3])))
    return fx.unpack_words(what == "unpack_seeded", index, call[4])


# ---- the device run -------------------------------------------------------------------------------------------------------------
def mirror(sample, n):
    s = sample.contents
    return np.array([s.a[i] for i in range(n)] + [s.b], dtype=I32)


def device_buffers(fx, calls, want):
    """call number -> (tensor, first word) for every call that reads or writes device memory, all made before the first
    call runs and waited for once: a wait in the middle of the program would finish the flush in flight and the
    stream-ordered transfers that the moves are there to meet.  An import of words that a device-form export of the same
    program wrote reads them where that export put them, with no host in between; any other import has its words uploaded
    here."""
    import torch
    buf, observers, nobs = {}, {}, 0
    for ci, call in enumerate(calls):
        what = call[0]
        if what == "export":
            buf[ci] = (torch.zeros(len(call[2]) * fx.pp.words, dtype=torch.int32, device="cuda:0"), 0)
        elif what == "pack" and call[1] == "device":
            buf[ci] = (torch.zeros(2 * fx.pp.N, dtype=torch.int32, device="cuda:0"), 0)
        elif what == "import" and call[1] != "host":
            src = call[3]
            if src[0] == "observed" and observers[src[1]] in buf:
                buf[ci] = (buf[observers[src[1]]][0], src[2] * fx.pp.words)
            else:
                words = np.ascontiguousarray(moved_words(fx, call, want["observed"]))
                buf[ci] = (torch.from_numpy(words.reshape(-1)).to("cuda:0"), 0)
        if what in ("observe",) + PC.OBSERVER_MOVES:
            observers[nobs] = ci
            nobs += 1
    torch.cuda.synchronize()
    return buf


def run_move(fx, L, arrs, call, buf, observed):
    """One movement call through the C API; -> what a host-form observation returned, else None.  `buf`: this call's
    (tensor, first word); `observed`: the expected observations (the words a host-form import brings back)."""
    from peba1_amd import lib
    api, pp, what, form = fx.api, fx.pp, call[0], call[1]
    at = lambda h: arrs[h[0]].at(h[1])
    ptr = C.c_void_p(buf[0].data_ptr() + 4 * buf[1]) if buf is not None else None
    if what in ("import", "export", "pack"):
        t = call[2]
        first, count = t[0], len(t)
        assert t == [(first[0], first[1] + j) for j in range(count)]
    if what == "import":
        if form == "host":
            words = np.ascontiguousarray(moved_words(fx, call, observed))
            assert L.tfhe_hip_import_samples(at(first), count, pp.ptr, words.ctypes.data_as(lib.I32P)) == 0, api.last_error()
        else:
            entry = L.tfhe_hip_import_samples_device if form == "device" else L.tfhe_hip_import_samples_device_async
            assert entry(at(first), count, pp.ptr, ptr) == 0, api.last_error()
    elif what == "export":
        entry = L.tfhe_hip_export_samples_device if form == "device" else L.tfhe_hip_export_samples_device_async
        assert entry(at(first), count, pp.ptr, ptr) == 0, api.last_error()
    elif what == "pack":
        if form == "host":
            return api.pack(fx.pk, arrs[first[0]], count, fx.ks[0], first=first[1])
        api.pack_device(fx.pk, arrs[first[0]], count, fx.ks[0], ptr.value, first=first[1])
    else:
        index, t = call[2], call[3]
        if form == "scattered":
            result, first = [at(h) for h in t], 0
        else:
            result, first = arrs[t[0][0]], t[0][1]
            assert t == [(t[0][0], first + j) for j in range(len(t))]
        if what == "import_seeded":
            if form == "device":
                api.import_seeded_device(fx.drecord.data_ptr(), PC.RECORD, pp, result, index=index, first=first)
            else:
                api.import_seeded(fx.record, pp, result, index=index, first=first)
        else:
            seeded, key = what == "unpack_seeded", fx.ks[call[4]]
            if form == "device":
                dev, entry = (fx.dcring, api.unpack_seeded_device) if seeded else (fx.dring, api.unpack_device)
                entry(dev.data_ptr(), 1 if seeded else 2, key, result, index=index, count=len(t), first=first)
            else:
                (api.unpack_seeded if seeded else api.unpack)(fx.cring if seeded else fx.ring, key, result, index=index,
                                                              count=len(t), first=first)
    return None


def run_device(fx, calls, want, immediate=False):
    """Runs the calls, checks every observation (and in immediate mode every result's host mirror on return) against
    `want`; returns (final words of every handle, statistics delta).  An observation into device memory is compared
    behind the final tfhe_hip_stream_sync, and every tensor lives until then.  Immediate mode and the mirrors of a moved
    sample, as the header has it: exact on return from an unpack and a seeded import of any form and from a host-form
    import; stale after a device-form import until the sample is synchronised, so not looked at."""
    from peba1_amd import lib
    api, pp, L = fx.api, fx.pp, lib.load()
    buffers = device_buffers(fx, calls, want) if any(c[0] in PC.MOVE_FORMS for c in calls) else {}
    later = []                                                # (observation number, call number) to compare at the end
    arrs = [api.CiphertextArray(pp, PER) for _ in range(NARR)]
    for a, w in fx.inputs.items():
        arrs[a].set_words(w)
    at = lambda h: arrs[h[0]].at(h[1])
    L.tfhe_hip_clear_error()
    before, seen = api.stats(), 0
    for ci, call in enumerate(calls):
        what = call[0]
        if what == "gate":
            getattr(L, "boots" + call[1])(at(call[2]), at(call[3]), at(call[4]), fx.ks[call[5]].cloud)
        elif what == "mux":
            L.bootsMUX(at(call[1]), at(call[2]), at(call[3]), at(call[4]), fx.ks[call[5]].cloud)
        elif what == "not":
            L.bootsNOT(at(call[1]), at(call[2]), fx.ks[call[3]].cloud)
        elif what == "copy":
            L.bootsCOPY(at(call[1]), at(call[2]), fx.ks[call[3]].cloud)
        elif what == "const":
            L.bootsCONSTANT(at(call[1]), call[2], fx.ks[call[3]].cloud)
        elif what == "gate3":
            api.gate3(call[1], at(call[3]), at(call[4]), at(call[5]), at(call[6]), fx.ks[call[7]], negate_mask=call[2])
        elif what == "lut":
            api.lut_bootstrap(fx.luts[call[1]], at(call[2]), [at(x) for x in call[3]], [PC.s32(c) for c in call[4]], PC.s32(call[5]),
                              fx.ks[call[6]])
        elif what == "lutm":
            api.lut_bootstrap_multi(fx.multi, [at(r) if r is not None else None for r in call[1]], [at(x) for x in call[2]],
                                    [PC.s32(c) for c in call[3]], call[4], fx.ks[call[5]])
        elif what == "lin":
            api.linear(at(call[1]), [at(x) for x in call[2]], call[3], call[4], fx.ks[call[5]])
        elif what == "flush":
            assert api.flush() >= 0, api.last_error()
        elif what == "flush_async":
            assert api.flush_async() >= 0, api.last_error()
        elif what == "observe":
            if call[2] == "export":
                got = np.zeros((1, pp.words), dtype=I32)
                assert L.tfhe_hip_export_samples(at(call[1]), 1, pp.ptr, got.ctypes.data_as(lib.I32P)) == 0, api.last_error()
                got = got[0]
            else:
                assert L.tfhe_hip_sync_samples(at(call[1]), 1) == 0, api.last_error()
                got = mirror(at(call[1]), pp.n)
            assert (got == want["observed"][seen]).all(), ("observation", seen, ci, call)
            seen += 1
        elif what == "realloc":
            arrs[call[1]].close()                             # its samples may hold pending results
            arrs[call[1]] = api.CiphertextArray(pp, PER)
        elif what in PC.MOVE_FORMS:
            got = run_move(fx, L, arrs, call, buffers.get(ci), want["observed"])
            if what in PC.OBSERVER_MOVES:
                if got is not None:
                    assert (got == want["observed"][seen]).all(), ("observation", seen, ci, call)
                else:
                    later.append((seen, ci))
                seen += 1
        assert api.last_error() == "", (ci, call, api.last_error())
        if immediate and not (what == "import" and call[1] != "host"):
            for r, w in want["steps"][ci].items():
                assert (mirror(at(r), pp.n) == w).all(), ("host mirror on return", ci, call)
    assert seen == len(want["observed"])
    assert L.tfhe_hip_stream_sync() == 0, api.last_error()
    for k, ci in later:
        got = buffers[ci][0].cpu().numpy().reshape(want["observed"][k].shape)
        assert (got == want["observed"][k]).all(), ("observation in device memory", k, ci, calls[ci])
    final = {(a, i): w for a in range(NARR) for i, w in enumerate(arrs[a].words())}
    now = api.stats()
    assert api.last_error() == ""
    for x in arrs:
        x.close()
    return final, {k: now[k] - before[k] for k in now}


def compare_final(final, want):
    for h, w in want["final"].items():
        assert (final[h] == w).all(), ("final words", h)


@contextlib.contextmanager
def tunings(api, deferred=True, **values):
    was = api.get_deferred()
    try:
        for name, v in dict(DEFAULTS, **values).items():
            api.set_tuning(name, v)
        api.set_deferred(deferred)
        yield
    finally:
        for name, v in DEFAULTS.items():
            api.set_tuning(name, v)
        api.set_deferred(was)


def moves_text(moves):
    return "moves " + " ".join(f"{k} {v}" for k, v in moves.items()) + ", " if sum(moves.values()) else ""


def report(mode, want, d, t0):
    print(f"[recorded programs] {mode}: calls {want['recorded']}, {moves_text(want['moves'])}flushes {d['flushes']}, rotations run {d['blind_rotates']} "
          f"of {want['rotations']} recorded, key switches {d['keyswitches']} of {want['keyswitches']}, {time.time() - t0:.2f} s")


# ---- fixtures shared by the modes: one key pair, one program and one replay for all of (a), (d) --------------------------
@pytest.fixture(scope="module")
def one_key(oracle):
    fx = Fixture(oracle)
    fx.open_device()
    yield fx
    fx.close()


@pytest.fixture(scope="module")
def program_a(one_key):
    calls = random_program(2026, 180)
    return calls, replay(one_key, calls)


@pytest.mark.parametrize("balance", [0, 1])
@pytest.mark.parametrize("eliminate", [0, 1])
@pytest.mark.parametrize("reuse", [0, 1])
def test_deferred_program_is_the_sequential_replay(one_key, program_a, reuse, eliminate, balance):
    calls, want = program_a
    t0 = time.time()
    with tunings(one_key.api, reuse_gates=reuse, eliminate_dead=eliminate, balance_levels=balance):
        final, d = run_device(one_key, calls, want)
    compare_final(final, want)
    report(f"(a) reuse {reuse} eliminate {eliminate} balance {balance}", want, d, t0)
    assert one_key.api.last_error() == ""
    if not reuse and not eliminate:
        assert d["blind_rotates"] == want["rotations"] and d["keyswitches"] == want["keyswitches"]
    else:
        assert d["blind_rotates"] <= want["rotations"] and d["keyswitches"] <= want["keyswitches"]


def test_immediate_mode_keeps_every_host_mirror_exact(one_key):
    calls = random_program(77, 60)
    want = replay(one_key, calls)
    t0 = time.time()
    with tunings(one_key.api, deferred=False):
        final, d = run_device(one_key, calls, want, immediate=True)
    compare_final(final, want)
    report("(b) immediate", want, d, t0)
    assert d["blind_rotates"] == want["rotations"]


def test_three_keys_in_one_recording(oracle):
    fx = Fixture(oracle, nkeys=3)
    try:
        fx.open_device()
        calls = random_program(303, 180, nkeys=3)
        want = replay(fx, calls)
        t0 = time.time()
        with tunings(fx.api, batch_keys=1):
            final, d = run_device(fx, calls, want)
        compare_final(final, want)
        report("(c) three keys", want, d, t0)
        assert fx.api.last_error() == ""
    finally:
        fx.close()


def test_folded_program_is_the_rule_from_truth_tables_and_decrypts_like_the_unfolded_one(one_key, program_a):
    from peba1_amd import lib
    fx, (calls, unfolded) = one_key, program_a
    want = replay(fx, calls, fold=True)
    assert want["rotations"] < unfolded["rotations"]             # the program does fold
    t0 = time.time()
    with tunings(fx.api, fold_constants=1, reuse_gates=0):      # (sharing would make two handles one sample by flush timing)
        final, d = run_device(fx, calls, want)
    compare_final(final, want)
    report("(d) fold_constants", want, d, t0)
    # decrypted bits of the Boolean results: the unfolded words (checked word for word in mode (a)) under the same key
    oks = fx.oks[0]
    checked = 0
    for h, ok in want["clean"].items():
        if ok:
            assert oks.decrypt(final[h])[0] == oks.decrypt(unfolded["final"][h])[0], h
            checked += 1
    assert checked >= 4
    assert fx.api.last_error() == ""


# ---- the same modes on programs with moves ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moves_a(one_key):
    calls = moves_program("a")
    return calls, replay(one_key, calls)


@pytest.mark.parametrize("balance", [0, 1])
@pytest.mark.parametrize("eliminate", [0, 1])
@pytest.mark.parametrize("reuse", [0, 1])
def test_deferred_program_with_moves_is_the_sequential_replay(one_key, moves_a, reuse, eliminate, balance):
    """the key switches of the unpacks run at once and are in the total whatever is eliminated or shared"""
    calls, want = moves_a
    t0 = time.time()
    with tunings(one_key.api, reuse_gates=reuse, eliminate_dead=eliminate, balance_levels=balance):
        final, d = run_device(one_key, calls, want)
    compare_final(final, want)
    report(f"(a) with moves, reuse {reuse} eliminate {eliminate} balance {balance}", want, d, t0)
    assert one_key.api.last_error() == ""
    unpacked = sum(len(c[3]) for c in calls if c[0].startswith("unpack"))
    assert unpacked > 0 and d["keyswitches"] >= unpacked
    if not reuse and not eliminate:
        assert d["blind_rotates"] == want["rotations"] and d["keyswitches"] == want["keyswitches"]
    else:
        assert d["blind_rotates"] <= want["rotations"] and d["keyswitches"] <= want["keyswitches"]


def test_immediate_mode_with_moves_keeps_every_host_mirror_exact(one_key):
    calls = moves_program("b")
    want = replay(one_key, calls)
    t0 = time.time()
    with tunings(one_key.api, deferred=False):
        final, d = run_device(one_key, calls, want, immediate=True)
    compare_final(final, want)
    report("(b) with moves, immediate", want, d, t0)
    assert d["blind_rotates"] == want["rotations"] and d["keyswitches"] == want["keyswitches"]


def test_three_keys_and_moves_in_one_recording(oracle):
    """unpacks under each of the three keys between gates of all three"""
    fx = Fixture(oracle, nkeys=3)
    try:
        fx.open_device()
        calls = moves_program("c")
        assert {c[4] for c in calls if c[0].startswith("unpack")} == {0, 1, 2}
        want = replay(fx, calls)
        t0 = time.time()
        with tunings(fx.api, batch_keys=1):
            final, d = run_device(fx, calls, want)
        compare_final(final, want)
        report("(c) with moves, three keys", want, d, t0)
        assert fx.api.last_error() == ""
        assert d["blind_rotates"] <= want["rotations"] and d["keyswitches"] <= want["keyswitches"]
    finally:
        fx.close()


def test_folded_program_with_moves_never_takes_a_moved_sample_for_a_constant(one_key, moves_a):
    fx, (calls, unfolded) = one_key, moves_a
    want = replay(fx, calls, fold=True)
    assert want["rotations"] < unfolded["rotations"]             # the program does fold
    t0 = time.time()
    with tunings(fx.api, fold_constants=1, reuse_gates=0):
        final, d = run_device(fx, calls, want)
    compare_final(final, want)
    report("(d) with moves, fold_constants", want, d, t0)
    assert fx.api.last_error() == ""


POOL_WORKER = r'''
import sys
sys.path[:0] = [%r, %r]
import test_gpu_recorded_programs as P
P.pool_worker(%r)
'''


def pool_worker(moves=False):
    from oracle import pyoracle
    from peba1_amd import api
    pyoracle.build()
    fx = Fixture(pyoracle)
    fx.open_device()
    calls = moves_program("e") if moves else random_program(55, 170)
    want = replay(fx, calls)
    final, d = run_device(fx, calls, want)
    compare_final(final, want)
    explicit = sum(c[0] in ("flush", "flush_async") for c in calls)
    assert api.last_error() == ""
    print("POOL-OK", "calls", want["recorded"], "explicit", explicit, "flushes", d["flushes"], "rotations", d["blind_rotates"],
          "recorded", want["rotations"], "moves", sum(want["moves"].values()), "keyswitches", d["keyswitches"],
          "ksrecorded", want["keyswitches"])
    fx.close()


def small_pool_run(moves):
    t0 = time.time()
    env = dict(os.environ, TFHE_HIP_POOL_SLOTS=str(POOL_SLOTS))
    out = subprocess.run([sys.executable, "-c", POOL_WORKER % (ROOT, os.path.join(ROOT, "tests"), moves)], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [x for x in out.stdout.splitlines() if x.startswith("POOL-OK")][0].split()
    f = dict(zip(line[1::2], map(int, line[2::2])))
    print(f"[recorded programs] (e) pool of {POOL_SLOTS}{' with moves' if moves else ''}: calls {f['calls']}, "
          f"{'moves %d, ' % f['moves'] if moves else ''}flushes {f['flushes']} ({f['explicit']} asked for), "
          f"rotations run {f['rotations']} of {f['recorded']} recorded, key switches {f['keyswitches']} of {f['ksrecorded']}, "
          f"{time.time() - t0:.2f} s")
    return f


def test_a_small_pool_flushes_in_the_middle_of_the_program():
    """The pool's size is read when the process starts, hence a process of its own.  With fewer than 4,096 slots free the
    recorder runs what is pending before it records the next call: far more flushes than the program asks for, the same
    words."""
    f = small_pool_run(False)
    assert f["flushes"] >= f["explicit"] + 40


# read off a run: 131 flushes with 9 asked for (the old program: 129 with 14) -- the 23 observations flush what is pending
# like the old program's, the other flushes are the recorder's own, one per recorded call that found an operation pending
SMALL_POOL_MOVES_MARGIN = 100


def test_a_small_pool_recycles_renamed_slots_in_the_middle_of_a_program_with_moves():
    """The mode in which a slot given back by a rename is taken again soonest: every recorded call that finds an operation
    pending runs it first, and the moves rename between them."""
    f = small_pool_run(True)
    assert f["flushes"] >= f["explicit"] + SMALL_POOL_MOVES_MARGIN
