// recorder.cpp -- see recorder.hpp.  Host logic only: no gate arithmetic happens here.
#include "recorder.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "op_graph.hpp"

namespace tfhe_hip {
namespace {

// truth tables of the two-input gates, index [gate code][2 a + b] (enum TfheHipGate; GATE_LIN's signs say the same)
const uint8_t GATE_TT[10][4] = {
    {1, 1, 1, 0}, {0, 1, 1, 1}, {0, 0, 0, 1}, {1, 0, 0, 0}, {0, 1, 1, 0}, {1, 0, 0, 1},
    {0, 1, 0, 0}, {0, 0, 1, 0}, {1, 1, 0, 1}, {1, 0, 1, 1},
};

struct Recorder {
    std::recursive_mutex mtx;
    // Default: deferred.  The reference (and any caller that stays inside the tfhe C API) never reads a field of LweSample
    // -- results are only ever observed through bootsSymDecrypt or an export, and both run the pending gates first -- so
    // recording is transparent to it and is what lets an UNMODIFIED caller run at batch throughput (one gate per launch is
    // 3.4 ms: 290 gates/s).  TFHE_HIP_DEFERRED=0 / tfhe_hip_set_deferred(0) restores strict per-call completion with the
    // host mirror (a, b) refreshed on return, as upstream's own struct has it.
    bool deferred = true;
    // cloud keys of the pending operations (PendingOp::key indexes this list) and the key of the op being recorded.  One
    // key unless batch_keys is on; several keys always share one parameter set, hence one slot pool
    std::vector<const TFheGateBootstrappingCloudKeySet *> keys;
    uint16_t cur_key = 0;
    SlotPool *pool = nullptr;
    // Multi-key flushes (OPT-IN: tuning "batch_keys", env TFHE_HIP_BATCH_KEYS).  Off: a gate under another cloud key than the
    // pending ones flushes them first (one flush per key).  On: gates under different keys of the SAME parameter set stay
    // recorded together and run as one level sequence, each rotation and key switch under its own gate's key -- K clients'
    // circuits fill the levels of one flush instead of running as K narrow flushes.  A key of another parameter set still
    // flushes.  Results are the same words either way.
    bool batch_keys = false;
    // the pending ops, their one index (tuning "reuse_gates": OpGraph::reuse) and the NOT-origin table (op_graph.hpp)
    OpGraph<SlotPool> graph;
    bool balance_levels = true;   // slack-aware level filling (scheduler.hpp)
    // the cost-driven pass behind it (scheduler.cpp relevel_by_cost; tuning "level_slack", env TFHE_HIP_LEVEL_SLACK): on,
    // a flush whose parameter set, card and tunings have a measured cost table (launch_plan.hpp level_cost_table) moves
    // gates with slack off the table's cost steps; off, or no table: the list scheduling's levels
    bool level_slack = true;
    // a table set by hand (tfhe_hip_test_set_level_cost) stands in for the compiled-in ones, whatever the parameter set
    std::vector<int32_t> cost_width;
    std::vector<double> cost_us;
    LevelSlackReport last_slack;
    // operations of a flush launched without waiting (tfhe_hip_flush_async): released when it is complete
    std::vector<PendingOp> flight_ops;
    std::vector<LinTerm> flight_terms;      // the term table its linear combinations name
    SlotPool *flight_pool = nullptr;
    std::vector<const TFheGateBootstrappingCloudKeySet *> flight_keys;   // keys it runs under: not deleted before it completes
    bool eliminate_dead = true;   // dead-op elimination at flush (OpGraph::eliminate_dead)
    // Constant folding at record time (round 6; OPT-IN: tuning "fold_constants", env TFHE_HIP_FOLD_CONSTANTS).  A trivial
    // sample -- bootsCONSTANT, a fresh sample, a copy of either -- is a PUBLIC constant, and a gate with such an operand
    // needs no bootstrap to be evaluated: its result is a constant, the other operand, or its negation (linear); a MUX with
    // a constant data operand is a two-input gate.  The reference's circuits are full of them (zero-padded partial products,
    // adders fed with constant zeros: 62 % of the 215,544 gates of a 128-slot Function_f).  Decrypted results are the
    // same; the CIPHERTEXTS are not what TFHE produces (it bootstraps every gate whatever its operands), which is why this is
    // off by default -- the drop-in's contract is TFHE's words.  The oracle's provider folds by the same rule
    // (oracle/boots_oracle.c orc_boots_set_fold), so folded circuits have oracle digests of their own.
    bool fold_constants = false;
};
Recorder &rec() {
    static Recorder r;
    static bool init = [] {
        if (const char *e = std::getenv("TFHE_HIP_DEFERRED")) r.deferred = std::atoi(e) != 0;
        if (const char *e = std::getenv("TFHE_HIP_FOLD_CONSTANTS")) r.fold_constants = std::atoi(e) != 0;   // opt-in (Recorder)
        if (const char *e = std::getenv("TFHE_HIP_BATCH_KEYS")) r.batch_keys = std::atoi(e) != 0;           // opt-in (Recorder)
        if (const char *e = std::getenv("TFHE_HIP_LEVEL_SLACK")) r.level_slack = std::atoi(e) != 0;
        return true;
    }();
    (void)init;
    return r;
}

void release_refs(SlotPool *pool, const PendingOp &op, const LinTerm *terms) {    // the pending references an op holds
    for_each_src(op, terms, [&](int32_t s) { pool->release(s); });
    for_each_dst(op, [&](int32_t d) { pool->release(d); });
}

// "Same parameter set" for a multi-key flush: every field that evaluation reads, by VALUE (two separately allocated sets
// with equal numbers are one set).  execute() runs all rotations of a flush with the DevParams, form rules and extract
// stride of its first key, so a key that differs in any of these must not join; sharing a slot pool is not enough, pools
// are matched on n alone (Engine::find_pool).  The three noise deviations are left out: they shape key generation and
// encryption only, no kernel and no launch rule reads them.
bool same_evaluation_params(const Params &a, const Params &b) {
    return a.n == b.n && a.N == b.N && a.k == b.k && a.l == b.l && a.Bgbit == b.Bgbit && a.ks_t == b.ks_t &&
           a.ks_basebit == b.ks_basebit;
}

// begin_op for a key other than the last op's: the recording's key list gains it, or the pending ops run first
void select_key(const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    auto known = std::find(r.keys.begin(), r.keys.end(), bk);
    if (known == r.keys.end() && !r.graph.ops().empty()) {
        // a key the recording does not hold yet: one more key of the flush (batch_keys, same parameter set) or a flush.
        // Every key of the list passed this test against the first, so comparing with the first compares with all
        if (!r.batch_keys || pool_of_key(bk) != r.pool || !same_evaluation_params(bk->bk->p, r.keys.front()->bk->p))
            flush_locked();
    }
    if (r.graph.ops().empty()) r.keys.clear();            // nothing pending: the list starts afresh with this key
    known = std::find(r.keys.begin(), r.keys.end(), bk);
    if (known == r.keys.end()) {
        if (r.keys.size() > UINT16_MAX) flush_locked();   // (PendingOp::key) -- a flush empties the list below
        if (r.graph.ops().empty()) r.keys.clear();
        r.keys.push_back(bk);
        known = r.keys.end() - 1;
    }
    r.cur_key = (uint16_t)(known - r.keys.begin());
}

void begin_op(const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    if (r.keys.empty() || r.keys[r.cur_key] != bk) select_key(bk);
    r.pool = pool_of_key(bk);
    // pending operations pin their slots until they run: flush before the pool runs dry, so
    // arbitrarily long recordings need only bounded device memory
    if (!r.graph.ops().empty() && r.pool->capacity() - r.pool->in_use() < 4096) flush_locked();
}

// the one tail of every record: immediate mode runs the op and refreshes the host mirrors, as upstream has them on return
void finish_op(LweSample *const *result, int count) {
    if (rec().deferred) return;
    flush_locked();
    for (int m = 0; m < count; ++m)
        if (result[m]) sync_sample_locked(result[m]);
}

// result becomes (a handle of) `slot`: a COPY
void point_at(LweSample *result, SlotPool *pool, int32_t slot) {
    pool->retain(slot);
    repoint(result, pool, slot);
    finish_op(&result, 1);
}

// 0 / 1 if `slot` is one of the pool's shared trivial samples (a public constant), else -1
int const_bit(const SlotPool *pool, int32_t slot) { return slot == pool->const_slot[0] ? 0 : slot == pool->const_slot[1] ? 1 : -1; }

PendingOp make_op(int kind, int32_t a, int32_t b, int32_t c) {    // two-input gates: c = -1; NOT: b = c = -1
    PendingOp op{};
    op.kind = (uint8_t)kind; op.dst = -1; op.a = a; op.b = b; op.c = c;
    return op;
}
PendingOp make_lut_op(int kind, SlotPool *pool, int32_t lut, int nin, const LweSample *const *in, const int32_t *coef, int32_t c0) {
    int32_t slot[3] = {-1, -1, -1};
    for (int i = 0; i < nin; ++i) slot[i] = ensure_slot(in[i], pool);
    PendingOp op = make_op(kind, slot[0], slot[1], slot[2]);
    op.lut = lut;
    op.sa = coef[0]; op.sb = nin > 1 ? coef[1] : 0; op.sc = nin > 2 ? coef[2] : 0;
    op.c0 = c0;
    return op;
}

// The one record path: the graph shares, widens or appends the op (op_graph.hpp) for the outputs with a result sample
// (result[m] non-null; a single-destination op has result[0] alone), and the handles are re-pointed at what it reports.
void record_op(PendingOp op, LweSample *const *result, const LinTerm *lin = nullptr) {
    Recorder &r = rec();
    SlotPool *pool = r.pool;
    op.key = r.cur_key;
    const int nout = op_outputs(op);
    unsigned wanted = 0;
    for (int m = 0; m < nout; ++m) wanted |= (result[m] ? 1u : 0u) << m;
    int32_t out[4];
    if (r.graph.record(*pool, op, wanted, [pool](int) { return alloc_slot(pool); }, out, lin) >= 0) ++Engine::get().stats.reused_gates;
    for (int m = 0; m < nout; ++m)
        if (result[m]) repoint(result[m], pool, out[m]);
    finish_op(result, nout);
}

}  // namespace

std::unique_lock<std::recursive_mutex> recorder_lock() { return std::unique_lock<std::recursive_mutex>(rec().mtx); }

SlotPool *pool_of_key(const TFheGateBootstrappingCloudKeySet *bk) {
    if (!bk || !bk->bk) api_fail("null cloud key");
    // keysets made host-only or loaded from a file get their device image at first use
    // (aborts with a clear message when there is no GPU: gates are never evaluated on the CPU)
    // (a device-expanded keyset holds seed and bodies only: its masks are made on the card)
    if (!bk->bk->dev)
        bk->bk->dev = bk->bk->mask_seed.empty() ? Engine::get().upload_key(*bk->bk) : Engine::get().upload_compressed_key(*bk->bk);
    return Engine::get().pool_for(bk->bk->p);
}

// a fresh slot; when the pool is dry, the pending operations (which pin their operands and
// results) are run first.  Throws ApiError if that frees nothing.
int32_t alloc_slot(SlotPool *pool) {
    Recorder &r = rec();
    if (pool->in_use() == pool->capacity()) {
        finish_flight_locked();                          // a completed asynchronous flush still pins its slots
        if (pool->in_use() == pool->capacity() && !r.graph.ops().empty() && r.pool == pool) flush_locked();
    }
    return pool->alloc();
}

int32_t ensure_slot(const LweSample *cs, SlotPool *pool) {
    auto *s = const_cast<LweSample *>(cs);
    bind_pool(cs, pool);
    if (s->slot >= 0) return s->slot;
    if (s->slot == SLOT_ZERO) {
        pool->retain(pool->const_slot[0]);
        s->slot = pool->const_slot[0];
        return s->slot;
    }
    const int32_t slot = alloc_slot(pool);
    Engine::get().write_slot(pool, slot, s->a, s->b);
    s->slot = slot;
    return slot;
}

void repoint(LweSample *s, SlotPool *pool, int32_t slot) {
    bind_pool(s, pool);
    if (s->slot >= 0) pool->release(s->slot);
    s->slot = slot;
}

void sync_sample_locked(const LweSample *cs) {
    Recorder &r = rec();
    auto *s = const_cast<LweSample *>(cs);
    if (s->slot < 0) return;                       // host mirror is authoritative (fresh: trivial 0)
    SlotPool *pool = pool_of_sample(s);
    // pending = written by a recorded operation that has not run (a gate, or a NOT riding on
    // level 0 of an already materialised operand)
    if (pool->pending[s->slot] && !r.graph.ops().empty()) flush_locked();
    Engine::get().read_slot(pool, s->slot, s->a, &s->b);
}

void record_gate2_locked(int code, LweSample *result, const LweSample *ca, const LweSample *cb,
                         const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);                  // refuse a foreign / mismatched result before anything changes
    const int32_t sa = ensure_slot(ca, pool), sb = ensure_slot(cb, pool);
    if (r.fold_constants) {
        const int ka = const_bit(pool, sa), kb = const_bit(pool, sb);
        if (ka >= 0 || kb >= 0) {
            // the gate as a function of its non-constant operand x: f(0), f(1)
            const uint8_t *tt = GATE_TT[code];
            const int f0 = ka >= 0 ? tt[2 * ka + (kb >= 0 ? kb : 0)] : tt[kb];
            const int f1 = ka >= 0 ? tt[2 * ka + (kb >= 0 ? kb : 1)] : tt[2 + kb];
            ++Engine::get().stats.folded_gates;
            if (f0 == f1) return point_at(result, pool, pool->const_slot[f0]);          // a constant
            if (f0 == 0) return point_at(result, pool, ka >= 0 ? sb : sa);                // x itself
            return record_not_locked(result, ka >= 0 ? cb : ca, bk);                      // NOT x: linear, no bootstrap
        }
    }
    record_op(make_op(code, sa, sb, -1), &result);
}

void record_not_locked(LweSample *result, const LweSample *ca, const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);
    const int32_t sa = ensure_slot(ca, pool);
    if (r.fold_constants && const_bit(pool, sa) >= 0)             // NOT of a public constant is the other constant
        return point_at(result, pool, pool->const_slot[1 - const_bit(pool, sa)]);
    // NOT of a still-pending NOT: -(-x) = x exactly, so alias the original operand; two NOTs
    // of one level would otherwise sit in the same launch and race
    if (r.graph.not_origin(sa) >= 0) return point_at(result, pool, r.graph.not_origin(sa));
    record_op(make_op(OP_NOT, sa, -1, -1), &result);
}

void record_mux_locked(LweSample *result, const LweSample *a, const LweSample *b, const LweSample *c,
                       const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);
    const int32_t sa = ensure_slot(a, pool), sb = ensure_slot(b, pool), sc = ensure_slot(c, pool);
    if (r.fold_constants) {
        const int ka = const_bit(pool, sa), kb = const_bit(pool, sb), kc = const_bit(pool, sc);
        if (ka >= 0 || kb >= 0 || kc >= 0 || sb == sc) {
            ++Engine::get().stats.folded_gates;
            if (ka >= 0) return point_at(result, pool, ka ? sb : sc);                     // a constant selector picks an operand
            if (sb == sc) return point_at(result, pool, sb);                                // both data operands the same sample
            if (kb >= 0 && kc >= 0) {                                                       // (kb != kc here)  MUX(a, 1, 0) = a, MUX(a, 0, 1) = NOT a
                if (kb == 1) return point_at(result, pool, sa);
                return record_not_locked(result, a, bk);
            }
            // one constant data operand: a two-input gate, one blind rotation instead of two
            if (kc >= 0) return record_gate2_locked(kc == 0 ? TFHE_HIP_AND : TFHE_HIP_ORNY, result, a, b, bk);   // a & b | !a | b
            return record_gate2_locked(kb == 0 ? TFHE_HIP_ANDNY : TFHE_HIP_OR, result, a, c, bk);               // !a & c | a | c
        }
    }
    record_op(make_op(OP_MUX, sa, sb, sc), &result);
}

// Three-input gates (tfhe_hip_gate3): gate = enum TfheHipGate3, bit i of negate_mask negates operand i.  The operands are
// recorded in slot order with their mask bits (the prelude's sum commutes word for word), so the same gate of the same
// samples in another order shares the pending result.
void record_gate3_locked(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b,
                         const LweSample *c, const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);
    struct Operand { int32_t slot; int neg; const LweSample *sample; };
    Operand in[3] = {{ensure_slot(a, pool), negate_mask & 1, a}, {ensure_slot(b, pool), (negate_mask >> 1) & 1, b},
                     {ensure_slot(c, pool), (negate_mask >> 2) & 1, c}};
    if (r.fold_constants) {
        int nconst = 0, which = -1;
        for (int i = 0; i < 3; ++i)
            if (const_bit(pool, in[i].slot) >= 0) { ++nconst; which = i; }
        if (nconst > 0) {
            // one constant operand v: the two-input gate of the other two, x and y, with the same truth table --
            // MAJ3 -> AND (v = 0) / OR (v = 1), XOR3 -> XOR / XNOR -- the negations carried into its variant.  More
            // constants: that gate folds again by its own rule (and counts the fold there)
            const int v = const_bit(pool, in[which].slot) ^ in[which].neg;
            const Operand &x = in[which == 0 ? 1 : 0], &y = in[which == 2 ? 1 : 2];
            int code;
            if (gate == TFHE_HIP_MAJ3) {
                static const int AND_CODE[4] = {TFHE_HIP_AND, TFHE_HIP_ANDNY, TFHE_HIP_ANDYN, TFHE_HIP_NOR};
                static const int OR_CODE[4] = {TFHE_HIP_OR, TFHE_HIP_ORNY, TFHE_HIP_ORYN, TFHE_HIP_NAND};
                code = (v ? OR_CODE : AND_CODE)[x.neg + 2 * y.neg];
            } else {
                const int odd = v ^ x.neg ^ y.neg ^ (gate == TFHE_HIP_XNOR3 ? 1 : 0);
                code = odd ? TFHE_HIP_XNOR : TFHE_HIP_XOR;
            }
            if (nconst == 1) ++Engine::get().stats.folded_gates;
            return record_gate2_locked(code, result, x.sample, y.sample, bk);
        }
    }
    if (in[1].slot < in[0].slot) std::swap(in[0], in[1]);
    if (in[2].slot < in[1].slot) std::swap(in[1], in[2]);
    if (in[1].slot < in[0].slot) std::swap(in[0], in[1]);
    const int mask = in[0].neg | in[1].neg << 1 | in[2].neg << 2;
    record_op(make_op(OP_GATE3 + 8 * gate + mask, in[0].slot, in[1].slot, in[2].slot), &result);
}

// Programmable bootstrap (tfhe_hip_lut_bootstrap): t = (0, c0) + sum coef[i] in[i] from test polynomial `lut` of the engine's
// table.  Never folded: a trivial operand is bootstrapped like any other (the result depends on the test polynomial, which
// the folding rules know nothing about).
void record_lut_locked(int32_t lut, LweSample *result, int nin, const LweSample *const *in, const int32_t *coef, int32_t c0,
                       const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);
    record_op(make_lut_op(OP_LUT, pool, lut, nin, in, coef, c0), &result);
}

// Multi-output programmable bootstrap (tfhe_hip_lut_bootstrap_multi): ONE op with up to four destinations -- the
// outputs of extract spec `spec` (nout of them) that the caller wants (result[m] non-null), each renamed to a fresh slot
// like a gate's result; all become available at the op's level.
void record_lutm_locked(int32_t lut, int32_t spec, int nout, LweSample *const *result, int nin, const LweSample *const *in,
                        const int32_t *coef, int32_t c0, const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    for (int m = 0; m < nout; ++m)
        if (result[m]) bind_pool(result[m], pool);      // refuse a foreign / mismatched result before anything changes
    PendingOp op = make_lut_op(OP_LUTM, pool, lut, nin, in, coef, c0);
    op.spec = spec; op.nout = nout;
    record_op(op, result);
}

// Linear combination (tfhe_hip_linear): result = (0, c0) + sum coef[i] in[i], nin in 1..LIN_MAX_IN (checked by the caller).
// No bootstrap and no key: bk names the parameter set and the pool.  Never folded, never shared; the graph replaces
// operands that pending NOTs write (op_graph.hpp).
void record_linear_locked(LweSample *result, int nin, const LweSample *const *in, const int32_t *coef, int32_t c0,
                          const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    SlotPool *pool = r.pool;
    bind_pool(result, pool);                                   // refuse a foreign / mismatched sample before anything changes
    for (int i = 0; i < nin; ++i) bind_pool(in[i], pool);
    LinTerm terms[LIN_MAX_IN];
    for (int i = 0; i < nin; ++i) terms[i] = LinTerm{ensure_slot(in[i], pool), coef[i]};
    PendingOp op = make_op(OP_LIN, -1, -1, -1);
    op.nout = nin;
    op.c0 = c0;
    record_op(op, &result, terms);
}

// something the recorded ops name by index is about to be deleted: run the recording (or finish the flight) if one does
template <typename Names>
static void run_if_named(Names names) {
    Recorder &r = rec();
    if (std::any_of(r.graph.ops().begin(), r.graph.ops().end(), names)) flush_locked();
    else if (std::any_of(r.flight_ops.begin(), r.flight_ops.end(), names)) finish_flight_locked();
}
void forget_lutm_locked(int32_t lut, int32_t spec) {
    run_if_named([=](const PendingOp &op) { return op.kind == OP_LUTM && (op.spec == spec || op.lut == lut); });
}
void forget_lut_locked(int32_t lut) {
    run_if_named([=](const PendingOp &op) { return op.kind == OP_LUT && op.lut == lut; });
}

void record_constant_locked(LweSample *result, int32_t value, const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    bind_pool(result, r.pool);          // refuse before anything changes
    const int32_t s = r.pool->const_slot[value ? 1 : 0];
    r.pool->retain(s);
    repoint(result, r.pool, s);
    if (!r.deferred) {   // keep the host mirror exact without a device round trip
        std::memset(result->a, 0, (size_t)bk->params->in_out_params->n * sizeof(Torus32));
        result->b = value ? (1 << 29) : -(1 << 29);
    }
}

void record_copy_locked(LweSample *result, const LweSample *ca, const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    begin_op(bk);
    if (result == ca) return;
    bind_pool(result, r.pool);
    const int32_t s = ensure_slot(ca, r.pool);
    r.pool->retain(s);
    repoint(result, r.pool, s);
    if (!r.deferred) sync_sample_locked(result);
}

void finish_flight_locked() {
    Recorder &r = rec();
    Engine::get().wait_flight();
    for (const PendingOp &op : r.flight_ops) release_refs(r.flight_pool, op, r.flight_terms.data());
    r.flight_ops.clear();
    r.flight_terms.clear();
    r.flight_pool = nullptr;
    r.flight_keys.clear();
}

int flush_locked(bool wait) {
    Recorder &r = rec();
    if (!r.graph.ops().empty() && r.eliminate_dead) Engine::get().stats.dead_gates += r.graph.eliminate_dead(*r.pool);
    if (r.graph.ops().empty()) { if (wait) finish_flight_locked(); return 0; }
    SlotPool *pool = r.pool;
    const std::vector<PendingOp> &ops = r.graph.ops();
    // level of every op: ASAP, or slack-aware balanced (same depth, fuller narrow levels)
    std::vector<int32_t> lvl, alap;
    LevelCost cost;                                                 // unknown unless ...
    if (r.level_slack && !r.cost_width.empty()) {
        cost = LevelCost{r.cost_width.data(), r.cost_us.data(), (int)r.cost_width.size(), 0};
    } else if (r.level_slack) {                                     // ... measured for this set, card and tunings
        const DevParams &dp = r.keys[ops[0].key]->bk->dev->dp;      // (the keys of a flush share one parameter set)
        cost = level_cost_table(LevelCostSet{dp.n, dp.N, dp.k, dp.l, dp.Bgbit, dp.ks_t, dp.ks_basebit}, Engine::get().cu_count(),
                                Engine::get().tunings);
    }
    const int levels = schedule_levels(ops, r.graph.max_level(), r.balance_levels, Engine::get().cu_count(), lvl, &alap, r.graph.terms(),
                                       &cost, &r.last_slack);
    r.last_slack.pool_slots = (long long)pool->in_use();           // slots are taken at record time: the flush's peak
    if (const char *trace = std::getenv("TFHE_HIP_TRACE_DAG")) {      // diagnostic: per op "kind asap alap level dst a b c" (slots)
        if (FILE *f = std::fopen(trace, "w")) {
            for (size_t i = 0; i < ops.size(); ++i)
                std::fprintf(f, "%d %d %d %d %d %d %d %d\n", (int)ops[i].kind, ops[i].level, alap[i], lvl[i],
                             ops[i].dst, ops[i].a, ops[i].b, ops[i].c);
            std::fclose(f);
        }
    }
    // the keys the ops use, in list order (a flush in the middle of recording an op can leave keys of no pending op)
    std::vector<int32_t> remap(r.keys.size(), -1);
    for (const PendingOp &op : ops) remap[op.key] = 0;
    std::vector<const TFheGateBootstrappingCloudKeySet *> used;
    std::vector<const DeviceKeyImage *> images;
    for (size_t k = 0; k < r.keys.size(); ++k)
        if (remap[k] == 0) { remap[k] = (int32_t)used.size(); used.push_back(r.keys[k]); images.push_back(r.keys[k]->bk->dev); }
    LevelPlan plan;
    if (used.size() == r.keys.size()) {
        plan = build_level_plan(ops, lvl, levels, (int)used.size(), r.graph.terms());
    } else {
        std::vector<PendingOp> rekeyed = ops;
        for (PendingOp &op : rekeyed) op.key = (uint16_t)remap[op.key];
        plan = build_level_plan(rekeyed, lvl, levels, (int)used.size(), r.graph.terms());
    }
    // everything above -- elimination, levelling, the plan -- ran while the device was busy with the previous asynchronous
    // flush, if any; execute() would wait for it first anyway
    finish_flight_locked();
    Engine::get().execute(images, pool, std::move(plan), wait);    // throws before anything runs, or runs it all
    for (const PendingOp &op : ops) {
        for_each_dst(op, [&](int32_t d) {
            pool->level[d] = 0;           // a later recording reads these slots as inputs: the stream orders it behind
            pool->pending[d] = 0;
        });
        if (wait) release_refs(pool, op, r.graph.terms());
    }
    if (!wait) { r.flight_pool = pool; r.flight_keys = std::move(used); }
    r.graph.clear(wait ? nullptr : &r.flight_ops, wait ? nullptr : &r.flight_terms);
    return levels;
}

void flush_pending_locked(bool wait) { if (!rec().graph.ops().empty()) flush_locked(wait); }

void forget_key_locked(const TFheGateBootstrappingCloudKeySet *bk) {
    Recorder &r = rec();
    const bool pending = std::find(r.keys.begin(), r.keys.end(), bk) != r.keys.end();
    const bool flying = std::find(r.flight_keys.begin(), r.flight_keys.end(), bk) != r.flight_keys.end();
    // the whole recording runs (gates of the other keys too), and a flush in flight under the key completes
    if (pending || flying) { flush_locked(); r.keys.clear(); }
}

bool deferred_mode() { return rec().deferred; }

bool set_deferred_locked(bool on) { return std::exchange(rec().deferred, on); }

bool set_batch_keys_locked(bool on) { return std::exchange(rec().batch_keys, on); }

void set_level_cost_locked(const int32_t *widths, const double *us, int count) {
    Recorder &r = rec();
    r.cost_width.assign(widths, widths + count);
    r.cost_us.assign(us, us + count);
}

void last_level_slack_locked(double *out4) {
    const LevelSlackReport &s = rec().last_slack;
    out4[0] = s.us_before; out4[1] = s.us_after; out4[2] = (double)s.moved; out4[3] = (double)s.pool_slots;
}

bool set_recorder_tuning_locked(const char *name, bool on) {
    Recorder &r = rec();
    bool *knob = std::strcmp(name, "reuse_gates") == 0      ? &r.graph.reuse
                 : std::strcmp(name, "level_slack") == 0    ? &r.level_slack
                 : std::strcmp(name, "eliminate_dead") == 0 ? &r.eliminate_dead
                 : std::strcmp(name, "fold_constants") == 0 ? &r.fold_constants
                 : std::strcmp(name, "balance_levels") == 0 ? &r.balance_levels
                 : std::strcmp(name, "batch_keys") == 0     ? &r.batch_keys
                                                            : nullptr;
    if (knob) *knob = on;
    return knob != nullptr;
}

}  // namespace tfhe_hip
