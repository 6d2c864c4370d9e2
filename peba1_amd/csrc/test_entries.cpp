// test_entries.cpp -- the entries of the C ABI that exist for the tests and the cost tools (include/tfhe_hip.h): the
// tfhe_hip_test_* hooks into the planners, the scheduler and the allocator, and the tfhe_hip_kernel_* raw launches of single
// kernels.  Nothing here is on a caller's path.  Compiled as part of shim.cpp's object (shim_internal.hpp).
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <numeric>
#include <vector>

#include "br_forms.hpp"
#include "op_graph.hpp"
#include "scheduler.hpp"
#include "shim_internal.hpp"

using namespace tfhe_hip;

extern "C" {

void tfhe_hip_test_chacha20_block(const uint32_t *key8, uint64_t counter, const uint32_t *nonce2, uint32_t *out16) {
    Rng::chacha_block(key8, counter, nonce2, out16);
}

void tfhe_hip_test_set_alloc_cap(int64_t bytes) {
    auto g = recorder_lock();
    set_alloc_cap((long long)bytes);
}

int64_t tfhe_hip_test_alloc_held(void) {
    auto g = recorder_lock();
    return (int64_t)alloc_held();
}

int tfhe_hip_test_stage_place(int64_t pos, int64_t capacity, int32_t outstanding, int64_t bytes, int64_t *out4) {
    if (pos < 0 || capacity < 0 || bytes < 0 || !out4) { set_error("test_stage_place: bad arguments"); return -1; }
    const StagePlace p = stage_place((size_t)pos, (size_t)capacity, outstanding != 0, (size_t)bytes);
    out4[0] = (int64_t)p.offset; out4[1] = p.wait ? 1 : 0; out4[2] = (int64_t)p.capacity; out4[3] = (int64_t)p.next;
    return 0;
}

int tfhe_hip_test_form_admissible(int form, int32_t N, int32_t l, int32_t Bgbit, int tables) {
    return br_form_admissible(form, N, l, Bgbit, tables) ? 1 : 0;
}

int tfhe_hip_test_ntt_bounds(int32_t logn, double x0, double *fwd2, int32_t *plan25, double *inv_out) {
    if (logn < 9 || logn > 11 || !(x0 >= 0) || !fwd2 || !plan25 || !inv_out) { set_error("test_ntt_bounds: bad arguments"); return -1; }
    fwd2[0] = pack_forward_bound(logn, x0);
    fwd2[1] = br_forms_detail::forward_bound(logn, x0 / (double)NTT_P[1], false);
    const InvPlanWords pl = inv_plan_words(logn);
    plan25[0] = pl.nsteps;
    for (int k = 0; k < 12; ++k) { plan25[1 + k] = pl.fan[k]; plan25[13 + k] = pl.renorm[k]; }
    *inv_out = pl.out_bound;
    return 0;
}

static int test_build_ops(const int32_t *ops5, int32_t count, std::vector<PendingOp> &ops) {
    // ops5[i] = {kind, dst, a, b, c}; ASAP levels are derived here exactly as the recorder derives them
    for (int32_t i = 0; i < count; ++i)
        if (!op_kind_valid(ops5[5 * (size_t)i])) { set_error("test schedule: unknown op kind"); return -1; }
    ops.resize((size_t)count);
    std::vector<int32_t> slot_level;
    int depth = 0;
    auto level_of = [&](int32_t s) { return s >= 0 && (size_t)s < slot_level.size() ? slot_level[s] : 0; };
    for (int32_t i = 0; i < count; ++i) {
        const int32_t *o = ops5 + 5 * (size_t)i;
        PendingOp op{(uint8_t)o[0], o[1], o[2], o[3], o[4], 0};
        const int32_t in = std::max(level_of(op.a), std::max(level_of(op.b), level_of(op.c)));
        op.level = op.kind == OP_NOT ? in : in + 1;
        if ((size_t)op.dst >= slot_level.size()) slot_level.resize((size_t)op.dst + 1, 0);
        slot_level[op.dst] = op.level;
        depth = std::max(depth, op.level);
        ops[i] = op;
    }
    return depth;
}

int tfhe_hip_test_schedule(const int32_t *ops5, int32_t count, int32_t unit, int32_t balance, int32_t *levels_out) {
    std::vector<PendingOp> ops;
    const int depth = test_build_ops(ops5, count, ops);
    if (depth < 0) return -1;
    std::vector<int32_t> lvl;
    const int d = schedule_levels(ops, depth, balance != 0, unit, lvl);
    for (int32_t i = 0; i < count; ++i) levels_out[i] = lvl[i];
    return d;
}

int tfhe_hip_test_level_slack(const int32_t *ops5, int32_t count, int32_t unit, int32_t level_slack, const int32_t *cost_widths,
                              const double *cost_us, int32_t ncost, int32_t period, int32_t *levels_out, int32_t *widths_out,
                              double *cost_out2) {
    if (!ops5 || count < 0 || unit < 1 || ncost < 0 || period < 0 || (ncost > 0 && (!cost_widths || !cost_us)) || !levels_out || !widths_out ||
        !cost_out2) {
        set_error("test_level_slack: bad arguments");
        return -1;
    }
    for (int32_t j = 0; j < ncost; ++j)
        if (cost_widths[j] < 1 || (j > 0 && cost_widths[j] <= cost_widths[j - 1]) || !(cost_us[j] >= 0)) {
            set_error("test_level_slack: the table's widths must ascend from 1 on, its costs must not be negative");
            return -1;
        }
    std::vector<PendingOp> ops;
    const int depth = test_build_ops(ops5, count, ops);
    if (depth < 0) return -1;
    std::vector<int32_t> lvl;
    const LevelCost table{cost_widths, cost_us, ncost, period}, none;
    LevelSlackReport report;
    schedule_levels(ops, depth, true, unit, lvl, nullptr, nullptr, level_slack ? &table : &none, &report);
    std::fill(widths_out, widths_out + depth + 1, 0);
    for (int32_t i = 0; i < count; ++i) {
        levels_out[i] = lvl[i];
        widths_out[lvl[i]] += op_rotations(ops[i]);
    }
    cost_out2[0] = cost_out2[1] = 0;
    for (int L = 1; L <= depth; ++L) cost_out2[0] += level_cost_at(table, widths_out[L]);
    // the sum without the pass: the pass reports it when it ran, else the levels are those
    cost_out2[1] = report.moved ? report.us_before : cost_out2[0];
    return depth;
}

int tfhe_hip_test_level_cost(int32_t n, int32_t N, int32_t k, int32_t l, int32_t Bgbit, int32_t ks_t, int32_t ks_basebit,
                             int32_t cu_count, int32_t width, double *us_out) {
    if (!us_out) { set_error("test_level_cost: null output"); return -1; }
    *us_out = level_cost_us(width, LevelCostSet{n, N, k, l, Bgbit, ks_t, ks_basebit}, cu_count, LaunchTunings{});
    return 0;
}

int tfhe_hip_test_set_level_cost(const int32_t *cost_widths, const double *cost_us, int32_t ncost) {
    if (ncost < 0 || (ncost > 0 && (!cost_widths || !cost_us))) { set_error("test_set_level_cost: bad arguments"); return -1; }
    for (int32_t j = 0; j < ncost; ++j)
        if (cost_widths[j] < 1 || (j > 0 && cost_widths[j] <= cost_widths[j - 1]) || !(cost_us[j] >= 0)) {
            set_error("test_set_level_cost: the table's widths must ascend from 1 on, its costs must not be negative");
            return -1;
        }
    auto g = recorder_lock();
    set_level_cost_locked(cost_widths, cost_us, ncost);
    return 0;
}

int tfhe_hip_last_level_slack(double *out4) {
    if (!out4) { set_error("last_level_slack: null output"); return -1; }
    auto g = recorder_lock();
    last_level_slack_locked(out4);
    return 0;
}

// rot_words = 6: the two-operand words of every rotation (the form older callers know); 8: slot_c and sc as well; 9: and
// the LUT index; 10: and the extract spec word.  ops = ops5, or records of 10 words when lut_ops
// (tfhe_hip_test_level_plan_lut), or of 16 when rec_words = 16 (tfhe_hip_test_level_plan_multi: dead_slots as well).
// lin (tfhe_hip_test_level_plan_lin): records of kind 66 name terms of lin->terms2; their part of the plan goes to lin->*
// (tfhe_hip_test_level_plan_full: lin->not_off and lin->nots2 are set and receive LevelPlan::not_off / nots)
struct TestLinPlan {
    const int32_t *terms2; int32_t nterms;
    int32_t *ranks_out, *sizes2, *level_off, *launch_off, *launch_rank, *descs35;
    int32_t *not_off = nullptr, *nots2 = nullptr;            // tfhe_hip_test_level_plan_full: the NOT descriptors as well
};
static int test_level_plan(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                           int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                           int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots, int rot_words, int32_t *kss4,
                           bool lut_ops = false, int32_t reuse = 0, int32_t *shared_with = nullptr, int rec_words = 10,
                           const int32_t *dead_slots = nullptr, int32_t ndead = 0, const TestLinPlan *lin = nullptr) {
    if (count < 0 || nkeys < 1 || nkeys > UINT16_MAX) { set_error("test_level_plan: bad count or nkeys"); return -1; }
    for (int32_t i = 0; i < count; ++i)
        if (op_keys[i] < 0 || op_keys[i] >= nkeys) { set_error("test_level_plan: key index out of range"); return -1; }
    std::vector<PendingOp> ops;
    std::vector<int32_t> op_of_record;                   // lut_ops: record -> index in ops (-1: eliminated)
    std::vector<LinTerm> terms;                          // the graph's term table (records of kind 66)
    int depth;
    if (!lut_ops) {
        depth = test_build_ops(ops5, count, ops);
        if (depth < 0) return -1;
        for (int32_t i = 0; i < count; ++i) ops[i].key = (uint16_t)op_keys[i];
    } else {
        // The records go through the recorder's own graph (op_graph.hpp) over a plain slot table.  Every id of the records
        // is a handle that holds the slot of its own number; the destination ids of a record are the fresh slots the graph
        // is offered, and a record that was shared re-points its handles, so later records read what the recorder's
        // would.  shared_with[i] = the record whose op record i shares or widens, or -1.
        struct SlotTable {
            std::vector<int32_t> ref, level;
            std::vector<uint8_t> pending;
            void retain(int32_t s) { ++ref[(size_t)s]; }
            void release(int32_t s) { --ref[(size_t)s]; }
            int32_t refs(int32_t s) const { return ref[(size_t)s]; }
        };
        const int id_words = rec_words == 16 ? 4 : 0;            // the destinations of a multi-output record: words 12..15
        int32_t top = 0;
        for (int32_t i = 0; i < count; ++i) {
            const int32_t *o = ops5 + (size_t)rec_words * (size_t)i;
            for (int w = 1; w <= 4; ++w) top = std::max(top, o[w] + 1);
            for (int w = 12; w < 12 + id_words; ++w) top = std::max(top, o[w] + 1);
            if (lin && o[0] == OP_LIN) {
                if (o[5] < 0 || o[6] < 1 || o[6] > LIN_MAX_IN || o[5] > lin->nterms - o[6]) { set_error("test_level_plan_lin: bad term range"); return -1; }
                for (int t = 0; t < o[6]; ++t) {
                    if (lin->terms2[2 * (size_t)(o[5] + t)] < 0) { set_error("test_level_plan_lin: a term without an operand"); return -1; }
                    top = std::max(top, lin->terms2[2 * (size_t)(o[5] + t)] + 1);
                }
            }
        }
        SlotTable slots{std::vector<int32_t>((size_t)top, 1), std::vector<int32_t>((size_t)top, 0), std::vector<uint8_t>((size_t)top, 0)};
        std::vector<int32_t> handle((size_t)top), record_of_op;
        std::iota(handle.begin(), handle.end(), 0);
        OpGraph<SlotTable> graph;
        graph.reuse = reuse != 0;
        op_of_record.assign((size_t)count, -1);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t *o = ops5 + (size_t)rec_words * (size_t)i;
            const bool multi = rec_words == 16 && o[0] == OP_LUTM;
            const bool is_lin = lin && o[0] == OP_LIN;
            if (!op_kind_valid_lut(o[0]) && !multi && !is_lin) { set_error("test schedule: unknown op kind"); return -1; }
            auto slot_of = [&](int32_t id) { return id >= 0 ? handle[(size_t)id] : -1; };
            PendingOp op{(uint8_t)o[0], -1, slot_of(o[2]), slot_of(o[3]), slot_of(o[4]), 0, (uint16_t)op_keys[i]};
            if (op.kind == OP_LUT || multi) { op.lut = o[5]; op.sa = o[6]; op.sb = o[7]; op.sc = o[8]; op.c0 = o[9]; }
            int32_t ids[4] = {o[1], -1, -1, -1}, out[4];
            if (multi) {
                op.spec = o[10]; op.nout = o[11];
                if (op.nout < 1 || op.nout > XS_MAX_OUT) { set_error("test_level_plan_multi: nout must be 1..4"); return -1; }
                std::copy(o + 12, o + 12 + op.nout, ids);
            }
            LinTerm lt[LIN_MAX_IN];
            if (is_lin) {
                op.a = op.b = op.c = -1;
                op.nout = o[6]; op.c0 = o[9];
                for (int t = 0; t < op.nout; ++t) lt[t] = LinTerm{slot_of(lin->terms2[2 * (size_t)(o[5] + t)]), lin->terms2[2 * (size_t)(o[5] + t) + 1]};
            }
            unsigned wanted = 0;
            for (int m = 0; m < op_outputs(op); ++m) {
                if (ids[m] < 0) continue;
                if (handle[(size_t)ids[m]] != ids[m] || slots.pending[(size_t)ids[m]] || std::count(ids, ids + m, ids[m])) {
                    set_error("test_level_plan: a destination id used twice");
                    return -1;
                }
                wanted |= 1u << m;
            }
            if (!wanted) { set_error("test_level_plan: an op without a destination"); return -1; }
            const int32_t shared = graph.record(slots, op, wanted, [&](int m) { return ids[m]; }, out, is_lin ? lt : nullptr);
            if (shared < 0) record_of_op.push_back(i);
            if (shared_with) shared_with[i] = shared < 0 ? -1 : record_of_op[(size_t)shared];
            op_of_record[(size_t)i] = shared < 0 ? (int32_t)record_of_op.size() - 1 : shared;
            for (int m = 0; m < op_outputs(op); ++m)
                if ((wanted >> m & 1) && out[m] != ids[m]) { slots.release(ids[m]); handle[(size_t)ids[m]] = out[m]; }   // (recorder.cpp repoint)
        }
        for (int32_t d = 0; d < ndead; ++d) {                    // these handles are gone before the flush
            const int32_t id = dead_slots[d];
            if (id < 0 || id >= top || handle[(size_t)id] < 0) continue;
            slots.release(handle[(size_t)id]);
            handle[(size_t)id] = -1;
        }
        std::vector<int32_t> moved_to;
        graph.eliminate_dead(slots, &moved_to);
        for (int32_t &at : op_of_record) at = moved_to[(size_t)at];
        ops = graph.ops();
        terms.assign(graph.terms(), graph.terms() + graph.term_count());
        depth = graph.max_level();
    }
    std::vector<int32_t> lvl;
    const int levels = schedule_levels(ops, depth, balance != 0, unit, lvl, nullptr, terms.data());
    const LevelPlan plan = build_level_plan(ops, lvl, levels, nkeys, terms.data());     // exactly what flush_locked hands to execute()
    for (int32_t i = 0; i < count; ++i) {
        const int32_t at = lut_ops ? op_of_record[(size_t)i] : i;
        levels_out[i] = at >= 0 ? lvl[(size_t)at] : -1;      // -1: eliminated (tfhe_hip_test_level_plan_multi's dead_slots)
        if (lin) lin->ranks_out[i] = at < 0 ? -1 : plan.op_rank.empty() ? 0 : plan.op_rank[(size_t)at];
    }
    if (lin) {
        static_assert(sizeof(LinDesc) == 35 * sizeof(int32_t), "a linear descriptor is 35 plain words");
        lin->sizes2[0] = plan.lins.empty() ? 0 : (int32_t)plan.lin_launch_off.size() - 1;
        lin->sizes2[1] = (int32_t)plan.lins.size();
        for (size_t L = 0; L < (size_t)levels + 2; ++L) lin->level_off[L] = plan.lins.empty() ? 0 : plan.lin_level_off[L];
        if (!plan.lins.empty()) {
            std::memcpy(lin->launch_off, plan.lin_launch_off.data(), plan.lin_launch_off.size() * sizeof(int32_t));
            std::memcpy(lin->launch_rank, plan.lin_launch_rank.data(), plan.lin_launch_rank.size() * sizeof(int32_t));
            std::memcpy(lin->descs35, plan.lins.data(), plan.lins.size() * sizeof(LinDesc));
        }
        if (lin->not_off) {
            static_assert(sizeof(NotDesc) == 2 * sizeof(int32_t), "a NOT descriptor is two plain words");
            std::memcpy(lin->not_off, plan.not_off.data(), plan.not_off.size() * sizeof(int32_t));
            if (!plan.nots.empty()) std::memcpy(lin->nots2, plan.nots.data(), plan.nots.size() * sizeof(NotDesc));
        }
    }
    sizes6[0] = plan.levels;
    sizes6[1] = (int32_t)plan.rots.size();
    sizes6[2] = (int32_t)plan.kss.size();
    sizes6[3] = (int32_t)plan.rot_koff.size();
    sizes6[4] = (int32_t)plan.ks_koff.size();
    sizes6[5] = (int32_t)plan.rot_key.size();
    static_assert(sizeof(RotDesc) == 10 * sizeof(int32_t) && offsetof(RotDesc, slot_c) == 6 * sizeof(int32_t) &&
                      offsetof(RotDesc, lut) == 8 * sizeof(int32_t) && offsetof(RotDesc, spec) == 9 * sizeof(int32_t) &&
                      sizeof(KsDesc) == 4 * sizeof(int32_t),
                  "descriptors are plain words: the third operand behind the first six, then the LUT index, the extract spec last");
    auto copy = [](int32_t *dst, const void *src, size_t words) { if (words) std::memcpy(dst, src, words * sizeof(int32_t)); };
    copy(rot_off, plan.rot_off.data(), plan.rot_off.size());
    copy(ks_off, plan.ks_off.data(), plan.ks_off.size());
    copy(rot_koff, plan.rot_koff.data(), plan.rot_koff.size());
    copy(ks_koff, plan.ks_koff.data(), plan.ks_koff.size());
    copy(rot_key, plan.rot_key.data(), plan.rot_key.size());
    for (size_t r = 0; r < plan.rots.size(); ++r) copy(rots + (size_t)rot_words * r, &plan.rots[r], (size_t)rot_words);
    copy(kss4, plan.kss.data(), 4 * plan.kss.size());
    return levels;
}

int tfhe_hip_test_level_plan(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                             int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                             int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots6, int32_t *kss4) {
    return test_level_plan(ops5, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots6, 6, kss4);
}
int tfhe_hip_test_level_plan3(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                              int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                              int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots8, int32_t *kss4) {
    return test_level_plan(ops5, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots8, 8, kss4);
}

int tfhe_hip_test_level_plan_lut(const int32_t *ops10, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, int32_t *levels_out, int32_t *shared_with, int32_t *sizes6,
                                 int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key,
                                 int32_t *rots9, int32_t *kss4) {
    if (reuse && !shared_with) { set_error("test_level_plan_lut: reuse needs shared_with"); return -1; }
    return test_level_plan(ops10, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots9, 9, kss4, true, reuse, shared_with);
}

int tfhe_hip_test_level_plan_multi(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                   int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                   int32_t *levels_out, int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                                   int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4) {
    if (!shared_with) { set_error("test_level_plan_multi: shared_with is needed"); return -1; }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_multi: bad dead_slots"); return -1; }
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead);
}

int tfhe_hip_test_level_plan_lin(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                 const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                 int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                 int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                 int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35) {
    if (!shared_with || !ranks_out || !lin_sizes2 || !lin_level_off || !lin_launch_off || !lin_launch_rank || !lins35) {
        set_error("test_level_plan_lin: null output");
        return -1;
    }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_lin: bad dead_slots"); return -1; }
    if (nterms < 0 || (nterms > 0 && !lin_terms2)) { set_error("test_level_plan_lin: bad term table"); return -1; }
    const TestLinPlan lin{lin_terms2, nterms, ranks_out, lin_sizes2, lin_level_off, lin_launch_off, lin_launch_rank, lins35};
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead, &lin);
}

int tfhe_hip_test_level_plan_full(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                  int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                  const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                  int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                  int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                  int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35,
                                  int32_t *not_off, int32_t *nots2) {
    if (!shared_with || !ranks_out || !lin_sizes2 || !lin_level_off || !lin_launch_off || !lin_launch_rank || !lins35 ||
        !not_off || !nots2) {
        set_error("test_level_plan_full: null output");
        return -1;
    }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_full: bad dead_slots"); return -1; }
    if (nterms < 0 || (nterms > 0 && !lin_terms2)) { set_error("test_level_plan_full: bad term table"); return -1; }
    const TestLinPlan lin{lin_terms2, nterms, ranks_out, lin_sizes2, lin_level_off, lin_launch_off, lin_launch_rank, lins35,
                          not_off, nots2};
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead, &lin);
}

int tfhe_hip_test_br_plan(int32_t N, int32_t l, int32_t Bgbit, const int32_t *tunings4, int32_t cu_count, int32_t count,
                          int32_t flags, int32_t *out3) {
    if (!tunings4 || !out3 || cu_count < 1 || count < 1) { set_error("test_br_plan: bad arguments"); return -1; }
    LaunchTunings t;
    t.br_variant = tunings4[0]; t.br8_max_rotations = tunings4[1]; t.br_tail8 = tunings4[2]; t.br_digit_table = tunings4[3];
    bool form_ok[BR_FORM_COUNT][3];
    fill_form_ok(form_ok, N, l, Bgbit);                       // as upload_key fills a key image's
    const BrPlan plan = plan_br(form_ok, N, l, t, cu_count, count, (flags & 1) != 0, (flags & 2) != 0);
    out3[0] = plan.form; out3[1] = plan.tables; out3[2] = plan.tail;
    return 0;
}

// The first `nout` of the seven words of the key-switch launch plan (launch_plan.hpp plan_ks_launch, what Engine::launch_ks
// runs): tiled, tile, chunk, ranges of a full chunk, ranges of the last chunk, partial-sum bytes, form.  tunings: the first
// `ntunings` of ks_target_blocks, ks_max_splits, ks_split_ties, ks_tile, ks_index, ks_matrix, ks_matrix_min
static int test_ks_plan_words(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings, int ntunings,
                              bool has_image, int32_t cu_count, int32_t count, int64_t *out, int nout) {
    if (!tunings || !out || cu_count < 1 || count < 1) { set_error("test_ks_plan: bad arguments"); return -1; }
    LaunchTunings t;
    int *const fields[7] = {&t.ks_target_blocks, &t.ks_max_splits, &t.ks_split_ties, &t.ks_tile, &t.ks_index, &t.ks_matrix, &t.ks_matrix_min};
    for (int i = 0; i < ntunings; ++i) *fields[i] = tunings[i];
    Params p{};
    p.n = n;
    const KsLaunchPlan plan = plan_ks_launch(t, cu_count, count, KsShape{k * N, ks_t, ks_basebit, p.ct_stride()}, has_image);
    const int64_t words[7] = {plan.full.form != KS_FORM_PERGATE, plan.full.tile, plan.chunk, plan.full.splits, plan.last.splits,
                              (int64_t)plan.partial_bytes, plan.full.form};
    std::copy(words, words + nout, out);
    return 0;
}

int tfhe_hip_test_ks_plan_form(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                               int32_t cu_count, int32_t count, int64_t *out7) {
    return test_ks_plan_words(n, N, k, ks_t, ks_basebit, tunings5, 5, false, cu_count, count, out7, 7);
}

// the entry above with the two tunings of the matrix form and has_image: the key holds its byte-plane image, as a flush finds
// it -- the plan Engine::prepare_flush makes and run_level runs
int tfhe_hip_test_ks_plan_form2(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings7,
                                int32_t has_image, int32_t cu_count, int32_t count, int64_t *out7) {
    return test_ks_plan_words(n, N, k, ks_t, ks_basebit, tunings7, 7, has_image != 0, cu_count, count, out7, 7);
}

// the byte planes of `count` words (ks_matrix.hpp ks_byte_planes): planes4[w][p]
int tfhe_hip_test_ks_byte_planes(const uint32_t *words, int32_t count, int8_t *planes4) {
    if (!words || !planes4 || count < 0) { set_error("test_ks_byte_planes: bad arguments"); return -1; }
    for (int32_t i = 0; i < count; ++i) ks_byte_planes(words[i], planes4 + 4 * (size_t)i);
    return 0;
}

// the first six words of the entry above: callers of this one provide room for six
int tfhe_hip_test_ks_plan(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                          int32_t cu_count, int32_t count, int64_t *out6) {
    return test_ks_plan_words(n, N, k, ks_t, ks_basebit, tunings5, 5, false, cu_count, count, out6, 6);
}

int tfhe_hip_test_wg_times(const TFheGateBootstrappingCloudKeySet *bk, int32_t width, uint64_t *times4, double *launch_ms) {
    if (!bk || !bk->bk || !times4 || width <= 0) { set_error("wg_times: bad arguments"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    const double ms = Engine::get().run_wg_times(bk->bk->dev, width, reinterpret_cast<unsigned long long *>(times4));
    if (launch_ms) *launch_ms = ms;
    if (ms < 0) { set_error("wg_times: the launched kernel form wrote no stamps"); return -1; }
    return 0;
}

int tfhe_hip_kernel_negacyclic(const TFheGateBootstrappingCloudKeySet *bk, const int32_t *ip, const Torus32 *tp,
                               Torus32 *res, int32_t count) {
    if (!bk || !bk->bk) { set_error("negacyclic: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_negacyclic(bk->bk->dev, ip, tp, res, count);
    return 0;
}
int tfhe_hip_kernel_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                   Torus32 *u_out, Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("bootstrap_woks: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_raw_rotations(bk->bk->dev, lin, count, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, u_out, acc_out, "bootstrap_woks");
    return 0;
}
int tfhe_hip_kernel_lut_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                       const int32_t *lut_index, const Torus32 *polys, int32_t npolys, Torus32 *u_out,
                                       Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("lut_bootstrap_woks: null keyset"); return -1; }
    if (!lut_index || !polys || npolys < 1) { set_error("lut_bootstrap_woks: null or empty LUT table"); return -1; }
    auto g = recorder_lock();
    return guarded_rc([&] {
        pool_of_key(bk);
        Engine::get().run_raw_rotations(bk->bk->dev, lin, count, lut_index, polys, npolys, nullptr, nullptr, 0, 1, u_out, acc_out, "lut_bootstrap_woks");
        return 0;
    });
}
int tfhe_hip_kernel_lut_bootstrap_multi_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                             const int32_t *lut_index, const Torus32 *polys, int32_t npolys,
                                             const int32_t *spec_index, const int32_t *specs, int32_t nspecs, Torus32 *u_out,
                                             Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("lut_bootstrap_multi_woks: null keyset"); return -1; }
    if (!lut_index || !polys || npolys < 1) { set_error("lut_bootstrap_multi_woks: null or empty LUT table"); return -1; }
    if (!spec_index || !specs || nspecs < 1) { set_error("lut_bootstrap_multi_woks: null or empty spec table"); return -1; }
    static_assert(XS_WORDS == TFHE_HIP_EXTRACT_SPEC_WORDS, "the spec records of the raw entry are ExtractSpec's words");
    auto g = recorder_lock();
    return guarded_rc([&] {
        pool_of_key(bk);
        Engine::get().run_raw_rotations(bk->bk->dev, lin, count, lut_index, polys, npolys, spec_index, reinterpret_cast<const ExtractSpec *>(specs),
                                        nspecs, XS_MAX_OUT, u_out, acc_out, "lut_bootstrap_multi_woks");
        return 0;
    });
}
int tfhe_hip_kernel_keyswitch(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *u, int32_t count, Torus32 *out) {
    if (!bk || !bk->bk) { set_error("keyswitch: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_keyswitch(bk->bk->dev, u, count, out);
    return 0;
}

int tfhe_hip_kernel_keyswitch_matrix(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *u, int32_t count, Torus32 *out) {
    if (!bk || !bk->bk || !u || !out) { set_error("keyswitch_matrix: null argument"); return -1; }
    auto g = recorder_lock();
    return guarded_rc([&] {
        pool_of_key(bk);
        Engine::get().run_keyswitch_matrix(bk->bk->dev, u, count, out);
        return 0;
    });
}

}  // extern "C"
