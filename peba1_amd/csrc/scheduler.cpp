// scheduler.cpp -- see scheduler.hpp.  Host logic only.
#include "scheduler.hpp"

#include "engine.hpp"
#include "launch_plan.hpp"

#include <algorithm>
#include <queue>
#include <unordered_map>

namespace tfhe_hip {

namespace {
struct HeapItem {
    int32_t alap, idx;
    bool operator>(const HeapItem &o) const { return alap != o.alap ? alap > o.alap : idx > o.idx; }
};

// The cost-driven pass behind the list scheduling (tuning "level_slack").  The list scheduling fills levels by a width
// policy; what a level really costs is a staircase in its width (launch_plan.hpp LevelCost: measured), and a level a few
// rotations past a step pays the whole step.  One forward sweep: at level L, the gates whose successors all run later than
// L + j may run j levels later (j up to 4: the look-ahead); among the amounts the table's own steps suggest -- down to a step
// below L's width, up to a step above the other level's, or all of them -- the one that lowers cost(L) + cost(L + j) most, by
// at least half a percent (the table is a measurement), is moved, gates with the latest bound first.  What was moved is
// looked at again where it landed, so a surplus travels until it finds room.  Depth, dependencies and the set of gates stay;
// linear ops follow their operands.  Sort aside, the work is one visit per gate and level it passes.  Nothing changes unless the sum over all levels fell.
struct SuccLists { const std::vector<int32_t> &off, &to; };
struct PredLists { const std::vector<size_t> &at; const std::vector<int32_t> &of, &count; };
void relevel_by_cost(const std::vector<PendingOp> &ops, int depth, const LevelCost &cost, const SuccLists &succ,
                     const PredLists &pred, std::vector<int32_t> &lvl, LevelSlackReport *report) {
    const int n = (int)ops.size();
    std::vector<long long> width((size_t)depth + 2, 0);
    std::vector<std::vector<int32_t>> at((size_t)depth + 2);
    for (int i = 0; i < n; ++i) {
        if (op_is_linear(ops[i].kind)) continue;
        width[(size_t)lvl[i]] += op_rotations(ops[i]);
        at[(size_t)lvl[i]].push_back(i);
    }
    auto total = [&] { double t = 0; for (int L = 1; L <= depth; ++L) t += level_cost_at(cost, width[(size_t)L]); return t; };
    const double before = total();
    if (report) { report->us_before = report->us_after = before; report->moved = 0; }
    const std::vector<int32_t> kept = lvl;
    // the latest level of op i its successors allow: a gate behind it runs a level later, a linear op rides along
    auto latest = [&](int32_t i, auto &&self) -> int32_t {
        int32_t ub = depth;
        for (int32_t e = succ.off[i]; e < succ.off[i + 1] && ub > lvl[i]; ++e) {
            const int32_t s = succ.to[e];
            ub = std::min(ub, op_is_linear(ops[s].kind) ? self(s, self) : lvl[s] - 1);
        }
        return ub;
    };
    std::vector<HeapItem> movable;          // (-latest level, op): sorts latest bound first, then recording order
    long long moved_gates = 0;
    constexpr int STEPS = 16, AHEAD = 4;
    for (int L = 1; L < depth; ++L) {
        movable.clear();
        long long free_rot = 0;
        for (int32_t i : at[(size_t)L]) {
            const int32_t ub = latest(i, latest);
            if (ub > L) { movable.push_back(HeapItem{-ub, i}); free_rot += op_rotations(ops[i]); }
        }
        if (!free_rot) continue;
        std::sort(movable.begin(), movable.end(), [](const HeapItem &x, const HeapItem &y) { return y > x; });
        // where to: one of the next AHEAD levels (a surplus that gains nothing next door may do so two levels on)
        const long long w = width[(size_t)L];
        double best_gain = 0;
        long long best_m = 0;
        int best_j = 0;
        size_t reach = movable.size();                              // gates that may run at L + j: a prefix
        for (int j = 1; j <= AHEAD && L + j <= depth; ++j) {
            while (reach > 0 && -movable[reach - 1].alap < L + j) free_rot -= op_rotations(ops[movable[--reach].idx]);
            if (!free_rot) break;
            const long long nx = width[(size_t)(L + j)];
            const double now = level_cost_at(cost, w) + level_cost_at(cost, nx);
            auto consider = [&](long long m) {
                if (m <= 0 || m > free_rot) return;
                const double gain = now - level_cost_at(cost, w - m) - level_cost_at(cost, nx + m);
                if (gain <= 0.005 * now) return;
                // (equal gains: the nearer level, then the fewer gates -- what stays behind can still go elsewhere)
                if (gain > best_gain + 1e-9 || (gain > best_gain - 1e-9 && j == best_j && m < best_m)) { best_gain = gain; best_m = m; best_j = j; }
            };
            long long steps[STEPS];
            consider(free_rot);
            for (int k = level_cost_steps(cost, w, -1, steps, STEPS); k-- > 0;) consider(w - steps[k]);
            for (int k = level_cost_steps(cost, nx, +1, steps, STEPS); k-- > 0;) consider(steps[k] - nx);
        }
        if (!best_m) continue;
        const int to = L + best_j;
        long long m = 0;
        size_t take = 0;
        for (; take < movable.size() && -movable[take].alap >= to; ++take) {
            const int r = op_rotations(ops[movable[take].idx]);
            if (m + r > best_m) break;                          // (a MUX is two rotations: never past the amount)
            m += r;
        }
        const double now = level_cost_at(cost, w) + level_cost_at(cost, width[(size_t)to]);
        if (now - level_cost_at(cost, w - m) - level_cost_at(cost, width[(size_t)to] + m) <= 0.005 * now) continue;
        for (size_t t = 0; t < take; ++t) {
            lvl[movable[t].idx] = to;
            at[(size_t)to].push_back(movable[t].idx);
        }
        width[(size_t)L] -= m;
        width[(size_t)to] += m;
        moved_gates += (long long)take;
    }
    const double after = total();
    if (!moved_gates || !(after < before)) { lvl = kept; return; }
    // linear ops: the highest level of what they read (recording order is topological)
    for (int i = 0; i < n; ++i) {
        if (!op_is_linear(ops[i].kind)) continue;
        int32_t l = 0;
        for (int t = 0; t < pred.count[i]; ++t) l = std::max(l, lvl[pred.of[pred.at[i] + t]]);
        lvl[i] = l;
    }
    if (report) { report->us_after = after; report->moved = moved_gates; }
}
}  // namespace


int schedule_levels(const std::vector<PendingOp> &ops, int asap_depth, bool balance, int unit,
                    std::vector<int32_t> &lvl, std::vector<int32_t> *alap_out, const LinTerm *terms,
                    const LevelCost *cost, LevelSlackReport *report) {
    if (report) *report = LevelSlackReport{};
    const int n = (int)ops.size();
    lvl.resize(n);
    for (int i = 0; i < n; ++i) lvl[i] = ops[i].level;
    if (alap_out) *alap_out = lvl;
    if (!balance || asap_depth <= 2 || n < 4 * unit) return asap_depth;

    // producer of each pending slot (destinations are unique: SSA; slot ids are pool indices, so a flat
    // table replaces the hash map that used to cost a third of a match's scheduling time)
    int32_t max_slot = -1;
    for (int i = 0; i < n; ++i) for_each_dst(ops[i], [&](int32_t d) { max_slot = std::max(max_slot, d); });
    std::vector<int32_t> producer((size_t)max_slot + 1, -1);
    for (int i = 0; i < n; ++i)
        for_each_dst(ops[i], [&](int32_t d) { if (producer[d] < 0) producer[d] = i; });   // (first writer, as emplace kept it)

    // predecessor lists (<= 3 each; a linear combination: one per term) and successor lists in CSR form
    std::vector<size_t> pred_at(n);
    size_t pred_room = 0;
    for (int i = 0; i < n; ++i) { pred_at[i] = pred_room; pred_room += 3 + (size_t)op_terms(ops[i]); }
    std::vector<int32_t> pred(pred_room, -1), npred(n, 0), succ_off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        for_each_src(ops[i], terms, [&](int32_t src) {
            const int32_t pr = src <= max_slot ? producer[src] : -1;
            if (pr < 0 || pr >= i) return;                           // materialised before this flush
            bool dup = false;
            for (int t = 0; t < npred[i]; ++t) dup |= pred[pred_at[i] + t] == pr;
            if (dup) return;
            pred[pred_at[i] + npred[i]++] = pr;
            ++succ_off[pr + 1];
        });
    }
    for (int i = 0; i < n; ++i) succ_off[i + 1] += succ_off[i];
    std::vector<int32_t> succ(succ_off[n]), cursor(succ_off.begin(), succ_off.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < npred[i]; ++t) succ[cursor[pred[pred_at[i] + t]]++] = i;

    // ALAP: recording order is topological, so one reverse sweep suffices
    std::vector<int32_t> alap(n, asap_depth);
    for (int i = n - 1; i >= 0; --i) {
        const int32_t need = op_is_linear(ops[i].kind) ? alap[i] : alap[i] - 1;   // a linear op runs after its level's gates
        for (int t = 0; t < npred[i]; ++t) {
            int32_t &a = alap[pred[pred_at[i] + t]];
            a = std::min(a, need);
        }
    }

    if (alap_out) *alap_out = alap;

    // list scheduling, least slack first
    long long remaining = 0;
    for (const PendingOp &op : ops) remaining += op_rotations(op);
    // (earliest level: 1 for a gate; a linear op takes the highest level of what it reads, 0 if all of it is materialised)
    std::vector<int32_t> left(npred), est(n, 1);
    for (int i = 0; i < n; ++i)
        if (op_is_linear(ops[i].kind)) est[i] = 0;
    std::vector<std::vector<int32_t>> avail(asap_depth + 2);
    auto release_successors = [&](int32_t i, int32_t level_done, auto &&self) -> void {
        for (int32_t e = succ_off[i]; e < succ_off[i + 1]; ++e) {
            const int32_t s = succ[e];
            const bool is_not = op_is_linear(ops[s].kind);
            est[s] = std::max(est[s], is_not ? level_done : level_done + 1);
            if (--left[s] != 0) continue;
            if (is_not) {                       // linear: rides along with its operand's level
                lvl[s] = est[s];
                self(s, lvl[s], self);
            } else {
                avail[std::min<int32_t>(est[s], asap_depth + 1)].push_back(s);
            }
        }
    };
    for (int i = 0; i < n; ++i) {
        if (left[i] != 0) continue;
        if (op_is_linear(ops[i].kind)) {
            if (npred[i] == 0) { lvl[i] = 0; est[i] = 0; }
        } else {
            avail[1].push_back(i);
        }
    }
    // linear ops of materialised inputs release their successors now (level 0 is "before level 1")
    for (int i = 0; i < n; ++i)
        if (op_is_linear(ops[i].kind) && npred[i] == 0) release_successors(i, 0, release_successors);

    std::priority_queue<HeapItem, std::vector<HeapItem>, std::greater<HeapItem>> heap;
    std::vector<int32_t> batch;
    // rotations not yet scheduled, by deadline (ALAP level)
    std::vector<long long> due(asap_depth + 2, 0);
    for (int i = 0; i < n; ++i) due[alap[i]] += op_rotations(ops[i]);
    for (int L = 1; L <= asap_depth; ++L) {
        for (int32_t i : avail[L]) heap.push(HeapItem{alap[i], i});
        const long long levels_left = asap_depth - L + 1;
        // Width policy.  A launch costs by occupancy steps (MI355X, P128: up to 1 workgroup per
        // CU 4.2 ms, up to 2 per CU 6.5 ms, then 10.1 and 12.6 ms for 3 and 4 units), so the
        // cheap widths are exactly 1x `unit` for a level that could not be wider anyway and
        // multiples of 2x `unit`; a width just above a multiple of 2x `unit` is the worst buy.
        // Base width: `unit` once the remaining work fits in one unit per remaining level, else
        // 2 units.  The base is doubled only when the deadlines demand it: if for some future
        // level D the rotations due by D exceed what base-wide levels L..D can hold (earliest-
        // deadline-first feasibility), some level must be wider, and a full double-width level
        // now is cheaper than forced overflows later.
        const long long base = remaining <= (long long)unit * levels_left ? unit : 2LL * unit;
        long long cap = base, running = 0, excess = 0;
        const int horizon = std::min(asap_depth, L + 1023);     // bounded look-ahead keeps deep DAGs cheap
        for (int D = L; D <= horizon; ++D) {
            running += due[D];
            excess = std::max(excess, running - base * (long long)(D - L + 1));
        }
        while (excess > cap - base && cap < 16LL * unit) cap *= 2;
        long long width = 0;
        batch.clear();
        auto take = [&](long long limit, bool forced_only) {
            while (!heap.empty()) {
                const HeapItem top = heap.top();
                const int w = op_rotations(ops[top.idx]);
                if (top.alap > L && (forced_only || width + w > limit)) break;
                heap.pop();
                lvl[top.idx] = L;
                width += w;
                due[top.alap] -= w;
                batch.push_back(top.idx);
            }
        };
        take(cap, false);
        // gates at their deadline overflowed the width: round it up to the next multiple of
        // two units and fill that with slack gates (the second half of an occupancy step is cheap)
        if (width > cap) take((width + 2LL * unit - 1) / (2LL * unit) * (2LL * unit), false);
        remaining -= width;
        for (int32_t i : batch) release_successors(i, L, release_successors);
    }
    if (cost && cost->n > 0) relevel_by_cost(ops, asap_depth, *cost, SuccLists{succ_off, succ}, PredLists{pred_at, pred, npred}, lvl, report);
    return asap_depth;
}

// The linear combinations of a plan: each op's rank from the levels the ops really run at, the descriptors ordered by
// (level, rank), one launch range per pair present.
static void plan_linear_ops(LevelPlan &plan, const std::vector<PendingOp> &ops, const std::vector<int32_t> &lvl, int levels,
                            const LinTerm *terms) {
    int32_t max_slot = -1;
    size_t nlin = 0;
    for (const PendingOp &op : ops)
        if (op.kind == OP_LIN) { max_slot = std::max(max_slot, op.dst); ++nlin; }
    if (!nlin) return;
    // recording order is topological: the producer of a term's slot, if a linear combination, has its rank already
    std::vector<int32_t> producer((size_t)max_slot + 1, -1);
    plan.op_rank.assign(ops.size(), 0);
    std::vector<std::pair<int64_t, int32_t>> order;       // (level, rank) -> op
    order.reserve(nlin);
    for (size_t i = 0; i < ops.size(); ++i) {
        const PendingOp &op = ops[i];
        if (op.kind != OP_LIN) continue;
        int32_t rank = 0;
        for (int t = 0; t < op.nout; ++t) {
            const int32_t s = terms[op.spec + t].slot;
            const int32_t pr = s <= max_slot ? producer[(size_t)s] : -1;
            if (pr >= 0 && lvl[(size_t)pr] == lvl[i]) rank = std::max(rank, plan.op_rank[(size_t)pr] + 1);
        }
        plan.op_rank[i] = rank;
        producer[(size_t)op.dst] = (int32_t)i;
        order.emplace_back((int64_t)lvl[i] << 32 | (uint32_t)rank, (int32_t)i);
    }
    std::stable_sort(order.begin(), order.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    plan.lins.resize(nlin);
    plan.lin_level_off.assign((size_t)levels + 2, 0);
    plan.lin_launch_off.assign(1, 0);
    for (size_t j = 0; j < nlin; ++j) {
        const PendingOp &op = ops[(size_t)order[j].second];
        LinDesc &d = plan.lins[j];
        d = LinDesc{};
        d.dst_slot = op.dst; d.nin = op.nout; d.c0 = op.c0;
        for (int t = 0; t < op.nout; ++t) { d.slot[t] = terms[op.spec + t].slot; d.coef[t] = terms[op.spec + t].coef; }
        if (j > 0 && order[j].first != order[j - 1].first) plan.lin_launch_off.push_back((int32_t)j);
        if (j == 0 || order[j].first != order[j - 1].first) {
            plan.lin_launch_rank.push_back((int32_t)(order[j].first & 0xFFFFFFFF));
            ++plan.lin_level_off[(size_t)(order[j].first >> 32) + 1];
        }
    }
    plan.lin_launch_off.push_back((int32_t)nlin);
    for (size_t L = 0; L <= (size_t)levels; ++L) plan.lin_level_off[L + 1] += plan.lin_level_off[L];
}

LevelPlan build_level_plan(const std::vector<PendingOp> &ops, const std::vector<int32_t> &lvl, int levels, int nkeys,
                           const LinTerm *terms) {
    LevelPlan plan;
    plan.levels = levels;
    plan.nkeys = nkeys;
    plan_linear_ops(plan, ops, lvl, levels, terms);
    // counting sort by level: gates of level L (1-based) in group L - 1, NOTs riding on level L (0 = inputs) in group L.
    // Several keys: gates of level L under key k in sub-group (L - 1) nkeys + k, so that a level's descriptors are
    // contiguous per key (rot_koff / ks_koff); with one key the sub-groups are the groups.
    const size_t groups = (size_t)levels * nkeys;
    // uoff: samples of the level's extract buffer.  One per rotation, so that u_index is the rotation's place in its
    // level -- except behind a multi-output op, which takes one sample per output of its spec
    std::vector<int32_t> roff(groups + 1, 0), koff(groups + 1, 0), uoff(groups + 1, 0);
    plan.not_off.assign((size_t)levels + 2, 0);
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].kind == OP_NOT) { ++plan.not_off[(size_t)lvl[i] + 1]; continue; }
        if (ops[i].kind == OP_LIN) continue;                   // (plan_linear_ops)
        const size_t sg = (size_t)(lvl[i] - 1) * nkeys + ops[i].key;
        roff[sg + 1] += op_rotations(ops[i]);
        koff[sg + 1] += op_keyswitches(ops[i]);
        uoff[sg + 1] += op_extracts(ops[i]);
    }
    for (size_t sg = 0; sg < groups; ++sg) { roff[sg + 1] += roff[sg]; koff[sg + 1] += koff[sg]; uoff[sg + 1] += uoff[sg]; }
    plan.rot_off.assign((size_t)levels + 1, 0);
    plan.ks_off.assign((size_t)levels + 1, 0);
    plan.max_rots = 0;
    plan.max_extracts = 0;
    for (size_t g = 0; g <= (size_t)levels; ++g) {
        plan.rot_off[g] = roff[g * nkeys];
        plan.ks_off[g] = koff[g * nkeys];
        if (g > 0) plan.max_rots = std::max(plan.max_rots, plan.rot_off[g] - plan.rot_off[g - 1]);
        if (g > 0) plan.max_extracts = std::max(plan.max_extracts, uoff[g * nkeys] - uoff[(g - 1) * nkeys]);
    }
    for (size_t g = 0; g <= (size_t)levels; ++g) plan.not_off[g + 1] += plan.not_off[g];
    plan.rots.resize(plan.rot_off.back());
    plan.kss.resize(plan.ks_off.back());
    plan.nots.resize(plan.not_off.back());
    if (nkeys > 1) plan.rot_key.resize(plan.rots.size());
    std::vector<int32_t> rpos(roff.begin(), roff.end() - 1);   // cursor per sub-group
    std::vector<int32_t> kpos(koff.begin(), koff.end() - 1);
    std::vector<int32_t> upos(uoff.begin(), uoff.end() - 1);
    std::vector<int32_t> npos(plan.not_off.begin(), plan.not_off.end() - 1);
    const int32_t mu = 1 << 29;
    for (size_t i = 0; i < ops.size(); ++i) {
        const PendingOp &op = ops[i];
        if (op.kind == OP_NOT) {
            plan.nots[npos[(size_t)lvl[i]]++] = NotDesc{op.a, op.dst};
            continue;
        }
        if (op.kind == OP_LIN) continue;
        const size_t g = (size_t)(lvl[i] - 1), sg = g * nkeys + op.key;
        const int32_t base = plan.rot_off[g];
        const int32_t r0 = rpos[sg];
        if (op.kind == OP_LUTM) {
            // the prelude and test polynomial of an OP_LUT; output m of spec op.spec goes to sample u0 + m of the level's
            // extract buffer and, if somebody wants it, through a key switch of its own
            const int32_t i0 = rpos[sg]++, u0 = upos[sg] - uoff[g * nkeys];
            plan.rots[i0] = RotDesc{op.a, op.b >= 0 ? op.b : op.a, op.sa, op.b >= 0 ? op.sb : 0, op.c0, u0,
                                    op.c, op.c >= 0 ? op.sc : 0, op.lut, op.spec | op_wanted(op) << XS_WANTED_SHIFT};
            for (int m = 0; m < op.nout; ++m)
                if (op.dsts[m] >= 0) plan.kss[kpos[sg]++] = KsDesc{u0 + m, -1, 0, op.dsts[m]};
            upos[sg] += op.nout;
            if (nkeys > 1) plan.rot_key[i0] = op.key;
            continue;
        }
        const int32_t ub = upos[sg] - uoff[g * nkeys] - (r0 - base);    // 0 unless a multi-output op stands before
        upos[sg] += op_rotations(op);
        if (op.kind == OP_MUX) {
            // tfhe bootsMUX: u1 = BR(-1/8 + a + b), u2 = BR(-1/8 - a + c), KS(u1 + u2 + 1/8)
            const int32_t i0 = rpos[sg]++, i1 = rpos[sg]++;
            plan.rots[i0] = RotDesc{op.a, op.b, 1, 1, -(mu), i0 - base + ub};
            plan.rots[i1] = RotDesc{op.a, op.c, -1, 1, -(mu), i1 - base + ub};
            plan.kss[kpos[sg]++] = KsDesc{i0 - base + ub, i1 - base + ub, mu, op.dst};
        } else if (op.kind == OP_LUT) {
            // t = (0, c0) + sa A (+ sb B) (+ sc C) from test polynomial op.lut: one rotation, one key switch.  The
            // kernels read slot_b's words whatever sb is, so a one-operand op names A twice with sb = 0
            const int32_t i0 = rpos[sg]++;
            plan.rots[i0] = RotDesc{op.a, op.b >= 0 ? op.b : op.a, op.sa, op.b >= 0 ? op.sb : 0, op.c0, i0 - base + ub,
                                    op.c, op.c >= 0 ? op.sc : 0, op.lut};
            plan.kss[kpos[sg]++] = KsDesc{i0 - base + ub, -1, 0, op.dst};
        } else if (op_is_gate3(op.kind)) {
            // t = sa A + sb B + sc C, c0 = 0: one rotation, one key switch
            const int32_t i0 = rpos[sg]++;
            plan.rots[i0] = RotDesc{op.a, op.b, gate3_coef(op.kind, 0), gate3_coef(op.kind, 1), 0, i0 - base + ub,
                                    op.c, gate3_coef(op.kind, 2)};
            plan.kss[kpos[sg]++] = KsDesc{i0 - base + ub, -1, 0, op.dst};
        } else {
            const GateLin &gl = GATE_LIN[op.kind];
            const int32_t i0 = rpos[sg]++;
            plan.rots[i0] = RotDesc{op.a, op.b, gl.sa, gl.sb, gl.c8 * mu, i0 - base + ub};
            plan.kss[kpos[sg]++] = KsDesc{i0 - base + ub, -1, 0, op.dst};
        }
        for (int32_t r = r0; r < rpos[sg] && nkeys > 1; ++r) plan.rot_key[r] = op.key;
    }
    if (nkeys > 1) { plan.rot_koff.swap(roff); plan.ks_koff.swap(koff); }
    return plan;
}

}  // namespace tfhe_hip
