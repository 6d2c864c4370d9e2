// op_graph.hpp -- the pending operations of a recording as a graph over slots.  Pure host logic: no HIP, no engine, no
// samples.  The recorder (recorder.cpp) runs it over the device slot pool; the plan test entries (test_entries.cpp) run the same
// code over a plain table of vectors.
//
// Slots is any table with retain(s), release(s), refs(s) and per-slot vectors `level` and `pending` (SlotPool has them).
// The graph owns the ops, their depth, the NOT-origin table, the set of slots a pending linear combination writes, the
// term table of the linear combinations and ONE index from OpKey to the op's position in `ops`.
// Invariant: every entry of the index, of the NOT-origin table and of the linear-result set names an op still recorded --
// eliminate_dead drops an op's entries in the step that drops the op and keeps the positions right when it compacts;
// clear drops everything.  (The terms of a dropped linear combination stay in the table, unread, until clear.)
//
// Two dependent linear ops of one level must not share a launch.  NOT(NOT x) is aliased to x by the recorder; here, with
// the same words mod 2^32: a term whose slot a pending NOT writes becomes the NOT's operand with the coefficient negated
// (the combination no longer depends on the NOT), and a NOT of a pending linear combination is recorded as the linear
// combination with the one coefficient -1.  What is left -- a linear combination that reads another one of its level --
// is ordered by rank when the plan is built (scheduler.hpp build_level_plan).
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "scheduler.hpp"

namespace tfhe_hip {

template <class Slots>
class OpGraph {
public:
    // An op recorded again with the same OpKey before the flush is the same function of the same ciphertexts, so its
    // result slots are shared instead of evaluated twice (the reference's circuits do this 12,545 times per match, mostly
    // AND / XOR against the shared constant samples).  Results are unchanged.  Off: nothing is indexed, every op is appended
    bool reuse = true;

    const std::vector<PendingOp> &ops() const { return ops_; }
    int32_t max_level() const { return max_level_; }
    // the (slot, coefficient) pairs of the linear combinations: op i's are terms()[ops()[i].spec ...], op_terms of them
    const LinTerm *terms() const { return terms_.data(); }
    size_t term_count() const { return terms_.size(); }
    // the operand of the pending NOT that writes `slot`, or -1
    int32_t not_origin(int32_t slot) const {
        auto it = not_origin_.find(slot);
        return it == not_origin_.end() ? -1 : it->second;
    }

    // Records `op` (kind, operands, key and the LUT fields filled in; level and destinations are set here) for the outputs
    // in `wanted` (bit m: output m; a single-destination op has output 0 alone).  A pending op with the same key serves
    // the outputs it has and is WIDENED by those it lacks; else the op is appended at level 1 + the highest operand level
    // (a NOT is linear: it rides on its operand's level), holding a reference to each operand.  fresh(m) gives a slot with
    // one reference for output m and is called only for an output that no pending op has; it may flush, which empties the
    // graph (clear), and if it throws the slots already taken go back and nothing is recorded.  out[m] := the slot of
    // wanted output m, with one reference taken for the caller's handle.  Returns the position in ops() of the pending op
    // that was shared or widened, -1 if the op was appended.
    // A linear combination (OP_LIN: op.nout terms in `lin`, op.c0) is never indexed, so never shared: it is appended at
    // the highest level of its terms' slots, holding one reference per term.
    template <class Fresh>
    int32_t record(Slots &slots, PendingOp op, unsigned wanted, Fresh &&fresh, int32_t *out, const LinTerm *lin = nullptr) {
        LinTerm negated;
        if (op.kind == OP_NOT && lin_dst_.count(op.a)) {      // NOT of a pending linear result: that result times -1
            negated = LinTerm{op.a, -1};
            lin = &negated;
            op.kind = OP_LIN; op.a = -1; op.nout = 1; op.c0 = 0;
        }
        const bool indexed = reuse && op.kind != OP_LIN;
        const OpKey key = op_key(op);
        const int nout = op_outputs(op);
        int32_t got[4] = {-1, -1, -1, -1};
        PendingOp *have;
        try {
            for (;;) {
                auto hit = indexed ? index_.find(key) : index_.end();
                have = hit == index_.end() ? nullptr : &ops_[(size_t)hit->second];
                unsigned need = 0;
                for (int m = 0; m < nout; ++m)
                    if ((wanted >> m & 1) && got[m] < 0 && !(have && op_dst(*have, m) >= 0)) need |= 1u << m;
                // a flush inside fresh() leaves no op behind: `have` is good exactly if the ops are as many as before,
                // else it is looked up again (and the outputs it would have served get slots of their own)
                const size_t before = ops_.size();
                for (int m = 0; m < nout; ++m)
                    if (need >> m & 1) got[m] = fresh(m);
                if (ops_.size() == before) break;
            }
        } catch (...) {
            for (const int32_t d : got) if (d >= 0) slots.release(d);
            throw;
        }
        const int32_t shared = have ? (int32_t)(have - ops_.data()) : -1;
        if (!have) {
            if (op.kind == OP_LIN) {
                // (after fresh(): a flush in there has emptied the NOT-origin table, and the NOTs' results are then read)
                op.spec = (int32_t)terms_.size();
                for (int t = 0; t < op.nout; ++t) {
                    const int32_t origin = not_origin(lin[t].slot);
                    terms_.push_back(origin >= 0 ? LinTerm{origin, (int32_t)(0u - (uint32_t)lin[t].coef)} : lin[t]);
                }
            }
            int32_t level = 0;
            for_each_src(op, terms_.data(), [&](int32_t s) { level = std::max(level, slots.level[s]); slots.retain(s); });   // and the pending references
            op.level = op_is_linear(op.kind) ? level : level + 1;
            for (int m = 0; m < nout; ++m) op_dst(op, m) = -1;
            if (indexed) index_.emplace(key, (int32_t)ops_.size());
            ops_.push_back(op);
            have = &ops_.back();
            max_level_ = std::max(max_level_, op.level);
        }
        for (int m = 0; m < nout; ++m) {
            if (!(wanted >> m & 1)) continue;
            int32_t &d = op_dst(*have, m);
            if (d < 0) {
                d = got[m];
                slots.level[d] = have->level;
                slots.pending[d] = 1;             // pending even at level 0 (NOT of a materialised sample)
                if (have->kind == OP_NOT) not_origin_.emplace(d, have->a);
                if (have->kind == OP_LIN) lin_dst_.insert(d);
            }
            slots.retain(d);                      // a fresh slot: the op's own reference; a shared one: the handle's
            out[m] = d;
        }
        return shared;
    }

    // Dead-op elimination: a destination whose only reference is the op's own -- every handle that pointed at it was
    // re-pointed or freed, no live op reads it -- can never be observed, so it is dropped (a multi-output op loses the
    // extracted sample and the key switch of that output), and an op dies with its last destination, releasing its
    // operands: what only it read dies too, since reverse recording order is reverse topological order.  The reference's
    // ripple adders compute a carry out of their last bit and drop it (Math.cpp:60-64 into a freed temporary): 5 of the 7
    // gates of that bit, ~55 gates per slot.  Returns the number of ops dropped; moved_to[i] := the new position of the
    // op that stood at i, -1 if it was dropped.
    size_t eliminate_dead(Slots &slots, std::vector<int32_t> *moved_to = nullptr) {
        std::vector<int32_t> at(ops_.size(), 0);
        size_t dead = 0;
        for (size_t i = ops_.size(); i-- > 0;) {
            PendingOp &op = ops_[i];
            bool live = false;
            for (int m = 0; m < op_outputs(op); ++m) {
                int32_t &d = op_dst(op, m);
                if (d < 0) continue;
                if (slots.refs(d) != 1) { live = true; continue; }   // a handle or a live op still holds the result
                slots.level[d] = 0;
                slots.pending[d] = 0;
                if (op.kind == OP_NOT) not_origin_.erase(d);
                if (op.kind == OP_LIN) lin_dst_.erase(d);
                slots.release(d);
                d = -1;
            }
            if (live) continue;
            auto it = index_.find(op_key(op));
            if (it != index_.end() && it->second == (int32_t)i) index_.erase(it);
            for_each_src(op, terms_.data(), [&](int32_t s) { slots.release(s); });
            at[i] = -1;
            ++dead;
        }
        size_t w = 0;
        int32_t depth = 0;
        for (size_t i = 0; i < ops_.size(); ++i) {
            if (at[i] < 0) continue;
            depth = std::max(depth, ops_[i].level);
            if (w != i) ops_[w] = ops_[i];
            at[i] = (int32_t)w++;
        }
        ops_.resize(w);
        max_level_ = depth;
        if (dead)
            for (auto &entry : index_) entry.second = at[(size_t)entry.second];
        if (moved_to) moved_to->swap(at);
        return dead;
    }

    // after a flush: nothing is pending.  `into` (if given) receives the ops, `terms_into` the term table they name
    void clear(std::vector<PendingOp> *into = nullptr, std::vector<LinTerm> *terms_into = nullptr) {
        if (into) into->swap(ops_);
        if (terms_into) terms_into->swap(terms_);
        ops_.clear();
        terms_.clear();
        index_.clear();
        not_origin_.clear();
        lin_dst_.clear();
        max_level_ = 0;
    }

private:
    std::vector<PendingOp> ops_;
    int32_t max_level_ = 0;
    std::unordered_map<OpKey, int32_t, OpKeyHash> index_;      // key -> position in ops_ (reuse only)
    std::unordered_map<int32_t, int32_t> not_origin_;          // pending NOT output slot -> its operand slot
    std::unordered_set<int32_t> lin_dst_;                      // slots a pending linear combination writes
    std::vector<LinTerm> terms_;                               // the terms of the linear combinations, op after op
};

}  // namespace tfhe_hip
