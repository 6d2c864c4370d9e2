// scheduler.hpp -- slack-aware levelisation of a recorded gate DAG.
//
// ASAP levelling (level = 1 + max level of the operands) runs the reference's
// Function_f as ~110 fat levels (all slots' squares at once, throughput-bound)
// followed by a ~260-level narrow tail (the slot-by-slot ripple accumulation,
// Math.cpp:351-360, latency-bound at ~80 gates per level).  Most gates of the fat
// part have slack: slot k's square is not needed before the tail reaches slot k.
// schedule_levels() keeps the depth of the DAG (every gate at or before its ALAP
// level) but defers slack gates into later, narrower levels, filling each level up
// to the width the kernels run well at.  Only the order among independent gates
// changes; every gate computes the same integers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace tfhe_hip {

struct PendingOp {
    uint8_t kind;       // 0..9 two-input gate code, OP_MUX, OP_NOT, OP_GATE3 + 8 gate + negation mask, OP_LUT, OP_LUTM, OP_LIN
    int32_t dst, a, b, c;   // slots; b, c = -1 when absent
    int32_t level;      // ASAP level (NOT: the level of its operand, 0 = already materialised)
    uint16_t key = 0;   // index of the gate's cloud key in the flush's key list (recorder "batch_keys"; NOT: unused)
    // OP_LUT only (tfhe_hip_lut_bootstrap): the test polynomial (index in the engine's LUT table) and the prelude
    // t = (0, c0) + sa A + sb B + sc C; the coefficient of an absent operand is 0
    int32_t lut = -1;
    int32_t sa = 0, sb = 0, sc = 0, c0 = 0;
    // OP_LUTM only (tfhe_hip_lut_bootstrap_multi): lut and the prelude as for OP_LUT; the extract spec (index in the
    // engine's spec table), its number of outputs, and the destination slot of every output -- -1 for one that nobody
    // wants (a null result, or dead at the flush).  `dst` is unused (-1): op_outputs / op_dst name the outputs of any op
    int32_t spec = -1;
    int32_t nout = 0;
    int32_t dsts[4] = {-1, -1, -1, -1};
    // OP_LIN only (tfhe_hip_linear): dst = (0, c0) + sum of `nout` terms (1..LIN_MAX_IN of them; op_terms) that start at
    // entry `spec` of the recording's term table (OpGraph::terms).  a, b, c are -1: the operands are the terms' slots
};
constexpr uint8_t OP_MUX = 16, OP_NOT = 17;
// programmable bootstrap (not in upstream's gate API): one rotation from a caller-supplied test polynomial, one key switch
constexpr uint8_t OP_LUT = 64;
// three-input gates (tfhe_hip_gate3; not in upstream's API): kind = OP_GATE3 + 8 * gate + mask, gate = enum TfheHipGate3,
// bit i of mask negates operand i (a = bit 0) -- 32..55.  The mask is part of the kind, hence of the recorder's index key
constexpr uint8_t OP_GATE3 = 32, OP_GATE3_END = OP_GATE3 + 3 * 8;
inline bool op_is_gate3(int kind) { return kind >= OP_GATE3 && kind < OP_GATE3_END; }
inline bool op_kind_valid(int kind) { return (kind >= 0 && kind < 10) || kind == OP_MUX || kind == OP_NOT || op_is_gate3(kind); }
inline bool op_kind_valid_lut(int kind) { return op_kind_valid(kind) || kind == OP_LUT; }
// multi-output programmable bootstrap: one rotation, then one extracted sample and one key switch per WANTED output
constexpr uint8_t OP_LUTM = 65;
// linear combination of up to LIN_MAX_IN samples with integer coefficients (tfhe_hip_linear): no rotation, no extract, no
// key switch.  Like a NOT it rides on the highest level of its operands (0: all materialised) and runs after that level's
// key switches; its (slot, coefficient) pairs live in a side table so that PendingOp does not grow for the gates
constexpr uint8_t OP_LIN = 66;
constexpr int LIN_MAX_IN = 16;
struct LinTerm { int32_t slot, coef; };
inline bool op_is_linear(int kind) { return kind == OP_NOT || kind == OP_LIN; }
inline int op_terms(const PendingOp &op) { return op.kind == OP_LIN ? op.nout : 0; }
// every slot an op reads: a, b, c where present, then the terms of a linear combination (`terms`: the recording's table)
template <class F>
inline void for_each_src(const PendingOp &op, const LinTerm *terms, F &&f) {
    for (const int32_t s : {op.a, op.b, op.c})
        if (s >= 0) f(s);
    for (int t = 0; t < op_terms(op); ++t) f(terms[op.spec + t].slot);
}

inline int op_rotations(const PendingOp &op) { return op_is_linear(op.kind) ? 0 : (op.kind == OP_MUX ? 2 : 1); }
// samples of the level's extract buffer an op takes (a multi-output op: one per output of its spec, wanted or not, so
// that output m sits at u_index + m) and key switches it needs
inline int op_extracts(const PendingOp &op) { return op.kind == OP_LUTM ? op.nout : op_rotations(op); }
inline int op_wanted(const PendingOp &op) {
    int w = 0;
    for (int m = 0; m < op.nout; ++m) w |= (op.dsts[m] >= 0) << m;
    return w;
}
inline int op_keyswitches(const PendingOp &op) {
    return op_is_linear(op.kind) ? 0 : op.kind == OP_LUTM ? __builtin_popcount((unsigned)op_wanted(op)) : 1;
}
// the outputs of any op: a single-destination op is the one-output case
inline int op_outputs(const PendingOp &op) { return op.kind == OP_LUTM ? op.nout : 1; }
inline int32_t &op_dst(PendingOp &op, int m) { return op.kind == OP_LUTM ? op.dsts[m] : op.dst; }
inline int32_t op_dst(const PendingOp &op, int m) { return op.kind == OP_LUTM ? op.dsts[m] : op.dst; }
template <class F>
inline void for_each_dst(const PendingOp &op, F &&f) {
    for (int m = 0; m < op_outputs(op); ++m)
        if (op_dst(op, m) >= 0) f(op_dst(op, m));
}

// prelude constants of the two-input gates: (c0 in eighths, sa, sb), tfhe boot-gates.cpp
struct GateLin { int32_t c8, sa, sb; };
constexpr GateLin GATE_LIN[10] = {
    {1, -1, -1}, {1, 1, 1}, {-1, 1, 1}, {-1, -1, -1}, {2, 2, 2}, {-2, -2, -2},
    {-1, -1, 1}, {-1, 1, -1}, {1, -1, 1}, {1, 1, -1},
};

// prelude coefficient of the three-input gates, by gate: t = s (+-A +- B +- C), c0 = 0 (MAJ3, XOR3, XNOR3); a set
// mask bit flips the sign of its operand's coefficient
constexpr int32_t GATE3_LIN[3] = {1, -2, 2};
inline int32_t gate3_coef(int kind, int operand) {
    const int32_t s = GATE3_LIN[(kind - OP_GATE3) >> 3];
    return ((kind - OP_GATE3) >> operand) & 1 ? -s : s;
}

// A pending op by what it computes: kind, operand slots (-1 = absent), the cloud key it bootstraps under (index in the
// recording's key list: the same gate of the same slots under two keys gives two different ciphertexts) and, for a LUT
// op, the test polynomial, the coefficients and the constant; for a multi-output one the extract spec as well (NOT the
// set of outputs wanted: an equal op that wants another output widens the pending one).  The recorder shares the result
// of two pending ops exactly when these are equal ("reuse_gates").
struct OpKey {
    int32_t kind, a, b, c, key;
    int32_t lut, sa, sb, sc, c0;
    int32_t spec = -1;
    bool operator==(const OpKey &o) const {
        return kind == o.kind && a == o.a && b == o.b && c == o.c && key == o.key && lut == o.lut && sa == o.sa &&
               sb == o.sb && sc == o.sc && c0 == o.c0 && spec == o.spec;
    }
};
struct OpKeyHash {
    size_t operator()(const OpKey &k) const {
        uint64_t h = ((uint64_t)(uint32_t)k.a << 32 | (uint32_t)k.b) * 0x9E3779B97F4A7C15ull;
        h ^= ((uint64_t)(uint32_t)k.c << 8 | (uint32_t)k.kind) * 0xC2B2AE3D27D4EB4Full;
        h ^= (uint64_t)(uint32_t)k.key * 0x165667B19E3779F9ull;
        if (k.kind == OP_LUT || k.kind == OP_LUTM) {
            h ^= ((uint64_t)(uint32_t)k.lut << 32 | (uint32_t)k.c0) * 0xD6E8FEB86659FD93ull;
            h ^= (uint64_t)(uint32_t)(k.spec + 1) * 0x9FB21C651E98DF25ull;
            h ^= ((uint64_t)(uint32_t)k.sa << 40 ^ (uint64_t)(uint32_t)k.sb << 20 ^ (uint32_t)k.sc) * 0xFF51AFD7ED558CCDull;
        }
        return (size_t)(h ^ (h >> 29));
    }
};
// symmetric two-input gates (sa == sb in GATE_LIN: t = c0 + s (A + B)) are keyed with ordered operands; a LUT op is keyed
// as it was given
inline OpKey op_key(const PendingOp &op) {
    int32_t a = op.a, b = op.b;
    if (op.kind < OP_MUX && GATE_LIN[op.kind].sa == GATE_LIN[op.kind].sb && b < a) std::swap(a, b);
    if (op.kind != OP_LUT && op.kind != OP_LUTM) return OpKey{op.kind, a, b, op.c, op.key, -1, 0, 0, 0, 0};
    return OpKey{op.kind, a, b, op.c, op.key, op.lut, op.sa, op.sb, op.sc, op.c0, op.kind == OP_LUTM ? op.spec : -1};
}

// Fills lvl[i] with the level at which ops[i] runs (bootstrapped gates: 1..depth,
// NOTs and linear combinations: 0..depth, executed after the gates of that level; `terms`: the
// table the linear combinations' operands are in, null when there are none).  `unit` = rotations one
// full pass of the latency kernel holds (the CU count); levels are filled to 1, 2
// or 4 units depending on how much work is left per remaining level.  With
// balance == false, or for trivial DAGs, lvl = ASAP.  Returns the depth.
// If alap_out is given it receives each op's ALAP level (== lvl when not balancing).
// cost (tuning "level_slack"; launch_plan.hpp): what a level costs by its width.  Given one, balanced levels go through the
// cost-driven pass (scheduler.cpp relevel_by_cost), which keeps them unless the sum of the levels' costs falls; null or an
// empty table: the levels are the list scheduling's.  report: that sum before and after, and the gates moved.
struct LevelCost;
struct LevelSlackReport { double us_before = 0, us_after = 0; long long moved = 0, pool_slots = 0; };
int schedule_levels(const std::vector<PendingOp> &ops, int asap_depth, bool balance, int unit,
                    std::vector<int32_t> &lvl, std::vector<int32_t> *alap_out = nullptr, const LinTerm *terms = nullptr,
                    const LevelCost *cost = nullptr, LevelSlackReport *report = nullptr);

// The descriptors of a flush (engine.hpp): ops[i] runs at level lvl[i] (schedule_levels), levels in all.  nkeys > 1 (a
// flush of gates under several cloud keys): within a level, descriptors are grouped by ops[i].key.  Linear combinations
// (terms: their table) get their rank here, from the levels they really run at: 1 + the rank of a linear combination of
// the same level whose result they read, else 0; a level's descriptors are ordered by rank, one launch range per rank.
struct LevelPlan;
__attribute__((visibility("hidden"))) LevelPlan build_level_plan(const std::vector<PendingOp> &ops,
                                                                 const std::vector<int32_t> &lvl, int levels, int nkeys = 1,
                                                                 const LinTerm *terms = nullptr);

}  // namespace tfhe_hip
