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
#include <cstdint>
#include <vector>

namespace tfhe_hip {

struct PendingOp {
    uint8_t kind;       // 0..9 two-input gate code, OP_MUX, OP_NOT, OP_GATE3 + 8 gate + negation mask
    int32_t dst, a, b, c;   // slots; b, c = -1 when absent
    int32_t level;      // ASAP level (NOT: the level of its operand, 0 = already materialised)
    uint16_t key = 0;   // index of the gate's cloud key in the flush's key list (recorder "batch_keys"; NOT: unused)
};
constexpr uint8_t OP_MUX = 16, OP_NOT = 17;
// three-input gates (tfhe_hip_gate3; not in upstream's API): kind = OP_GATE3 + 8 * gate + mask, gate = enum TfheHipGate3,
// bit i of mask negates operand i (a = bit 0) -- 32..55.  The mask is part of the kind, hence of the recorder's index key
constexpr uint8_t OP_GATE3 = 32, OP_GATE3_END = OP_GATE3 + 3 * 8;
inline bool op_is_gate3(int kind) { return kind >= OP_GATE3 && kind < OP_GATE3_END; }
inline bool op_kind_valid(int kind) { return (kind >= 0 && kind < 10) || kind == OP_MUX || kind == OP_NOT || op_is_gate3(kind); }

inline int op_rotations(const PendingOp &op) { return op.kind == OP_NOT ? 0 : (op.kind == OP_MUX ? 2 : 1); }

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

// Fills lvl[i] with the level at which ops[i] runs (bootstrapped gates: 1..depth,
// NOTs: 0..depth, executed after the gates of that level).  `unit` = rotations one
// full pass of the latency kernel holds (the CU count); levels are filled to 1, 2
// or 4 units depending on how much work is left per remaining level.  With
// balance == false, or for trivial DAGs, lvl = ASAP.  Returns the depth.
// If alap_out is given it receives each op's ALAP level (== lvl when not balancing).
int schedule_levels(const std::vector<PendingOp> &ops, int asap_depth, bool balance, int unit,
                    std::vector<int32_t> &lvl, std::vector<int32_t> *alap_out = nullptr);

// The descriptors of a flush (engine.hpp): ops[i] runs at level lvl[i] (schedule_levels), levels in all.  nkeys > 1 (a
// flush of gates under several cloud keys): within a level, descriptors are grouped by ops[i].key.
struct LevelPlan;
__attribute__((visibility("hidden"))) LevelPlan build_level_plan(const std::vector<PendingOp> &ops,
                                                                 const std::vector<int32_t> &lvl, int levels, int nkeys = 1);

}  // namespace tfhe_hip
