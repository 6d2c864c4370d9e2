// launch_plan.hpp -- which kernel launches a level of a flush turns into (host side, no device code, no runtime calls).
//
// Pure functions of the tunings, the CU count, the parameter set and the level's width (plan_br -> BrPlan, plan_ks_launch ->
// KsLaunchPlan): the engine (engine.cpp prepare_flush / launch_br / launch_ks) builds a plan once per launch and runs it, and
// tests/test_launch_plan_cpu.py reads the same plans through tfhe_hip_test_br_plan / tfhe_hip_test_ks_plan* on a machine
// without a GPU.  Not a file the kernels are built from (peba1_amd/kernel_id.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "br_forms.hpp"

namespace tfhe_hip {

// Tunings of the launch rules (tfhe_hip_set_tuning: br_variant, br8_max_rotations, br_tail8, br_digit_table, ks_tile,
// ks_index, ks_max_splits, ks_matrix and ks_matrix_min; beside them the recorder's reuse_gates / eliminate_dead /
// balance_levels / fold_constants / batch_keys, and the engine's sync_deadline_ms).  The ks_* ones are read by plan_ks and
// ks_splits alone, both called by plan_ks_launch alone.  HISTORY.md lists the forms and knobs removed in round 6.
struct LaunchTunings {
    // which form of the blind-rotate kernel runs wide launches (kernels.hip): -1 = the fastest measured for the ring size
    // (N = 1024: 4-wave; N = 2048: split), 0 = 4-wave (N = 1024), 2 = split (8 waves, half transforms), 4 = 2-wave
    // (N = 1024).  A form whose lazy-arithmetic bounds do not admit the key's gadget is replaced by one that does
    // (plan_br).  Tuning "br_variant", env TFHE_HIP_BR_VARIANT
    int br_variant = -1;
    // launches of at most min(this, CU count) rotations (at most one workgroup per CU) use the 8-wave form
    // of the kernel, N = 1024 only; 0 = never (env TFHE_HIP_BR8_MAX, tuning "br8_max_rotations")
    int br8_max_rotations = 1 << 30;
    // A 4-wave launch whose last round would leave at most one workgroup per CU (count = q * 2 * CUs + r, q >= 1,
    // 0 < r <= CUs) hands those r rotations to the 8-wave form as a second launch: 2.9 ms instead of the 3.75 ms a
    // lone 4-wave workgroup per CU takes (env TFHE_HIP_BR_TAIL8, tuning "br_tail8"; 0 = one launch)
    int br_tail8 = 1;
    // 1 = the first radix-4 step of the forward transforms looks digit products up in LDS (gadget digits
    // of at most 7 bits; split form: stage 0, and the first radix-4 step too where digits have at most 6
    // bits); 2 = split form: stage 0 only; 0 = multiplies (env TFHE_HIP_BR_TABLE, tuning "br_digit_table")
    int br_digit_table = 1;
    // Key switches of a narrow launch are split (power of two <= ks_max_splits) until about ks_target_blocks workgroups
    // exist: beyond filling the chip, more splits mean the blocks in flight share a KSK sub-table small enough for an
    // XCD's L2 (measured optimum of the per-gate kernel: 32 splits).  The tiled launches take any count of coefficient
    // ranges up to ks_max_splits whose grid fills whole rounds of resident workgroups (ks_splits); a cap of 48 measured
    // 56.1 against 61.0 ms per match at 32 (env TFHE_HIP_KS_BLOCKS, not a tuning; tuning "ks_max_splits", env
    // TFHE_HIP_KS_MAX_SPLITS)
    int ks_target_blocks = 32768;
    int ks_max_splits = 48;
    // among the range counts that fill the workgroup slots equally well: 1 = the largest (more, shorter ranges), 0 = the smallest
    // (less partial-sum traffic: one match 55.4 against 56.1 ms; env TFHE_HIP_KS_SPLIT_TIES)
    int ks_split_ties = 0;
    // gates per workgroup of the tiled key switch (16, 24 or 32; 0 = per-gate kernel only); tuning "ks_tile"
    int ks_tile = 16;
    // 1 (default) = the tiled key switch keeps a thread's column of the staged rows in PINNED registers, picked through the
    // VGPR index mode (kernels.hip keyswitch_index_kernel): 56 ms per match; 0 = the LDS-strip form (keyswitch_strip_kernel,
    // tiles of 16): 105 ms -- plain HIP source, the form to fall back on.  Tuning "ks_index", env TFHE_HIP_KS_INDEX
    int ks_index = 1;
    // 1 (default) = a flush's key-switch launches of at least ks_matrix_min gates run as an int8 matrix product on the matrix
    // cores (ks_matrix.hip keyswitch_matrix_kernel) where the tiled kernels would have run and the key holds its byte-plane
    // image: one pass over the image serves 64 gates, no partial sums.  Unpack, pack and the raw entries keep the forms
    // above.  Tunings "ks_matrix" and "ks_matrix_min"
    int ks_matrix = 1;
    int ks_matrix_min = 512;
};

// form_ok[form][tables]: the kernel form's magnitude bounds hold for the gadget (l, Bgbit) at ring size N (br_forms.hpp)
inline void fill_form_ok(bool form_ok[BR_FORM_COUNT][3], int N, int l, int Bgbit) {
    for (int f = 0; f < BR_FORM_COUNT; ++f)
        for (int t = 0; t < 3; ++t) form_ok[f][t] = br_form_admissible(f, N, l, Bgbit, t);
}

// The blind-rotate launches of `count` rotations: kernel form (BR_FORM_*; -1 = no form admits the gadget), digit-table
// mode, and -- 4-wave form only -- tail > 0: the first count - tail rotations on the 4-wave form, the last `tail` on the
// 8-wave form as a second launch.
struct BrPlan { int form; int tables; int tail; };

// stamps: the workgroup-time probe is on (forces the 4-wave form at N = 1024, which alone writes the stamps; forbids the
// 8-wave form and the tail); acc_dump: the caller reads the raw accumulators back (forbids the tail only: the debug
// probes index by workgroup and keep one launch)
inline BrPlan plan_br(const bool form_ok[BR_FORM_COUNT][3], int N, int l, const LaunchTunings &t, int cu_count, int count,
                      bool stamps, bool acc_dump) {
    // the form the tunings ask for ...
    int form;
    if (t.br_variant == 4 && N == 1024) form = BR_FORM_WAVE2;
    else if (t.br_variant == 2 || N == 2048) form = BR_FORM_SPLIT;
    // launches that leave CUs with at most one workgroup: the 8-wave form (a second wave per SIMD)
    else if (t.br8_max_rotations > 0 && count <= std::min(t.br8_max_rotations, cu_count) && l >= 2 && !stamps)
        form = BR_FORM_WAVE8;
    else form = BR_FORM_WIDE4;
    // the workgroup-time probe reads stamps only the 4-wave kernel writes
    if (stamps && N == 1024) form = BR_FORM_WIDE4;
    // ... if its magnitude bounds hold for this key's gadget (br_forms.hpp; every built-in set passes in every form of its
    // ring); else the same form with smaller or no digit tables, else the next form of the order
    int tables = t.br_digit_table < 0 || t.br_digit_table > 2 ? 0 : t.br_digit_table;
    if (!form_ok[form][tables]) {
        static const int order[BR_FORM_COUNT] = {BR_FORM_WIDE4, BR_FORM_SPLIT, BR_FORM_WAVE2, BR_FORM_WAVE8};
        int pick_f = -1, pick_t = 0;
        for (int k = -1; k < BR_FORM_COUNT && pick_f < 0; ++k) {
            const int f = k < 0 ? form : order[k];
            if (f == BR_FORM_WAVE8 && count > cu_count) continue;          // its LDS allows one workgroup per CU only
            for (int tt : {tables, 2, 0})
                if (form_ok[f][tt]) { pick_f = f; pick_t = tt; break; }
        }
        if (pick_f < 0) return BrPlan{-1, 0, 0};
        form = pick_f; tables = pick_t;
    }
    // the last, at most half-filled round of a wide launch on the 8-wave form (descriptors carry their own output
    // index, so a level splits anywhere)
    const int round = 2 * cu_count, tail = count % round;
    const bool split = form == BR_FORM_WIDE4 && t.br_tail8 && count > round && tail > 0 &&
                       tail <= std::min(t.br8_max_rotations, cu_count) && l >= 2 && !acc_dump && !stamps &&
                       form_ok[BR_FORM_WAVE8][tables];
    return BrPlan{form, tables, split ? tail : 0};
}

// The key-switch launch rule (plan_ks_launch below: what the engine sizes the partial sums from, what launch_ks runs and what
// the test entries return): a launch of `count` gates runs in chunks of at most KS_CHUNK gates when tiled (bounds the
// partial-sum buffer: 0.66 GB at P128), each chunk of cnt gates in ks_splits(cnt) coefficient ranges.  Tiles of 24 or 32
// gates exist in the index form only (kernels.hip keyswitch_index_kernel); tile 0 = per-gate kernel only.
constexpr int KS_CHUNK = 8192;
// what the rule reads of a parameter set: nin = k N input coefficients, the key-switch digits, words per ciphertext slot
struct KsShape { int nin, ks_t, ks_basebit, ct_stride; };

// one 16-byte lane per 4 output words, rounded up to a wave: 64 .. 320 threads a workgroup
inline int ks_threads(const KsShape &p) { return ((p.ct_stride / 4 + 63) / 64) * 64; }

// The kernel a launch of `count` gates runs (kernels.hip): one workgroup per (gate, range) [keyswitch_kernel], or a tile of
// gates per workgroup with the staged rows in LDS strips [keyswitch_strip_kernel, tile 16] or in pinned registers
// [keyswitch_index_kernel, tile 16 / 24 / 32].  tile = gates per workgroup, 0 for the per-gate kernel.
// KS_FORM_MATRIX [ks_matrix.hip keyswitch_matrix_kernel]: the whole launch in one grid, tile = its 64 gates a workgroup.
enum KsForm { KS_FORM_PERGATE = 0, KS_FORM_STRIP = 1, KS_FORM_INDEX = 2, KS_FORM_MATRIX = 3 };
constexpr int KS_MATRIX_TILE = 64;
// the matrix form's waves take whole blocks of 32 coefficients each: 8 waves a workgroup (ks_matrix.hpp)
constexpr int KS_MATRIX_SPAN = 256;
// splits: the coefficient ranges (partial sums per range where more than one); filled in by plan_ks_launch
struct KsPlan { int form; int tile; int splits = 1; };

inline int ks_tile_size(const LaunchTunings &t) { return (t.ks_tile > 16 && !t.ks_index) ? 16 : t.ks_tile; }

// The form of a launch or chunk of `count` gates, decided here alone (launch_keyswitch decides nothing).  The tiled kernels
// are built for the key switch of the built-in sets only -- t = 8, base 4 -- for ranges of at most 64 input coefficients and for workgroups of 128, 192 or 320 threads
// (n in 256 .. 511, in 512 .. 767, and n = 1024); they take wide launches, from two tiles on.
// Everything else -- every other accepted (ks_t, ks_basebit), row widths of 64 and 256 threads -- is the per-gate kernel,
// planned as such: the narrow-launch split rule, one chunk.
// matrix: the caller is a flush (engine.cpp prepare_flush) and the key holds its byte-plane image -- only then may the plan
// be the matrix form; unpack and the raw entries pass false, and so does every chunk of a launch that is not the matrix form.
inline KsPlan plan_ks(const LaunchTunings &t, int count, const KsShape &p, bool matrix) {
    const int tile = ks_tile_size(t), threads = ks_threads(p);
    const bool tiled = (tile == 16 || tile == 24 || tile == 32) && count >= 2 * tile && p.ks_t == 8 && p.ks_basebit == 2 &&
                       t.ks_max_splits > 1 && (p.nin + t.ks_max_splits - 1) / t.ks_max_splits <= 64 &&
                       (threads == 128 || threads == 192 || threads == 320);
    if (!tiled) return KsPlan{KS_FORM_PERGATE, 0};
    if (matrix && t.ks_matrix && count >= t.ks_matrix_min && p.nin % KS_MATRIX_SPAN == 0) return KsPlan{KS_FORM_MATRIX, KS_MATRIX_TILE};
    return KsPlan{t.ks_index ? KS_FORM_INDEX : KS_FORM_STRIP, tile};
}

// the coefficient ranges of `cnt` gates in the form `plan` (a tiled form or the per-gate kernel; the matrix form has none)
inline int ks_splits(const LaunchTunings &t, int cu_count, int cnt, const KsShape &p, const KsPlan &plan) {
    int splits = 1;
    if (plan.form != KS_FORM_PERGATE) {
        // the number of coefficient ranges is free between nin/64 and ks_max_splits: take the
        // one whose grid (tiles x ranges) fills whole rounds of the workgroups the chip holds,
        // e.g. 36 tiles x 28 ranges = 1008 of 1024 slots in two rounds instead of 36 x 32 = 1152 in three
        const int tile = plan.tile;
        const int threads = ks_threads(p);
        // index form: no LDS strips; 120 VGPRs at tile 16 (four waves per SIMD), 162 at 24 (three), 204 at 32 (two);
        // strip form: ~235 VGPRs (two waves per SIMD) and 16 x threads x 16 bytes of strips
        int per_cu = std::max(1, (tile == 16 ? 16 : tile == 24 ? 12 : 8) / (threads / 64));
        if (plan.form == KS_FORM_STRIP) {
            const size_t lds = (size_t)16 * threads * 16 + (size_t)tile * 65 * 4;
            per_cu = std::max(1, std::min((int)((160 * 1024) / lds), 8 / (threads / 64)));
        }
        const long long slots = (long long)cu_count * per_cu;
        const long long tiles = (cnt + tile - 1) / tile;
        const int lo = std::max(2, (p.nin + 63) / 64);
        double best = -1.0;
        for (int sp = lo; sp <= t.ks_max_splits; ++sp) {
            const long long blocks = tiles * sp, rounds = (blocks + slots - 1) / slots;
            const double eff = (double)blocks / (double)(rounds * slots);
            // ties: fewer, longer ranges (less partial-sum traffic) or more, shorter ones (ks_split_ties)
            if (t.ks_split_ties ? eff >= best - 1e-9 : eff > best + 1e-9) { best = eff; splits = sp; }
        }
    } else {
        // narrow launches: doubling may pass ks_max_splits once (up to 64)
        while (splits < t.ks_max_splits && cnt * splits * 2 <= t.ks_target_blocks) splits *= 2;
    }
    return splits;
}

// Everything a key-switch launch of `count` gates turns into: `parts` kernel launches, each but the last of `chunk` gates as
// `full` says, the last of the remaining gates as `last` says (one part: the same), and the partial sums the widest of them
// needs.  The matrix form is one part whatever the width, with no partial sums.
struct KsLaunchPlan {
    int count = 0, chunk = 0, parts = 0;
    KsPlan full{}, last{};
    size_t partial_bytes = 0;
    const KsPlan &part(int i) const { return i + 1 < parts ? full : last; }
    int gates(int i) const { return i + 1 < parts ? chunk : count - (parts - 1) * chunk; }
};

// the matrix form of `count` gates (planned below; forced by the raw entry tfhe_hip_kernel_keyswitch_matrix)
inline KsLaunchPlan ks_matrix_plan(int count) {
    const KsPlan part{KS_FORM_MATRIX, KS_MATRIX_TILE, 1};
    return KsLaunchPlan{count, count, 1, part, part, 0};
}

// has_image: plan_ks's `matrix`.  A tiled launch runs in chunks of KS_CHUNK gates; its last chunk is planned by its own width
// and may be narrower than two tiles -- the per-gate kernel.
inline KsLaunchPlan plan_ks_launch(const LaunchTunings &t, int cu_count, int count, const KsShape &p, bool has_image) {
    if (count <= 0) return KsLaunchPlan{};
    auto part_of = [&](int cnt, bool image) {
        KsPlan k = plan_ks(t, cnt, p, image);
        if (k.form != KS_FORM_MATRIX) k.splits = ks_splits(t, cu_count, cnt, p, k);
        return k;
    };
    const KsPlan whole = part_of(count, has_image);
    if (whole.form == KS_FORM_MATRIX) return ks_matrix_plan(count);
    KsLaunchPlan plan{count, whole.form != KS_FORM_PERGATE ? KS_CHUNK : count};
    plan.parts = (count + plan.chunk - 1) / plan.chunk;
    plan.full = plan.parts > 1 ? part_of(plan.chunk, false) : whole;
    plan.last = plan.parts > 1 ? part_of(plan.gates(plan.parts - 1), false) : whole;
    auto bytes = [&](int i) { return plan.part(i).splits > 1 ? (size_t)plan.gates(i) * plan.part(i).splits * p.ct_stride * 4 : 0; };
    plan.partial_bytes = std::max(bytes(0), bytes(plan.parts - 1));
    return plan;
}

// What a level of a flush costs, by its width in rotations: MEASURED microseconds of the blind-rotate launches plan_br
// forms for that width plus the key switch (tools/level_cost.py -> profiles/level_cost_<set>.json).  The leveller
// (scheduler.cpp relevel_by_cost) minimises the sum over a flush's levels; it asks for nothing but this function.
// n == 0: unknown -- the leveller then leaves its levels as they are.
struct LevelCost {
    const int32_t *width = nullptr;     // ascending
    const double *us = nullptr;
    int n = 0;
    // beyond the table a launch repeats its last `period` rotations (a full round of the wide form: 2 workgroups per CU);
    // 0 = the last segment's slope goes on
    int period = 0;
};

// how many periods to take off a width beyond the table so that it falls into the table's last period
inline long long level_cost_fold(const LevelCost &c, long long width) {
    const long long top = c.width[c.n - 1];
    if (width <= top || c.period <= 0 || c.period > top - c.width[0]) return 0;
    return (width - top + c.period - 1) / c.period;
}

// 0 for an empty level, the first entry below it, linear between entries; beyond the table see `period`
inline double level_cost_at(const LevelCost &c, long long width) {
    if (width <= 0 || c.n <= 0) return 0.0;
    if (width <= c.width[0] || c.n == 1) return c.us[0];
    const long long top = c.width[c.n - 1], fold = level_cost_fold(c, width);
    if (fold > 0) return level_cost_at(c, width - fold * c.period) + (double)fold * (c.us[c.n - 1] - level_cost_at(c, top - c.period));
    const int32_t *hi = std::lower_bound(c.width, c.width + c.n, (int32_t)std::min<long long>(width, top));
    const int j = (int)(hi - c.width);
    return c.us[j - 1] + (c.us[j] - c.us[j - 1]) * (double)(width - c.width[j - 1]) / (double)(c.width[j] - c.width[j - 1]);
}

// The table's own widths next to `width`, nearest first -- where its cost steps are: up to `most` below it (dir < 0) or above
// it (dir > 0), beyond the table those of the last period shifted.  Returns how many.
inline int level_cost_steps(const LevelCost &c, long long width, int dir, long long *out, int most) {
    if (c.n <= 0) return 0;
    const long long shift = level_cost_fold(c, width) * c.period, at = width - shift;
    int count = 0;
    if (dir < 0) {
        for (int j = (int)(std::lower_bound(c.width, c.width + c.n, (int32_t)std::min<long long>(at, INT32_MAX)) - c.width) - 1;
             j >= 0 && count < most; --j)
            out[count++] = c.width[j] + shift;
    } else {
        for (int j = (int)(std::upper_bound(c.width, c.width + c.n, (int32_t)std::min<long long>(at, INT32_MAX)) - c.width);
             j < c.n && count < most; ++j)
            out[count++] = c.width[j] + shift;
    }
    return count;
}

// The compiled-in copies of the measured tables: level_cost_tables.inc, written by tools/level_cost_inc.py from
// profiles/level_cost_*.json when the library is built (absent: no table, every set unknown).
struct LevelCostEntry {
    int n, N, k, l, Bgbit, ks_t, ks_basebit;      // the parameter set ...
    int cus;                                      // ... the card ...
    int br_variant, br8_max_rotations, br_tail8, br_digit_table, ks_tile, ks_index, ks_max_splits, ks_target_blocks,
        ks_split_ties, ks_matrix, ks_matrix_min;  // ... and the tunings it was measured under
    int count;
    const int32_t *width;
    const double *us;
};
#if __has_include("level_cost_tables.inc")
#include "level_cost_tables.inc"
#else
#warning "level_cost_tables.inc is missing (run tools/level_cost_inc.py before peba1_amd/csrc/build.sh): this library knows no level-cost table and the tuning level_slack does nothing"
static constexpr LevelCostEntry LEVEL_COST_TABLES[1] = {};
static constexpr int LEVEL_COST_TABLE_COUNT = 0;
#endif

// what a parameter set is to the tables: the sizes the launches depend on
struct LevelCostSet { int n, N, k, l, Bgbit, ks_t, ks_basebit; };

// the table of this set on a card of `cus` CUs under these tunings; unknown (n == 0) unless all three are what a table was
// measured with -- a launch rule switched by a tuning has other cost steps
inline LevelCost level_cost_table(const LevelCostSet &p, int cus, const LaunchTunings &t) {
    for (int i = 0; i < LEVEL_COST_TABLE_COUNT; ++i) {
        const LevelCostEntry &e = LEVEL_COST_TABLES[i];
        if (e.n == p.n && e.N == p.N && e.k == p.k && e.l == p.l && e.Bgbit == p.Bgbit && e.ks_t == p.ks_t &&
            e.ks_basebit == p.ks_basebit && e.cus == cus && e.br_variant == t.br_variant &&
            e.br8_max_rotations == t.br8_max_rotations && e.br_tail8 == t.br_tail8 && e.br_digit_table == t.br_digit_table &&
            e.ks_tile == t.ks_tile && e.ks_index == t.ks_index && e.ks_max_splits == t.ks_max_splits &&
            e.ks_target_blocks == t.ks_target_blocks && e.ks_split_ties == t.ks_split_ties && e.ks_matrix == t.ks_matrix &&
            e.ks_matrix_min == t.ks_matrix_min)
            return LevelCost{e.width, e.us, e.count, 2 * e.cus};
    }
    return LevelCost{};
}

// microseconds of a level of `width` rotations, -1 = unknown
inline double level_cost_us(int width, const LevelCostSet &p, int cus, const LaunchTunings &t) {
    const LevelCost c = level_cost_table(p, cus, t);
    return c.n ? level_cost_at(c, width) : -1.0;
}

}  // namespace tfhe_hip
