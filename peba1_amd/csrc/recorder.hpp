// recorder.hpp -- the deferred gate recorder behind the boots* entries (recorder.cpp).  Host logic only.
//
// Every ciphertext value lives in an immutable device slot.  A boots* call allocates a fresh destination slot, records an
// op that reads its operands' CURRENT slots, and re-points the destination handle to the new slot (SSA renaming): safe
// under deferral for a result aliasing an input (Math.cpp:272), a temporary overwritten four times (Math.cpp:34-42),
// temporaries freed right after use (Math.cpp:47-49).  An op's level is 1 + the maximum level of its operand slots; a
// flush executes level 1, 2, ... as batched kernel launches.  bootsCOPY and bootsCONSTANT only re-point handles.
//
// The pending ops live in one graph over slots (op_graph.hpp), which alone shares, widens, levels and eliminates them and
// keeps the one index (OpKey -> the op) and the NOT-origin table.  A record_*_locked binds the pool, gets the operands'
// slots, folds constants, and hands the op to the one record path (record_op in recorder.cpp), single- or
// multi-destination alike: the graph reports the slot of every wanted result, the handles are re-pointed, and immediate
// mode runs the op.  A flush refused for want of device memory changes nothing but what elimination dropped, so it can
// be retried; a successful one clears the graph.
//
// Every function here expects the recorder lock (recorder_lock()) to be held.
#pragma once
#include <cstdint>
#include <mutex>

#include "engine.hpp"
#include "../../include/tfhe/tfhe.h"

namespace tfhe_hip {
#pragma GCC visibility push(hidden)   // library-internal: the exported surface is the C ABI

constexpr int32_t SLOT_HOST = -1;   // LweSample::slot: the value lives in the host mirror
constexpr int32_t SLOT_ZERO = -2;   // fresh sample: trivial encryption of bit 0, (0, -1/8)

// provided by shim.cpp (the array headers): bind the sample's array to `pool` on first device use; the pool it is bound to
void bind_pool(const LweSample *sample, SlotPool *pool);
SlotPool *pool_of_sample(const LweSample *sample);

std::unique_lock<std::recursive_mutex> recorder_lock();
SlotPool *pool_of_key(const TFheGateBootstrappingCloudKeySet *bk);   // uploads the key image at first use

// recording (each refuses a foreign result sample before anything changes)
void record_gate2_locked(int code, LweSample *result, const LweSample *a, const LweSample *b,
                         const TFheGateBootstrappingCloudKeySet *bk);
void record_not_locked(LweSample *result, const LweSample *a, const TFheGateBootstrappingCloudKeySet *bk);
void record_mux_locked(LweSample *result, const LweSample *a, const LweSample *b, const LweSample *c,
                       const TFheGateBootstrappingCloudKeySet *bk);
void record_gate3_locked(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b,
                         const LweSample *c, const TFheGateBootstrappingCloudKeySet *bk);
// t = (0, c0) + coef[0] in[0] (+ coef[1] in[1]) (+ coef[2] in[2]), nin in 1..3 (checked by the caller), bootstrapped from
// test polynomial `lut` of the engine's table and key-switched
void record_lut_locked(int32_t lut, LweSample *result, int nin, const LweSample *const *in, const int32_t *coef, int32_t c0,
                       const TFheGateBootstrappingCloudKeySet *bk);
// the same with several destinations: result[m] (null: not wanted; at least one is, and no two are the same sample --
// checked by the caller) = key switch of output m of extract spec `spec` (nout outputs) of the engine's table
void record_lutm_locked(int32_t lut, int32_t spec, int nout, LweSample *const *result, int nin, const LweSample *const *in,
                        const int32_t *coef, int32_t c0, const TFheGateBootstrappingCloudKeySet *bk);
// result = (0, c0) + sum coef[i] in[i], nin in 1..16 (checked by the caller): no bootstrap, no key switch
void record_linear_locked(LweSample *result, int nin, const LweSample *const *in, const int32_t *coef, int32_t c0,
                          const TFheGateBootstrappingCloudKeySet *bk);
void forget_lutm_locked(int32_t lut, int32_t spec);   // likewise for a multi-output LUT about to be deleted
void forget_lut_locked(int32_t lut);   // a test polynomial about to be deleted: run the recording if an op in it names it
void record_constant_locked(LweSample *result, int32_t value, const TFheGateBootstrappingCloudKeySet *bk);
void record_copy_locked(LweSample *result, const LweSample *a, const TFheGateBootstrappingCloudKeySet *bk);

int32_t alloc_slot(SlotPool *pool);                          // may flush when the pool is dry
int32_t ensure_slot(const LweSample *s, SlotPool *pool);     // a device slot holding the sample's current value
void repoint(LweSample *s, SlotPool *pool, int32_t slot);    // `slot` already retained for the handle
void sync_sample_locked(const LweSample *s);                 // host mirror := current value (flushes if pending)

// levelise, build the plan, execute, release; wait = false leaves the launches in flight (tfhe_hip_flush_async).  Returns
// the number of levels; throws ApiError, with nothing run and everything still recorded, when the scratch cannot be had.
int flush_locked(bool wait = true);
void flush_pending_locked(bool wait = true);   // flush_locked if anything is recorded
void finish_flight_locked();                   // the asynchronous flush (if any) is complete: wait, release what it pinned
void forget_key_locked(const TFheGateBootstrappingCloudKeySet *bk);   // a key about to be deleted: run the recording it is in
bool deferred_mode();
bool set_deferred_locked(bool on);                          // returns the previous mode
bool set_batch_keys_locked(bool on);                        // tuning "batch_keys"; returns the previous setting
// a cost table for the leveller's cost-driven pass in place of the compiled-in ones (count 0: those again), and what the
// pass did at the last flush: {sum of the levels' costs before, after, gates moved, pool slots in use at the flush}
void set_level_cost_locked(const int32_t *widths, const double *us, int count);
void last_level_slack_locked(double *out4);
bool set_recorder_tuning_locked(const char *name, bool on); // reuse_gates, eliminate_dead, fold_constants, balance_levels,
                                                            // batch_keys, level_slack
#pragma GCC visibility pop

}  // namespace tfhe_hip
