// kernels.hpp -- host-visible declarations of the HIP kernels' launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfhe_hip {

struct ExtractSpec;

// Parameters of one key as the kernels see them.
struct DevParams {
    int32_t n, N, k, l, Bgbit, ks_t, ks_basebit;
    int32_t kpl;            // (k+1) l
    int32_t ct_stride;      // words per ciphertext slot: n+1 rounded up to 4
    int32_t u_stride;       // words per extracted sample: kN+1 rounded up to 4
    uint32_t decomp_offset; // sum_j (Bg/2) 2^{32-j Bgbit}
    uint32_t ks_prec_offset;// 2^{32-(1+basebit t)}
    int32_t mu;             // test-vector amplitude, 1/8
    int32_t digit_table;    // 1 = digit products of the first NTT step from an LDS table where Bgbit allows (kernels.hip)
    int32_t br_variant;     // 2 = split transforms: only read by the negacyclic test launcher
    unsigned long long *clock_acc;  // kernel timing: [2] running sums of shader cycles (s_memtime) and of 100 MHz ticks
                                    // (s_memrealtime) over every 61st workgroup of every blind-rotate launch -> the shader
                                    // clock the launches ran at; or null
    unsigned long long *wg_times;   // diagnostic: [4 * grid] s_memtime (shader cycles) at workgroup start and end, then
                                    // s_memrealtime (100 MHz) at start and end; or null
    const int32_t *luts;            // table of caller-supplied test polynomials, LUT_STRIDE words apiece (RotDesc::lut indexes
                                    // it); null when no rotation of the launch names one
    const ExtractSpec *specs;       // table of extract specs (RotDesc::spec indexes it); null when no rotation of the launch
                                    // names one
};

// words between two test polynomials of a LUT table: the largest ring, so that one table serves every parameter set
constexpr int LUT_STRIDE = 2048;

// What leaves one blind rotation when more than coefficient 0 is wanted (tfhe_hip_lut_bootstrap_multi): output m is
//     (0, out_c0[m]) + sum_{t < ntaps[m]} weight[m][t] * Extract_{index[m][t]}(ACC)          (include/tfhe_hip.h)
// Plain words, the same on host and device; the limits are checked before a spec reaches a table (extract_spec_error).
constexpr int XS_MAX_OUT = 4, XS_MAX_TAPS = 8, XS_MAX_WEIGHT = 8;
struct ExtractSpec {
    int32_t nout;
    int32_t ntaps[XS_MAX_OUT];
    int32_t out_c0[XS_MAX_OUT];
    int32_t index[XS_MAX_OUT][XS_MAX_TAPS];
    int32_t weight[XS_MAX_OUT][XS_MAX_TAPS];
};
constexpr int XS_WORDS = sizeof(ExtractSpec) / sizeof(int32_t);
// RotDesc::spec, when >= 0: the table entry in the low bits, above them the set of outputs that are written (bit m =
// output m; an output nobody reads -- a null result, a dead one -- is neither extracted nor key-switched)
constexpr int XS_WANTED_SHIFT = 24;
constexpr int32_t XS_ENTRY_MASK = (1 << XS_WANTED_SHIFT) - 1;
// null if `xs` is within the limits for ring size N, else what is wrong with it
inline const char *extract_spec_error(const ExtractSpec &xs, int N) {
    if (xs.nout < 1 || xs.nout > XS_MAX_OUT) return "nout must be 1..4";
    for (int m = 0; m < xs.nout; ++m) {
        if (xs.ntaps[m] < 1 || xs.ntaps[m] > XS_MAX_TAPS) return "an output takes 1..8 taps";
        for (int t = 0; t < xs.ntaps[m]; ++t) {
            if (xs.index[m][t] < 0 || xs.index[m][t] >= N) return "a tap index outside 0..N-1";
            if (xs.weight[m][t] == 0 || xs.weight[m][t] > XS_MAX_WEIGHT || xs.weight[m][t] < -XS_MAX_WEIGHT)
                return "a tap weight that is zero or beyond +-8";
            for (int s = 0; s < t; ++s)
                if (xs.index[m][s] == xs.index[m][t]) return "two taps of one output at the same index";
        }
    }
    return nullptr;
}

// Device-resident evaluation key.
struct DevKey {
    const uint32_t *bk_img;  // [n][kpl][prime 2][w 2][N] NTT image, Montgomery form, x N^-1
    const int32_t *ksk;      // [kN][t][base-1][ct_stride]
    const int32_t *ksk_zero; // one more row of ct_stride zeros (digit 0 of the key switch)
    const uint32_t *tw;      // [prime 2][fwd, inv][N] twiddles, Montgomery form, then the radix-4 quads
                             // [prime 2][fwd, inv][N/2][4] = {w2, w3, w1 w2, P - w1 w3} (ntt_wave.hpp): 12N words;
                             // then the same for the two half transforms of the split kernels, 6N words each
};

// One blind rotation: t = (0, c0) + sa * slot_a + sb * slot_b (+ sc * slot_c), then
// modswitch, blind rotate, sample extract into u_buf[u_index].  slot_c = -1: no third operand (every upstream gate);
// the three-input gates of tfhe_hip_gate3 set it.  The kernels read slot_c's words only when it is >= 0.
// lut < 0: the accumulator starts from the constant test vector mu (1 + X + ... + X^(N-1)) of every gate; lut >= 0
// (tfhe_hip_lut_bootstrap): from test polynomial `lut` of DevParams::luts, read only then.
// spec < 0: the sample extract at index 0 into u_buf[u_index]; spec >= 0 (tfhe_hip_lut_bootstrap_multi): the outputs of
// extract spec `spec & XS_ENTRY_MASK` of DevParams::specs, output m into u_buf[u_index + m] if bit m of
// spec >> XS_WANTED_SHIFT is set.  Read after the step loop only.
struct RotDesc {
    int32_t slot_a, slot_b;
    int32_t sa, sb;
    int32_t c0;
    int32_t u_index;
    int32_t slot_c = -1;
    int32_t sc = 0;
    int32_t lut = -1;
    int32_t spec = -1;
};

// One key switch: (u_buf[u0] (+ u_buf[u1]) + (0, add_b)) -> pool[dst_slot].
struct KsDesc {
    int32_t u0, u1;   // u1 = -1 when absent
    int32_t add_b;
    int32_t dst_slot;
};

struct NotDesc { int32_t src_slot, dst_slot; };

// One linear combination (tfhe_hip_linear): pool[dst_slot] = (0, c0) + sum_{t < nin} coef[t] * pool[slot[t]], wrapping
// mod 2^32 on every word; dst_slot is none of slot[].  Entries from nin on are not read.
constexpr int LIN_DESC_MAX_IN = 16;
struct LinDesc {
    int32_t dst_slot, nin, c0;
    int32_t slot[LIN_DESC_MAX_IN];
    int32_t coef[LIN_DESC_MAX_IN];
};


void launch_bk_transform(hipStream_t s, const DevParams &p, const int32_t *raw_polys, uint32_t *img,
                         const uint32_t *tw, int npoly_per_w, int nw, const uint32_t scale[2]);
// 2-wave form (N = 1024): the admissibility fallback (br_forms.hpp BR_FORM_WAVE2)
void launch_blind_rotate2(hipStream_t s, const DevParams &p, const DevKey &key, const int32_t *pool,
                          const RotDesc *rots, int count, int32_t *u_buf, int32_t *acc_dbg);
// 4-wave form (N = 1024): the streaming form, two workgroups per CU
void launch_blind_rotate4(hipStream_t s, const DevParams &p, const DevKey &key, const int32_t *pool,
                          const RotDesc *rots, int count, int32_t *u_buf, int32_t *acc_dbg);
// 8-wave form (N = 1024, l >= 2) for launches of at most one workgroup per CU: a second wave per SIMD
void launch_blind_rotate8(hipStream_t s, const DevParams &p, const DevKey &key, const int32_t *pool,
                          const RotDesc *rots, int count, int32_t *u_buf, int32_t *acc_dbg);
// multi-key forms of the 4- and 8-wave launches (tuning "batch_keys"): rotation i runs under the key image
// keys[rot_keys[i]].bk_img (device table and indices); the twiddles come from key0, the same for every key of the set
void launch_blind_rotate4_mk(hipStream_t s, const DevParams &p, const DevKey &key0, const DevKey *keys, const int32_t *rot_keys,
                             const int32_t *pool, const RotDesc *rots, int count, int32_t *u_buf);
void launch_blind_rotate8_mk(hipStream_t s, const DevParams &p, const DevKey &key0, const DevKey *keys, const int32_t *rot_keys,
                             const int32_t *pool, const RotDesc *rots, int count, int32_t *u_buf);
// split form (8 waves per rotation, every transform as two half-size ones; N = 1024 or 2048)
void launch_blind_rotate_split(hipStream_t s, const DevParams &p, const DevKey &key, const int32_t *pool,
                               const RotDesc *rots, int count, int32_t *u_buf, int32_t *acc_dbg);
// The key switches of `count` gates in the form the planner chose (launch_plan.hpp plan_ks; nothing is decided here).
// splits > 1: each gate's key switch is cut into `splits` ranges of input coefficients (partial sums in
// `partial[count][splits][ct_stride]`, then a reduce launch).  tile = 0: one workgroup per (gate, range); tile = 16, 24 or
// 32: a tiled kernel (one pass over the KSK rows of a range serves `tile` gates) -- the index form (rows in pinned registers
// picked through the VGPR index mode: keyswitch_index_kernel) or, index = false, the LDS-strip form (tile 16 only:
// keyswitch_strip_kernel).  Returns false and launches nothing for a form without an instantiation.
bool launch_keyswitch(hipStream_t s, const DevParams &p, const DevKey &key, const int32_t *u_buf,
                      const KsDesc *descs, int count, int32_t *pool, int splits, int32_t *partial, int tile,
                      bool index = true);
void launch_not(hipStream_t s, const DevParams &p, const NotDesc *descs, int count, int32_t *pool);
void launch_linear(hipStream_t s, const DevParams &p, const LinDesc *descs, int count, int32_t *pool);
// res[c] = ip[c] * (poly whose image is img[c]) through the device NTT
void launch_negacyclic(hipStream_t s, const DevParams &p, const uint32_t *tw, const int32_t *ip,
                       const uint32_t *img, int32_t *res, int count);


void launch_gather_slots(hipStream_t s, const int32_t *pool, int stride, int words, const int32_t *slots, int count,
                         int32_t *packed);
void launch_scatter_slots(hipStream_t s, int32_t *pool, int stride, int words, const int32_t *slots, int count,
                          const int32_t *packed);

}  // namespace tfhe_hip
