// expand.hpp -- seed-compressed cloud keys on the device (include/tfhe_hip.h "seed-compressed cloud keys"): the public
// mask words of a cloud key are regenerated from a ChaCha20 seed straight into the layouts the kernels read, so only the
// bodies cross the bus.  Host-visible side of expand.hip: what each launch works on, and the launchers.
//
// Mask word m of a key is word 2 (m mod 8) + 1 of ChaCha20 block floor(m / 8) under (key, nonce), 64-bit block counter
// from 0 -- what Rng::torus() yields on its m-th call (host_keys.cpp).  The BK's masks come first, in [i][row][u < k][j]
// order, then the KSK's in [i][j][v = 1 .. base-1][q < n] order.  A block is therefore eight mask words.
// A seed-compressed packing key has a stream of its own seed: its masks in [i][p][j] order, which launch_expand_bk writes
// with rows = n t, k = 1.  A seed-compressed ring sample likewise, N words (unpack.hpp).  A seed-compressed LWE sample
// array likewise: the n mask words of sample s are words s n .. s n + n - 1, which launch_lwe_expand writes into slots.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfhe_hip {

struct ExpandSeed { uint32_t key[8], nonce[2]; };

// The raw staging buffer launch_bk_transform reads, [rows][k+1][N] with rows = n (k+1) l: polynomials u < k of a row are
// stream words (mask block (row k + u) N/8 + j/8), polynomial k is the row's uploaded body.  body: [rows][N].  Both
// 16-byte aligned.  One lane per group of eight consecutive words; N is a multiple of 8, so a group is one stream block
// (or eight body words) and never straddles a polynomial.
struct ExpandBkArgs {
    ExpandSeed seed;
    int32_t rows, k, N;
    const int32_t *body;
    int32_t *raw;
};
// The compact key-switching key, [rows + 1][stride] with rows = kN t (base-1): row r gets mask words r n .. r n + n - 1 of
// the KSK's part of the stream (which starts at block first_block = BK mask words / 8), its body at word n, zeros up to
// stride.  The all-zero digit-0 row behind them is the caller's (an explicit clear).  body: [rows].
struct ExpandKskArgs {
    ExpandSeed seed;
    uint64_t first_block;
    int64_t rows;
    int32_t n, stride;
    const int32_t *body;
    int32_t *ksk;
};
// the most stream words one launch_expand_masks call yields
constexpr int EXPAND_MASKS_MAX = 1 << 24;

// A seed-compressed LWE sample array (include/tfhe_hip.h "seed-compressed LWE sample arrays") is a record of
// LWE_SEED_WORDS + record_count words: the mask seed, then one body per sample.  Mask word i of sample s is stream word
// s n + i of the record's seed.  A record holds at most LWE_RECORD_MAX samples: with n <= LWE_EXPAND_MAX_N the last stream
// word index is 2^20 * 2^10 - 1 = 2^30 - 1, so every index, and the end s n + n of every row, stays below 2^31.
constexpr int LWE_SEED_WORDS = 10;
constexpr int LWE_RECORD_MAX = 1 << 20;
constexpr int LWE_EXPAND_MAX_N = 1024;
// the most rows one expand launch writes
constexpr int LWE_EXPAND_CHUNK = 8192;
// One expand launch: row j becomes sample index[j] of the record -- its n mask words, its body at word n, zeros up to
// `stride` -- at rows + slots[j] * stride (the slot pool), or at rows + j * stride when slots is null (scratch rows).
// seed: the record's ten seed words in device memory.  body: body[j] is row j's body when `gathered` (the host forms
// upload only the bodies a chunk names), else body[index[j]] (the whole body array lies on the device).  The caller has
// checked every index (0 <= index[j] < LWE_RECORD_MAX) and every slot; rows is 16-byte aligned, stride a multiple of 4.
struct LweExpandArgs {
    int32_t n, count, stride, gathered;
    const uint32_t *seed;
    const int32_t *body;
    const int32_t *index;
    const int32_t *slots;
    int32_t *rows;
};

// false, and nothing launched, for arguments outside what the kernels were built for
bool launch_lwe_expand(hipStream_t s, const LweExpandArgs &a);
bool launch_expand_bk(hipStream_t s, const ExpandBkArgs &a);
bool launch_expand_ksk(hipStream_t s, const ExpandKskArgs &a);
// test path: out[i] = mask word first_word + i of the stream, i < count, through the kernels' block function
bool launch_expand_masks(hipStream_t s, const ExpandSeed &seed, int64_t first_word, int32_t count, uint32_t *out);

}  // namespace tfhe_hip
