/*
 * tfhe_hip.h -- extensions of libtfhe-hip beyond the upstream tfhe C API.
 *
 * Everything here is plain C ABI (pointers and sizes, no C++/torch types).  The
 * upstream-compatible surface is in tfhe/tfhe_gate_bootstrapping_functions.h;
 * this header adds what a one-gate-per-call API cannot express: seeded keys,
 * deferred (batched, levelised) execution, array-wide gates, raw ciphertext
 * words, statistics, and kernel-level entry points used by the parity tests.
 */
#ifndef TFHE_HIP_H
#define TFHE_HIP_H

#include <stdio.h>

#include "tfhe/tfhe_core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gate codes for tfhe_hip_gate_batch (2-input gates share one kernel and differ
 * only in the linear prelude) */
enum TfheHipGate {
    TFHE_HIP_NAND = 0, TFHE_HIP_OR, TFHE_HIP_AND, TFHE_HIP_NOR, TFHE_HIP_XOR, TFHE_HIP_XNOR,
    TFHE_HIP_ANDNY, TFHE_HIP_ANDYN, TFHE_HIP_ORNY, TFHE_HIP_ORYN
};

/* ---- error channel: the upstream API returns void everywhere, so failures
 * are reported here.  Conditions the caller can recover from -- ciphertext slot pool exhausted,
 * a sample this library did not allocate, a sample used with a key of another LWE dimension,
 * a null key, a malformed / truncated / foreign file -- leave the call WITHOUT EFFECT (result
 * untouched; loaders return NULL; int entry points return -1) and set the message.  Only HIP
 * runtime failures and "no GPU present" abort the process, like upstream's fatal paths. ---- */
const char *tfhe_hip_last_error(void);
void tfhe_hip_clear_error(void);

/* ---- device selection (call before the first keyset is created) ---- */
int tfhe_hip_set_device(int device);
int tfhe_hip_get_device(void);
/* PCI bus id ("0000:c1:00.0", NUL-terminated; len >= 16) of the device the library runs on: what a multi-GPU job prints
 * per rank to show that N ranks drive N distinct GPUs (bench.py `dist.devices`).  Initialises the engine.  Returns 0 / -1.
 * The library binds the calling thread to its device only for the duration of the calls that reach the HIP runtime and
 * gives the caller's current device back on return. */
int tfhe_hip_device_pci_bus_id(char *out, int len);

/* ---- parameters ---- */
TFheGateBootstrappingParameterSet *tfhe_hip_new_parameters(
    int32_t n, int32_t N, int32_t k, int32_t l, int32_t Bgbit, int32_t ks_t, int32_t ks_basebit,
    double ks_stdev, double bk_stdev, double max_stdev);
/* BASELINE.json configs[4]: N=2048, Bg=2^6, l=3 (n=1024, ks 8x2 bit fixed by this repo) */
TFheGateBootstrappingParameterSet *tfhe_hip_new_p2048_parameters(void);

/* ---- randomness ----
 * Default (new_random_gate_bootstrapping_secret_keyset, bootsSymEncrypt): ChaCha20 key streams (RFC 8439 block
 * function), each under its own 256-bit key + 64-bit nonce from getrandom(); the secrets (key bits, every noise
 * sample) and the public masks (bk / ksk masks, the `a` words of ciphertexts) come from two independently keyed
 * streams.  No OS entropy = abort with a message.
 * The entry points below replace that with the SEEDED generator of the key-derivation specification this library
 * shares with the test oracle (xoshiro256** through splitmix64, one stream for secrets and masks):
 * reproducible and NOT cryptographic -- for tests and golden fixtures only, never for keys that protect data. ---- */
TFheGateBootstrappingSecretKeySet *tfhe_hip_new_secret_keyset_seeded(
    const TFheGateBootstrappingParameterSet *params, uint64_t seed);
/* host-only keyset (no device upload): lets CPU-only tests check key derivation */
TFheGateBootstrappingSecretKeySet *tfhe_hip_new_secret_keyset_seeded_host(
    const TFheGateBootstrappingParameterSet *params, uint64_t seed);
void tfhe_hip_set_encrypt_seed(uint64_t seed);
/* 1 after tfhe_hip_set_encrypt_seed (bootsSymEncrypt is reproducible, not secure), else 0 */
int tfhe_hip_randomness_is_seeded(void);
/* known-answer hook for the default generator: ChaCha20 key-stream block of (key[8], 64-bit counter, nonce[2]);
 * RFC 8439 2.3.2 = counter 1 | 0x09000000 << 32, nonce {0x4a000000, 0} */
void tfhe_hip_test_chacha20_block(const uint32_t *key8, uint64_t counter, const uint32_t *nonce2, uint32_t *out16);

/* read-only views of the key material (parity tests hash these) */
const int32_t *tfhe_hip_key_lwe(const TFheGateBootstrappingSecretKeySet *key, int64_t *count);
const int32_t *tfhe_hip_key_tlwe(const TFheGateBootstrappingSecretKeySet *key, int64_t *count);
const Torus32 *tfhe_hip_key_bk(const TFheGateBootstrappingCloudKeySet *cloud, int64_t *count);
const Torus32 *tfhe_hip_key_ksk(const TFheGateBootstrappingCloudKeySet *cloud, int64_t *count);

/* ---- raw ciphertext words: n mask words then the body ---- */
int32_t tfhe_hip_sample_words(const TFheGateBootstrappingParameterSet *params);
/* samples[0..count) are consecutive elements of one array; words are packed
 * [count][n+1].  One call moves at most 65,536 samples through the device: more are refused ("too many samples in one
 * packed transfer") with nothing changed.
 * An import beside a recording: every imported sample is renamed into a fresh slot, so recorded operations that have not
 * run stay recorded and keep the samples they named -- one that reads the handle still reads the sample it held when the
 * operation was recorded, and one whose result the handle held still runs (unless "eliminate_dead" finds its result
 * unread) and writes the slot it was given, never the imported one.  A flush in flight is not waited for: the import is
 * enqueued behind it on tfhe_hip_stream().  An export is an observation point: the recorded operations run first.
 * Host mirrors: the host-form import sets sample->a / sample->b to the imported words in either mode; the device forms
 * leave them stale, in immediate mode too, until the sample is passed to tfhe_hip_sync_samples(). */
int tfhe_hip_export_samples(const LweSample *samples, int32_t count,
                            const TFheGateBootstrappingParameterSet *params, Torus32 *out_words);
int tfhe_hip_import_samples(LweSample *samples, int32_t count,
                            const TFheGateBootstrappingParameterSet *params, const Torus32 *in_words);
/* same, to/from DEVICE memory (e.g. a torch tensor's data_ptr) for collectives */
int tfhe_hip_export_samples_device(const LweSample *samples, int32_t count,
                                   const TFheGateBootstrappingParameterSet *params, void *device_words);
int tfhe_hip_import_samples_device(LweSample *samples, int32_t count,
                                   const TFheGateBootstrappingParameterSet *params, const void *device_words);
/* Stream-ordered forms for collectives driven from the host language (libpeba1-dist): the transfer is ENQUEUED on
 * the library's own HIP stream, tfhe_hip_stream(), and the call returns without waiting.  Anything the caller then
 * enqueues on that same stream -- an RCCL collective on the exported buffer, or the next flush after an import -- is
 * ordered behind it by the stream itself, with no host synchronisation.  The buffer must stay allocated until the
 * stream has passed the transfer (hipStreamSynchronize(tfhe_hip_stream()), or an event). */
int tfhe_hip_export_samples_device_async(const LweSample *samples, int32_t count,
                                         const TFheGateBootstrappingParameterSet *params, void *device_words);
int tfhe_hip_import_samples_device_async(LweSample *samples, int32_t count,
                                         const TFheGateBootstrappingParameterSet *params, const void *device_words);
/* the hipStream_t every kernel and transfer of this library runs on (created non-blocking, highest priority) */
void *tfhe_hip_stream(void);
/* Every read of a sample by the host (bootsSymDecrypt, tfhe_hip_sync_samples, the exports) is ordered behind whatever
 * was enqueued on that stream before it -- a flush in flight, a stream-ordered import behind a collective -- and
 * tfhe_hip_wait() returns only when all of it has completed. */
/* refresh the host mirror (a, b) of samples whose value lives on the device */
int tfhe_hip_sync_samples(const LweSample *samples, int32_t count);

/* ---- execution mode ----
 * deferred (default): boots* calls are recorded (SSA-renamed, so overwritten and freed
 * temporaries are safe), levelised by data dependence, and executed level by level as batched
 * kernels at the next bootsSymDecrypt / export / tfhe_hip_flush() (and on their own before the
 * slot pool runs dry).  Everything observable through the API is identical to per-call
 * execution; only the public struct fields sample->a / sample->b are stale until the sample
 * is decrypted, exported or passed to tfhe_hip_sync_samples().
 * immediate (TFHE_HIP_DEFERRED=0 in the environment, or tfhe_hip_set_deferred(0)): every
 * boots* call is complete on return with the host mirror refreshed, as upstream -- one gate
 * per kernel launch, 3.4 ms per gate. */
void tfhe_hip_set_deferred(int on);
int tfhe_hip_get_deferred(void);
int tfhe_hip_flush(void);   /* returns the number of levels executed, <0 on error */
/* Pipelined form for a stream of circuits (a server matching one probe after another): the pending gates are levelised and
 * their launches ENQUEUED, and the call returns while the device works.  The caller goes on recording the next circuit --
 * its recording, the elimination of dead gates, the levelling and the plan of its own flush all overlap the execution of
 * this one (at most one flush is in flight: the next flush waits for it just before it launches).  Everything that
 * observes a result (bootsSymDecrypt, exports, tfhe_hip_sync_samples, tfhe_hip_get_stats) waits first;
 * tfhe_hip_wait() waits explicitly.  tfhe_hip_flush() is the synchronous form and also completes a flush in flight. */
int tfhe_hip_flush_async(void);
int tfhe_hip_wait(void);

/* ---- bounded host waits (multi-process runs) ----
 * "sync_deadline_ms" (tfhe_hip_set_tuning; env TFHE_HIP_SYNC_DEADLINE_MS; default 0 = wait for ever): when > 0, no
 * host wait on the library's stream lasts longer than this.  A wait that does -- a collective whose peer never
 * arrived, a kernel that never ends -- prints what was waited for and the label below on stderr and ends the process
 * with exit code TFHE_HIP_EXIT_DEADLINE (_exit: no retry, no re-exec -- the state of the device is unknown).
 * libpeba1-dist sets it for every communicator of more than one rank (PEBA1_DIST_TIMEOUT_S, default 600 s). */
#define TFHE_HIP_EXIT_DEADLINE 86
/* waits (bounded as above) until everything enqueued on tfhe_hip_stream() so far -- by this library or by the caller
 * (a collective) -- has completed; also completes a flush in flight.  Returns 0. */
int tfhe_hip_stream_sync(void);
/* waits (bounded as above) for a HIP event of the caller's own (a hipEvent_t recorded on any stream of the library's
 * device) -- libpeba1-dist reads the status words of a collective back this way, from a stream of its own, without waiting
 * for the gates in flight on tfhe_hip_stream().  `what` names the wait in the deadline message.  Returns 0. */
int tfhe_hip_wait_event(void *hip_event, const char *what);
/* who is waiting, for that message ("rank 3 of 8: gather of the partial sums"); copied, at most 127 characters */
void tfhe_hip_set_diag_label(const char *label);

/* result[i] = gate(a[i], b[i]) for i < count, one batched launch */
int tfhe_hip_gate_batch(int gate, LweSample *result, const LweSample *a, const LweSample *b,
                        int32_t count, const TFheGateBootstrappingCloudKeySet *bk);

/* ---- three-input gates: NOT PART OF UPSTREAM TFHE'S API.  With the +-1/8 encoding and the constant test vector every
 * gate uses, one bootstrap also evaluates the majority and the parity of three bits, so sum and carry of a full adder
 * are 2 bootstraps at depth 1.  The words are this library's own, defined by integers: the result is the bootstrap (test
 * vector and mu = 1/8 as for every gate) and key switch of
 *     t = sa A + sb B + sc C      (wrapping mod 2^32 on all n+1 words; no constant term)
 * with (sa, sb, sc) = (+1, +1, +1) for MAJ3, (-2, -2, -2) for XOR3, (+2, +2, +2) for XNOR3; bit i of negate_mask (a = bit
 * 0, b = bit 1, c = bit 2) flips the sign of operand i's coefficient -- the gate of the NEGATED operand, at no cost:
 * borrow = MAJ3(!a, b, c) is tfhe_hip_gate3(TFHE_HIP_MAJ3, 1, ...).  One blind rotation and one key switch per gate.
 * Noise: the sum of three samples stands 1/8 (MAJ3) or 1/4 (XOR3) from the decision boundary like AND / XOR do, under
 * three input noises instead of two.  Recorded in deferred mode (shared, eliminated and levelled like every gate), complete
 * on return in immediate mode; "fold_constants" turns a gate with a constant operand into the two-input gate with the same
 * truth table (MAJ3 with 0 -> AND, with 1 -> OR; XOR3 with 0 -> XOR, with 1 -> XNOR; negations carried into ANDNY / ANDYN
 * / NOR / ORNY / ORYN / NAND / XOR / XNOR), bootstrapped with exactly the words bootsAND etc. give.  Errors as for every
 * boots* entry: tfhe_hip_last_error(), call without effect. ---- */
enum TfheHipGate3 { TFHE_HIP_MAJ3 = 0, TFHE_HIP_XOR3, TFHE_HIP_XNOR3 };
void tfhe_hip_gate3(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b,
                    const LweSample *c, const TFheGateBootstrappingCloudKeySet *bk);
/* result[i] = gate3(a[i], b[i], c[i]) for i < count, one batched launch; 0 / -1 */
int tfhe_hip_gate3_batch(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b,
                         const LweSample *c, int32_t count, const TFheGateBootstrappingCloudKeySet *bk);

/* ---- programmable bootstrap (LUT gates): NOT PART OF UPSTREAM TFHE'S GATE API.  Every gate above starts its blind rotation
 * from one test polynomial, mu (1 + X + ... + X^(N-1)) with mu = 1/8.  Here the caller supplies it: a LUT is N Torus32 words
 * v[0..N-1] bound to a parameter set, and a LUT bootstrap evaluates the negacyclic table v on the phase of a linear
 * combination of up to three samples -- a sign at another amplitude, a re-encoding, a multi-valued table, a noise refresh.
 * Upstream has the same below its gate API (tfhe_bootstrap_FFT takes any mu, tfhe_blindRotateAndExtract_FFT any test vector).
 * The words are this library's own, defined by integers:
 *     t = (0, c0) + coef[0] in[0] (+ coef[1] in[1]) (+ coef[2] in[2])     (wrapping mod 2^32 on all n+1 words)
 *     (abar_i, bbar) = the modulus switch of t to Z_2N, as for every gate
 *     ACC = (0, X^-bbar v): body coefficient j is v[j + bbar] for an index (mod 2N) below N, -v[index - N] otherwise
 *     then the n CMUX steps, the sample extract at index 0 and the key switch of every gate, unchanged.
 * With v[j] = 2^29 for every j the words are those of the gate with the same prelude (bootsAND: coef (1, 1), c0 = -2^29).
 * Parity is against the test oracle's pieces (accumulator, CMUX steps, extract, key switch), not against a boots* call.
 * Decrypted: the result's phase is v[p] for p = bbar - sum abar_i s_i mod 2N below N, -v[p - N] otherwise, plus noise.
 * A LUT can be made, read and deleted without a GPU; its words reach the device at the first bootstrap that names it
 * (device memory exhausted there: the error channel, call without effect).  Deleting a LUT runs the recording first if a
 * recorded bootstrap names it, as deleting a keyset does.
 * tfhe_hip_new_lut: v[N] is copied.  _constant: v[j] = mu (upstream's tfhe_bootstrap test vector).  _from_table: v[j] =
 * values[j * slots / N]; slots must divide N.  NULL and the error channel on bad arguments.
 * tfhe_hip_lut_words: a read-only view of the N words (*count = N).
 * tfhe_hip_lut_bootstrap: nin in 1..3, in[nin] sample pointers, coef[nin].  Recorded in deferred mode like every gate
 * (SSA-renamed, levelled, dead results eliminated, batched across keys with "batch_keys"), complete on return in immediate
 * mode.  "reuse_gates" shares two pending LUT bootstraps only if LUT, operands (in the order given), coefficients, c0 and
 * key are all equal.  "fold_constants" NEVER folds a LUT bootstrap: a trivial operand is bootstrapped like any other.
 * Errors (tfhe_hip_last_error(), call without effect): a null or deleted LUT, a LUT of another N than the key's, nin outside
 * 1..3, and those of every boots* entry.
 * tfhe_hip_lut_bootstrap_batch: one LUT, result[i] from in[0][i] (, in[1][i], in[2][i]) for i < count -- in[k] is an array of
 * count samples; 0 / -1. ---- */
typedef struct TfheHipLut TfheHipLut;
TfheHipLut *tfhe_hip_new_lut(const TFheGateBootstrappingParameterSet *params, const Torus32 *v);
TfheHipLut *tfhe_hip_new_lut_constant(const TFheGateBootstrappingParameterSet *params, Torus32 mu);
TfheHipLut *tfhe_hip_new_lut_from_table(const TFheGateBootstrappingParameterSet *params, const Torus32 *values, int32_t slots);
void tfhe_hip_delete_lut(TfheHipLut *lut);
const Torus32 *tfhe_hip_lut_words(const TfheHipLut *lut, int32_t *count);
void tfhe_hip_lut_bootstrap(const TfheHipLut *lut, LweSample *result, int32_t nin, const LweSample *const *in,
                            const int32_t *coef, Torus32 c0, const TFheGateBootstrappingCloudKeySet *bk);
int tfhe_hip_lut_bootstrap_batch(const TfheHipLut *lut, LweSample *result, int32_t nin, const LweSample *const *in,
                                 const int32_t *coef, Torus32 c0, int32_t count, const TFheGateBootstrappingCloudKeySet *bk);

/* ---- several extractions from one rotation (multi-output LUT bootstrap): NOT PART OF UPSTREAM TFHE'S GATE API.  After
 * the n CMUX steps the accumulator ACC = (A, B) holds X^-p v for the encrypted phase p; coefficient 0, which every entry
 * above extracts, is one of N.  Coefficient e decrypts to the negacyclic table v read at p + e, and a small-integer
 * combination of a few coefficients is again one LWE sample under the same key -- so one rotation can feed several key
 * switches, each a different function of the same input (the multi-value bootstrap of Carpov, Izabachene and Mollimard).
 * Defined by integers:
 *     Extract_e(ACC), 0 <= e < N, is the sample with  b = B[e],  a_i = A[e - i] for i <= e,  a_i = -A[N + e - i] for i > e
 *     (the negacyclic extension of A read at (e - i) mod 2N; Extract_0 is the extract of every entry above)
 *     u_m = (0, out_c0[m]) + sum_t weight[m][t] * Extract_{index[m][t]}(ACC)        (wrapping mod 2^32 on all N+1 words)
 *     result[m] = the key switch of u_m, as for every extracted sample.
 * Prelude, modulus switch, ACC and the CMUX steps are those of tfhe_hip_lut_bootstrap.
 * Limits: nout in 1..4 outputs; 1..8 taps per output; 0 <= index < N; weight non-zero with |weight| <= 8; the taps of one
 * output have distinct indices.  One output with the one tap (0, +1) and out_c0 = 0 gives tfhe_hip_lut_bootstrap's words.
 * Noise (COMPUTED, not measured -- see profiles/lut_multi.txt for what was): the taps multiply the accumulator's noise by
 * their weights, so to first order an output's variance is sum_t weight^2 times the rotation variance of a gate, plus the
 * key-switch term, which does not grow.  The caller chooses tables whose weights its margins can bear.
 * tfhe_hip_new_lut_multi: everything is copied, the LUT's words included (the object holds its own entry in the engine's
 * table, so the LUT may be deleted afterwards); taps of all outputs are concatenated in output order (tap_index,
 * tap_weight: sum ntaps words); out_c0 null = zeros.  Like a LUT it is made, read and deleted without a GPU, reaches the
 * device at its first bootstrap, and deleting it runs the recording first if a recorded bootstrap names it.
 * tfhe_hip_new_lut_multi_from_tables: the usable form.  For an input phase in sector s of the half torus (`slots` sectors,
 * slots >= 2 divides N) output m has phase step * levels[m * slots + s].  Construction: the constant polynomial step/2
 * (step must be even); taps at j N/slots, j = 1..slots-1, with weight levels[m][slots-1-j] - levels[m][slots-j], zero
 * weights dropped; out_c0[m] = (step/2)(levels[m][0] + levels[m][slots-1]).  Why: for p in sector s coefficient j N/slots
 * decrypts to +step/2 when j <= slots-1-s and to -step/2 above, the weights up to J telescope to levels[slots-1-J] -
 * levels[slots-1], and the two partial sums give step levels[s] - (step/2)(levels[0] + levels[slots-1]).  Refused: a
 * weight beyond the limits, an output that would need no tap (equal levels everywhere), more than 8 taps.
 * tfhe_hip_lut_multi_nout / _output (taps and constant of output m into caller arrays of 8; returns the tap count) /
 * _words (the N words of the test polynomial): read-only accessors; -1 / NULL and the error channel on bad arguments.
 * tfhe_hip_lut_bootstrap_multi: result[nout] sample pointers; a NULL result[m] means "not wanted": that output is neither
 * extracted nor key-switched.  Recorded like every gate: ONE operation of one level whose wanted results are each
 * SSA-renamed and become available together; dead results are eliminated per output (the operation goes when all are
 * dead); "reuse_gates" shares two pending ones only if spec, LUT (the same object), operands, coefficients, c0 and key are
 * all equal, output by output, and an output the earlier one lacked is ADDED to it (the earlier operation is widened);
 * never constant-folded; batched across keys like a LUT bootstrap.
 * Errors (tfhe_hip_last_error(), call without effect): those of tfhe_hip_lut_bootstrap, a null or deleted object, two
 * results that are the same sample, every result null.
 * tfhe_hip_lut_bootstrap_multi_batch: result[m] (or NULL) is an array of count samples, in[k] likewise; 0 / -1. ---- */
typedef struct TfheHipLutMulti TfheHipLutMulti;
TfheHipLutMulti *tfhe_hip_new_lut_multi(const TfheHipLut *lut, int32_t nout, const int32_t *ntaps, const int32_t *tap_index,
                                        const int32_t *tap_weight, const Torus32 *out_c0);
TfheHipLutMulti *tfhe_hip_new_lut_multi_from_tables(const TFheGateBootstrappingParameterSet *params, Torus32 step, int32_t slots,
                                                    int32_t nout, const int32_t *levels /*[nout][slots]*/);
void tfhe_hip_delete_lut_multi(TfheHipLutMulti *mo);
int32_t tfhe_hip_lut_multi_nout(const TfheHipLutMulti *mo);
int32_t tfhe_hip_lut_multi_output(const TfheHipLutMulti *mo, int32_t m, int32_t *tap_index, int32_t *tap_weight, Torus32 *out_c0);
const Torus32 *tfhe_hip_lut_multi_words(const TfheHipLutMulti *mo, int32_t *count);
void tfhe_hip_lut_bootstrap_multi(const TfheHipLutMulti *mo, LweSample *const *result /*[nout]*/, int32_t nin,
                                  const LweSample *const *in, const int32_t *coef, Torus32 c0,
                                  const TFheGateBootstrappingCloudKeySet *bk);
int tfhe_hip_lut_bootstrap_multi_batch(const TfheHipLutMulti *mo, LweSample *const *result /*[nout]*/, int32_t nin,
                                       const LweSample *const *in, const int32_t *coef, Torus32 c0, int32_t count,
                                       const TFheGateBootstrappingCloudKeySet *bk);

/* ---- linear combinations of samples: NOT PART OF UPSTREAM TFHE'S GATE API (upstream has them below it: lweAddTo,
 * lweAddMulTo).  The free operations every programmable bootstrap is paired with: sums of more than the three samples a
 * bootstrap's prelude holds (the parity of five bits is ONE bootstrap of 1/4 + 2 * sum), weighted sums of bootstrapped
 * results as samples of their own (recombining a decomposition, a partial sum to export).  Defined by integers:
 *     result = (0, c0) + sum_{i < nin} coef[i] * in[i]           (wrapping mod 2^32 on all n+1 words)
 * nin in 1..TFHE_HIP_LINEAR_MAX_IN; any int32_t coefficient (0, -1, INT32_MIN included); the same sample may appear more
 * than once; result may be one of the operands (SSA renaming, as for every gate).  No bootstrap, no key switch, no noise
 * reset: the noise variance of the result is sum coef[i]^2 times the operands'.  bk only names the parameter set and the
 * slot pool, as it does for bootsNOT; with "batch_keys" the operands may be results under different keys of one set (the
 * words are defined whatever they mean).
 * Recorded in deferred mode like bootsNOT: it rides on the highest level of its operands (level 0: all materialised) and
 * runs after that level's key switches; a linear combination that reads another one of the same level runs one launch
 * later (its rank), so trees of them -- 128 terms as eight 16-term sums and a sum of those -- stay one recording.  An
 * operand that a pending bootsNOT writes is read as the NOT's operand with the coefficient negated, and bootsNOT of a
 * pending linear result is recorded as that result times -1: the same words.  Dead results are eliminated; "reuse_gates"
 * never shares one and "fold_constants" never folds one (nor treats its result as a constant).  Complete on return, host
 * mirror refreshed, in immediate mode.
 * Errors (tfhe_hip_last_error(), call without effect): nin outside 1..16, a null pointer, and those of every boots* entry
 * (a foreign sample, a sample of another LWE dimension, the slot pool exhausted).
 * tfhe_hip_linear_batch: result[i] from in[0][i], ..., in[nin-1][i] for i < count -- in[k] is an array of count samples;
 * 0 / -1.
 * tfhe_hip_sym_encrypt_torus: bootsSymEncrypt's path with the message mu in place of +-2^29 -- the same noise deviation,
 * the same two ChaCha20 streams (or the seeded generator after tfhe_hip_set_encrypt_seed, in the same draw order: mu =
 * +-2^29 gives bootsSymEncrypt's words for the same seed).
 * tfhe_hip_sym_phase: b - <a, s> mod 2^32 of the sample, after running pending operations exactly where bootsSymDecrypt
 * does (which returns phase > 0); 0 and the error channel on a null key or a foreign sample. ---- */
#define TFHE_HIP_LINEAR_MAX_IN 16
void tfhe_hip_linear(LweSample *result, int32_t nin, const LweSample *const *in, const int32_t *coef, Torus32 c0,
                     const TFheGateBootstrappingCloudKeySet *bk);
int tfhe_hip_linear_batch(LweSample *result, int32_t nin, const LweSample *const *in, const int32_t *coef, Torus32 c0,
                          int32_t count, const TFheGateBootstrappingCloudKeySet *bk);
void tfhe_hip_sym_encrypt_torus(LweSample *result, Torus32 mu, const TFheGateBootstrappingSecretKeySet *key);
Torus32 tfhe_hip_sym_phase(const LweSample *sample, const TFheGateBootstrappingSecretKeySet *key);

/* ---- tuning (twelve names that results never depend on, and the opt-in "fold_constants") ----
 * "br_variant": which form of the blind-rotate kernel runs wide launches (env TFHE_HIP_BR_VARIANT): -1 (default) =
 * the fastest measured for the ring size (N = 1024: 4 waves per rotation; N = 2048: split), 0 = 4 waves (N = 1024),
 * 2 = split (8 waves, every transform as two half-size ones), 4 = 2 waves (N = 1024; the form with the widest admissible
 * gadget range).  A form whose bounds do not admit the key's gadget is replaced by one that does (br_forms.hpp).
 * "br8_max_rotations": launches of at most min(this, CU count) rotations use the 8-wave form at N = 1024 (default 2^30,
 * env TFHE_HIP_BR8_MAX; 0 = never).
 * "br_tail8": 1 (default, env TFHE_HIP_BR_TAIL8) = the last, at most half-filled round of a wide 4-wave launch runs on the
 * 8-wave form as a second launch.
 * "br_digit_table": 1 (default, env TFHE_HIP_BR_TABLE) = products of gadget digits with the first twiddles come from
 * LDS tables where the digits are at most 7 bits wide (split form: 2 = the stage-0 table only); 0 = multiplies.
 * "ks_tile": 16 (default), 24 or 32 (index form only; elsewhere read as 16) = launches of at least 2*tile key switches use
 * a tiled kernel (a workgroup streams the KSK rows of one range once for `tile` gates); 0 = always one workgroup per
 * (gate, range); env TFHE_HIP_KS_TILE.
 * "ks_index": 1 (default, env TFHE_HIP_KS_INDEX) = the tiled kernel keeps a thread's 16-byte column of the three rows of a
 * digit position in pinned registers addressed through the VGPR index mode by the wave-uniform digit (56 ms of key switch
 * per match); 0 = the rows in thread-private LDS strips (105 ms; plain HIP source).
 * "reuse_gates": 1 (default) = in deferred mode a gate recorded again with the same operand
 * samples before the flush shares the pending gate's result instead of being evaluated again
 * (same function of the same ciphertexts, so the same words); 0 = evaluate every call.
 * "eliminate_dead": 1 (default) = at a flush, a recorded gate whose result no sample handle holds any more and no
 * live gate reads is not evaluated (the reference's adders compute carries they then drop: 3 % of a match); nothing
 * observable changes; 0 = evaluate every recorded gate.
 * "balance_levels": 1 (default) = slack-aware level filling at flush, 0 = plain ASAP
 * levels.
 * "level_slack" (env TFHE_HIP_LEVEL_SLACK): 1 (default) = behind that filling, gates with slack move off the cost steps
 * of a MEASURED table of level costs, where the library holds one for the parameter set, the CU count and the launch
 * tunings (profiles/level_cost_*.json); 0 = never.
 * "fold_constants": 0 (default) / 1 (env TFHE_HIP_FOLD_CONSTANTS) = OPT-IN constant folding at record time: a gate one of
 * whose operands is a trivial sample (bootsCONSTANT, a fresh sample, a copy of either: a PUBLIC constant) is not
 * bootstrapped -- its result is the constant, the other operand or its negation; a MUX with a constant data operand becomes
 * a two-input gate.  The reference's match circuit loses 62 % of its bootstraps that way.  Decrypted results are the same;
 * the ciphertext WORDS are not TFHE's (which bootstraps every gate), which is why it is off unless asked for -- the only
 * tuning results depend on.  The oracle folds by the same rule (orc_boots_set_fold): folded circuits have digests too.
 * "batch_keys": 0 (default) / 1 (env TFHE_HIP_BATCH_KEYS) = OPT-IN multi-key flushes: gates recorded under different cloud
 * keys of the SAME parameter set stay recorded together and run as one level sequence (one flush), each bootstrap and key
 * switch under its own gate's key -- a server's K clients fill the levels of one flush instead of running as K narrow
 * flushes.  0: a gate under another key than the pending gates' flushes them first.  A key of another parameter set
 * flushes either way; the same set = equal n, N, k, l, Bgbit, ks_t and ks_basebit, by value (two parameter-set objects
 * with equal numbers are one set; the noise deviations do not matter).  The words are the same as with 0; every key of
 * such a flush stays alive until it has run (deleting a keyset runs the whole recording first).
 * "sync_deadline_ms": see "bounded host waits" above.
 * "ks_max_splits": 1 .. 64, default 48 (env TFHE_HIP_KS_MAX_SPLITS): the most coefficient ranges a key switch is cut into; 1 =
 * never cut, every result goes straight to its slot (peba1_amd/csrc/launch_plan.hpp).
 * (Environment only: TFHE_HIP_KS_BLOCKS / TFHE_HIP_KS_SPLIT_TIES, the rest of how key switches are cut into ranges.)
 * Returns 0, or -1 for an unknown name. */
int tfhe_hip_set_tuning(const char *name, int64_t value);

/* ---- statistics ---- */
typedef struct TfheHipStats {
    uint64_t blind_rotates;     /* K2 instances */
    uint64_t keyswitches;       /* K3 instances */
    uint64_t linear_ops;        /* NOTs and linear combinations (tfhe_hip_linear) run */
    uint64_t levels;            /* batched levels executed */
    uint64_t flushes;
    uint64_t br_launches;       /* blind-rotate kernel launches */
    double   ms_blind_rotate;   /* device time, HIP events on the engine stream */
    double   ms_keyswitch;
    double   ms_flush_wall;     /* host wall time inside flush */
    double   ms_blind_rotate_busy; /* time during which at least one blind-rotate launch was running
                                      (== ms_blind_rotate: a flush is one level sequence on one stream) */
    uint64_t reused_gates;      /* recorded gates served by an identical pending gate ("reuse_gates") */
    /* of the blind-rotate totals above, the part run by the 8-wave form (launches of at most one
     * workgroup per CU); the rest is the 4-wave kernel */
    uint64_t br8_launches;
    uint64_t br8_rotations;
    double   ms_blind_rotate8;
    /* with kernel timing on: shader cycles (s_memtime) and 100 MHz reference ticks (s_memrealtime) that every 61st workgroup
     * of every blind-rotate launch of the flushes lived for; 0.1 * cycles / ticks = the shader clock in GHz the
     * timed launches ran at (a cold chip runs them at ~2.0 GHz, a warm one at ~2.37) */
    uint64_t clk_shader_cycles;
    uint64_t clk_ref_ticks;
    /* recorded gates (and NOTs) dropped at a flush because nothing could ever observe their result: no sample
     * handle held it and no live gate read it ("eliminate_dead") */
    uint64_t dead_gates;
    /* gates answered WITHOUT a bootstrap because an operand was a public constant (a trivial sample): "fold_constants",
     * opt-in; a MUX turned into a two-input gate counts once */
    uint64_t folded_gates;
    /* blind-rotate kernel launches by the form that really ran (after the fallback of br_forms.hpp) and by the digit-table
     * mode it ran with, counted where the kernel is launched -- the raw test path (tfhe_hip_kernel_bootstrap_woks)
     * included, which the totals above leave out.  A level split into a 4-wave launch and an 8-wave tail counts one of each. */
    uint64_t br_wide4_launches;
    uint64_t br_split_launches;
    uint64_t br_wave8_launches;
    uint64_t br_wave2_launches;
    uint64_t br_tables0_launches;
    uint64_t br_tables1_launches;
    uint64_t br_tables2_launches;
    /* of blind_rotates, those that started from a caller-supplied test polynomial (tfhe_hip_lut_bootstrap; the raw
     * entry tfhe_hip_kernel_lut_bootstrap_woks included) */
    uint64_t lut_rotations;
    /* of blind_rotates, those that left through an extract spec (tfhe_hip_lut_bootstrap_multi; the raw entry
     * tfhe_hip_kernel_lut_bootstrap_multi_woks included), and the outputs they wrote.  `keyswitches` counts one per
     * output written by a flush */
    uint64_t multi_rotations;
    uint64_t multi_outputs;
    /* of linear_ops, the linear combinations (tfhe_hip_linear, and a bootsNOT recorded as one), and the kernel launches they
     * took: one per (level, rank) present in a flush */
    uint64_t lincomb_ops;
    uint64_t lincomb_launches;
    /* key-switch kernel launches by the form that ran, counted where the launch is issued, from its plan
     * (peba1_amd/csrc/launch_plan.hpp plan_ks) -- the raw test path (tfhe_hip_kernel_keyswitch) included: the per-gate kernel
     * (narrow launches, every key-switch decomposition other than t = 8, base 4, and row widths the tiled kernels are not
     * built for), the LDS-strip form, the index form.  A tiled launch counts one per chunk of 8,192 gates; the reduce
     * launches behind split forms are not counted */
    uint64_t ks_pergate_launches;
    uint64_t ks_strip_launches;
    uint64_t ks_index_launches;
    /* ring-encrypted inputs (tfhe_hip_unpack_samples*): the samples written into slots -- each also counts one in
     * `keyswitches` -- and the extract kernel launches they took, one per chunk of 8,192 (the raw entry
     * tfhe_hip_kernel_ring_extract counts its launches too) */
    uint64_t unpacked_samples;
    uint64_t unpack_launches;
} TfheHipStats;
void tfhe_hip_get_stats(TfheHipStats *out);
void tfhe_hip_reset_stats(void);
/* seed-compressed cloud keys: the keysets whose masks were made on the device (tfhe_hip_expand_cloud_key, at first use)
 * and the expand kernel launches that took, two per key (the raw entry tfhe_hip_kernel_expand_masks counts its one launch
 * too); a host-expanded keyset counts nothing.  A struct and an entry of their own: TfheHipStats is allocated by the
 * caller and filled whole, so it cannot grow under a caller built against this header's earlier form.
 * tfhe_hip_reset_stats() clears these too. */
typedef struct TfheHipExpandStats {
    uint64_t expanded_keys;
    uint64_t expand_launches;
} TfheHipExpandStats;
void tfhe_hip_get_expand_stats(TfheHipExpandStats *out);
/* the matrix key switch (tunings "ks_matrix", "ks_matrix_min"): the launches of a flush's wide levels that ran as an int8
 * matrix product on the matrix cores, one per (level, key) (the raw entry tfhe_hip_kernel_keyswitch_matrix counts its one
 * launch too).  Such a launch counts in none of ks_pergate / ks_strip / ks_index_launches.  A struct and an entry of their
 * own, for the same reason as above; tfhe_hip_reset_stats() clears these too. */
typedef struct TfheHipKsMatrixStats {
    uint64_t ks_matrix_launches;
} TfheHipKsMatrixStats;
void tfhe_hip_get_ks_matrix_stats(TfheHipKsMatrixStats *out);
/* seed-compressed packing keys and ring samples, a struct of their own for the same reason: the packing keys whose masks
 * were made on the device (tfhe_hip_expand_packing_key, at the first pack) and the expand kernel launches that took, one per
 * key -- a host-expanded or plain key counts nothing; the samples opened by the seeded unpack entries and their extract
 * launches (tfhe_hip_kernel_ring_extract_seeded counts its launches too).  A seeded unpack also counts in unpacked_samples,
 * unpack_launches and keyswitches of TfheHipStats, as a plain one does.  tfhe_hip_reset_stats() clears these too. */
typedef struct TfheHipSeededStats {
    uint64_t expanded_packing_keys;
    uint64_t packing_expand_launches;
    uint64_t seeded_unpacked_samples;
    uint64_t seeded_unpack_launches;
} TfheHipSeededStats;
void tfhe_hip_get_seeded_stats(TfheHipSeededStats *out);
/* seed-compressed LWE sample arrays, a struct of their own for the same reason: the samples written into slots by the
 * seeded import entries and the expand kernel launches they took, one per chunk of 8,192 (the raw entry
 * tfhe_hip_kernel_lwe_expand counts its launches too, and no samples).  A seeded import switches no key and runs no flush:
 * nothing in TfheHipStats moves.  tfhe_hip_reset_stats() clears these too. */
typedef struct TfheHipSeededLweStats {
    uint64_t seeded_imported_samples;
    uint64_t seeded_import_launches;
} TfheHipSeededLweStats;
void tfhe_hip_get_seeded_lwe_stats(TfheHipSeededLweStats *out);
/* when on, every kernel launch is bracketed by HIP events, read back after the flush */
void tfhe_hip_set_kernel_timing(int on);
/* distinct cloud keys the last executed flush ran under (1 unless "batch_keys" is on; 0 before the first flush) */
int tfhe_hip_last_flush_keys(void);
/* "batch_keys" := on (0 / 1); returns the previous setting (so that a caller can restore it) */
int tfhe_hip_set_batch_keys(int on);

/* ---- host-logic test entry: does blind-rotate kernel form `form` (0 = 4 waves, 1 = split, 2 = 8 waves, 3 = 2 waves)
 * keep its magnitude bounds for gadget (l, Bgbit) at ring size N with digit-table mode
 * `tables` (0, 1, 2 as "br_digit_table")?  A key is refused at upload when no form does; a launch falls back to an
 * admissible form (peba1_amd/csrc/br_forms.hpp).  Returns 1 or 0. ---- */
int tfhe_hip_test_form_admissible(int form, int32_t N, int32_t l, int32_t Bgbit, int tables);

/* ---- host-logic test entry: where the engine's pinned staging area (peba1_amd/csrc/host_stage.hpp) puts a reservation of
 * `bytes`, given its write position, its capacity and whether an upload from it is outstanding, without touching the
 * device.  out4 = {offset, 1 = the area's event is waited for first, capacity afterwards, write position afterwards}.
 * Returns 0, -1 on bad arguments. ---- */
int tfhe_hip_test_stage_place(int64_t pos, int64_t capacity, int32_t outstanding, int64_t bytes, int64_t *out4);

/* ---- test entry: device allocations of key images, the ciphertext slot pool and the per-flush scratch that would bring their total
 * above `bytes` fail as if the card were full (0 = no cap).  Running out of device memory there is RECOVERABLE: the call
 * that needed the memory has no effect (recorded gates stay recorded, tfhe_hip_flush returns -1), tfhe_hip_last_error()
 * says what could not be allocated, and the caller may free ciphertext arrays and carry on. ---- */
void tfhe_hip_test_set_alloc_cap(int64_t bytes);
/* ---- test entry (read-only): the bytes those allocations hold now, the figure the cap is compared with ---- */
int64_t tfhe_hip_test_alloc_held(void);

/* ---- host-logic test entry: levelise a DAG given as count x {kind, dst, a, b, c} slot
 * records (kind: gate code 0..9, 16 = MUX, 17 = NOT, 32 + 8 * TfheHipGate3 + negate_mask = a three-input gate; absent
 * operands -1) without touching the device; writes the level of each op, returns the depth (-1: unknown kind) ---- */
int tfhe_hip_test_schedule(const int32_t *ops5, int32_t count, int32_t unit, int32_t balance, int32_t *levels_out);
/* ---- host-logic test entry: the same levelisation, then the level plan a flush of these ops under `nkeys` cloud keys
 * hands to the engine (op i bootstraps under key op_keys[i], 0 <= op_keys[i] < nkeys), without touching the device.
 * The caller provides room for the largest plan `count` ops can give: levels_out[count]; rot_off, ks_off
 * [count + 1]; rot_koff, ks_koff [count * nkeys + 1]; rot_key [2 count]; rots6 [6 * 2 count] ({slot_a, slot_b,
 * sa, sb, c0, u_index} per rotation); kss4 [4 count] ({u0, u1, add_b, dst_slot} per key switch; u0 / u1 index the
 * level's extracted samples).  sizes6 = {levels, rotations, key switches, entries of rot_koff, of ks_koff, of rot_key}
 * (the last three are 0 with one key); rot_off and ks_off hold levels + 1 entries.  Returns the number of levels,
 * -1 on bad arguments. ---- */
int tfhe_hip_test_level_plan(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                             int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                             int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots6, int32_t *kss4);
/* The same with eight words per rotation: {slot_a, slot_b, sa, sb, c0, u_index, slot_c, sc}; slot_c = -1, sc = 0 where the
 * rotation has no third operand (rots8 [8 * 2 count]).  tfhe_hip_test_level_plan gives the first six of these. */
int tfhe_hip_test_level_plan3(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                              int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                              int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots8, int32_t *kss4);
/* The same for recordings that hold LUT bootstraps, with the recorder's sharing rule: ops10 = count x {kind, dst, a, b, c, lut,
 * sa, sb, sc, c0} (kind 64 = a LUT bootstrap; the last five words are read for that kind only).  reuse != 0: a record equal
 * to an earlier one in kind, operands, key and -- for a LUT bootstrap -- LUT, coefficients and c0 shares its result exactly
 * as "reuse_gates" does: shared_with[i] = that record (-1: evaluated), it takes no rotation, and later records that read its
 * dst read the earlier one's.  rots9 [9 * 2 count]: the eight words above and the LUT index (-1: the constant test vector). */
int tfhe_hip_test_level_plan_lut(const int32_t *ops10, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, int32_t *levels_out, int32_t *shared_with, int32_t *sizes6,
                                 int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key,
                                 int32_t *rots9, int32_t *kss4);
/* The same for recordings that hold multi-output bootstraps, with the recorder's sharing and elimination rules: ops16 =
 * count x {kind, dst, a, b, c, lut, sa, sb, sc, c0, spec, nout, d0, d1, d2, d3} (kind 65 = a multi-output bootstrap: dst is
 * not read, d_m = the destination of output m or -1 when it is not wanted; other kinds as in ops10, the last six words not
 * read).  reuse != 0: an equal earlier multi-output record serves a later one output by output and gains the outputs it
 * lacked (shared_with as above).  dead_slots[ndead]: destinations no handle holds at the flush -- one that no surviving
 * record reads is eliminated, per output for kind 65; a record eliminated altogether gets level -1.  rots10: the nine
 * words above and the extract spec word (-1, or spec | wanted outputs << 24); a multi-output rotation's output m is sample
 * u_index + m of its level, and kss4 holds one {u, -1, 0, destination} per wanted output. */
int tfhe_hip_test_level_plan_multi(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                   int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                   int32_t *levels_out, int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                                   int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4);
/* The same for recordings that hold linear combinations: a record of kind 66 is {66, dst, -1, -1, -1, first term, nin, 0, 0,
 * c0, ...} and its nin terms are lin_terms2[2 * (first term + t)] = {operand id, coefficient} (nterms pairs in all); a
 * record of kind 17 (NOT) whose operand a pending linear combination writes becomes one, as in the recorder.  ranks_out[i]:
 * the rank of record i (0 for all but linear combinations; -1: eliminated).  lin_sizes2 = {launches, descriptors};
 * lin_level_off [levels + 2]: the launches of level L (0 = inputs) are [L], [L + 1]); lin_launch_off [launches + 1] and
 * lin_launch_rank [launches]: the descriptor range and the rank of every launch; lins35 [35 * descriptors]: {dst, nin, c0,
 * slot[16], coef[16]} each, operands as the recorder rewrote them.  Room for `count` launches and descriptors. */
int tfhe_hip_test_level_plan_lin(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                 const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                 int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                 int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                 int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35);
/* The same, and the NOT launches as well -- the whole plan, so that a test can execute it: not_off [levels + 2]: the NOTs
 * that ride on level L (0 = inputs) are descriptors [not_off[L], not_off[L + 1]); nots2 [2 * count]: {source slot,
 * destination slot} each.  A level runs its rotations, its key switches, its NOT launch and then its linear launches. */
int tfhe_hip_test_level_plan_full(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                  int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                  const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                  int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                  int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                  int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35,
                                  int32_t *not_off, int32_t *nots2);
/* ---- host-logic test entries: the launch rules of peba1_amd/csrc/launch_plan.hpp, without touching the device.
 * tfhe_hip_test_br_plan: the blind-rotate launches of a level of `count` rotations of gadget (l, Bgbit) at ring size N on
 * a card of `cu_count` CUs under tunings4 = {br_variant, br8_max_rotations, br_tail8, br_digit_table}; flags bit 0 = the
 * workgroup-time probe is on, bit 1 = the raw accumulators are read back.  out3 = {form (as tfhe_hip_test_form_admissible;
 * -1: no form admits the gadget), digit-table mode, tail}: tail > 0 = the first count - tail rotations on the 4-wave form,
 * the last `tail` on the 8-wave form as a second launch.
 * tfhe_hip_test_ks_plan: the key-switch launches of `count` gates of a set with LWE dimension n, ring (N, k) and key-switch
 * digits (ks_t, ks_basebit) under tunings5 = {ks_target_blocks, ks_max_splits, ks_split_ties, ks_tile, ks_index}.
 * out6 = {tiled kernel 1 / 0, gates per tile (0: per-gate kernel), gates per launch (all launches but the last), coefficient
 * ranges of the first launch, of the last launch, bytes of partial sums the whole sequence needs}.
 * tfhe_hip_test_ks_plan_form: the same six words and, seventh, the kernel form: 0 = per gate, 1 = LDS strips, 2 = index
 * (out7).  What Engine::launch_ks runs and counts (ks_*_launches) is this plan.
 * All return 0, -1 on bad arguments. ---- */
/* ---- the cost-driven levelling (tuning "level_slack", peba1_amd/csrc/scheduler.cpp relevel_by_cost), without touching
 * the device.  tfhe_hip_test_level_slack: levelise the DAG ops5 (records as tfhe_hip_test_schedule's, balance = 1) and,
 * with level_slack != 0, run the pass under the cost table (cost_widths ascending from >= 1, cost_us; linear between
 * entries; beyond the last one the last slope goes on (period = 0) or the table's last `period` rotations repeat, as
 * for a compiled-in table with period = 2 CUs; ncost = 0: no table).  levels_out[count]: the level of every op; widths_out[depth + 1]:
 * rotations per level; cost_out2 = {sum of the table's cost over the levels, the same sum without the pass}.  Returns the
 * depth.  level_slack = 0 gives tfhe_hip_test_schedule's levels.
 * tfhe_hip_test_level_cost: launch_plan.hpp level_cost_us under the default tunings: the compiled-in measured table's
 * microseconds for a level of `width` rotations of this parameter set on a card of cu_count CUs, -1 = no table.
 * tfhe_hip_test_set_level_cost: flushes use this table for every parameter set in place of the compiled-in ones
 * (ncost = 0: those again).  tfhe_hip_last_level_slack: out4 = {sum before the pass, after it, gates moved, pool slots in use
 * when the flush began -- its peak: slots are taken at record time} of the last flush (the first three 0: the pass did not run).  Return 0 (the first: the depth), -1 on bad arguments. ---- */
int tfhe_hip_test_level_slack(const int32_t *ops5, int32_t count, int32_t unit, int32_t level_slack, const int32_t *cost_widths,
                              const double *cost_us, int32_t ncost, int32_t period, int32_t *levels_out, int32_t *widths_out,
                              double *cost_out2);
int tfhe_hip_test_level_cost(int32_t n, int32_t N, int32_t k, int32_t l, int32_t Bgbit, int32_t ks_t, int32_t ks_basebit,
                             int32_t cu_count, int32_t width, double *us_out);
int tfhe_hip_test_set_level_cost(const int32_t *cost_widths, const double *cost_us, int32_t ncost);
int tfhe_hip_last_level_slack(double *out4);
int tfhe_hip_test_br_plan(int32_t N, int32_t l, int32_t Bgbit, const int32_t *tunings4, int32_t cu_count, int32_t count,
                          int32_t flags, int32_t *out3);
int tfhe_hip_test_ks_plan(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                          int32_t cu_count, int32_t count, int64_t *out6);
int tfhe_hip_test_ks_plan_form(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                               int32_t cu_count, int32_t count, int64_t *out7);
/* tfhe_hip_test_ks_plan_form2: the plan of a FLUSH's key-switch launch.  tunings7: the five words above, then the tunings
 * ks_matrix and ks_matrix_min; has_image: the key holds the byte-plane image of the matrix form.  Form 3 = the matrix form
 * (tile 64, one launch of `count` gates, one range, no partial sums) at and above ks_matrix_min where the tiled forms would
 * have run; otherwise what tfhe_hip_test_ks_plan_form returns.  The two entries above have no word for these tunings and
 * return the plan with the matrix form off: that of every caller but a flush. */
int tfhe_hip_test_ks_plan_form2(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings7,
                                int32_t has_image, int32_t cu_count, int32_t count, int64_t *out7);
/* the four signed bytes s_0 .. s_3 in [-128, 127] of each word w, sum_p s_p 2^(8p) = w (mod 2^32): planes4[count][4] */
int tfhe_hip_test_ks_byte_planes(const uint32_t *words, int32_t count, int8_t *planes4);
/* Diagnostic (tools/wg_times.py): a 4-wave blind-rotate launch of `width` random gates (the second of two back to back);
 * times4[4i .. 4i+3] = s_memtime (shader cycles; the start stamp carries the XCC / CU id in its top 16
 * bits) at the start and end of workgroup i, then s_memrealtime (constant 100 MHz) at its start and
 * end; *launch_ms = the launch's duration between two stream events. */
int tfhe_hip_test_wg_times(const TFheGateBootstrappingCloudKeySet *bk, int32_t width, uint64_t *times4, double *launch_ms);

/* ---- packing key switch: up to N LWE samples under the LWE key -> ONE TLWE sample under the ring key ----
 * A server returns M result bits as M samples of n + 1 words; packed, up to N of them travel as (k+1) N words and the
 * client runs one ring decryption: coefficient j of the packed sample's phase is the phase of sample j (plus noise).
 *
 * A packing key belongs to a keyset and a decomposition (pk_t, pk_basebit); 0, 0 = the set's own (ks_t, ks_basebit).
 * For i < n and p < pk_t, row[i][p] is a TLWE sample under the keyset's ring key -- uniform masks, noise of the set's
 * bk_stdev (NOT ks_stdev: see the variance below), message the constant polynomial lwe_key[i] << (32 - (p+1) pk_basebit)
 * -- laid out [n][t][k+1][N], the k mask polynomials of a row first, then its body; phase = body - sum_u mask_u * S_u.
 * For samples c_0 .. c_{count-1}, 1 <= count <= N, c_j = (a_j, b_j), with t = pk_t, basebit = pk_basebit, base = 2^basebit:
 *     prec       = 2^(32 - (1 + basebit t))                 (0 when basebit t = 32: nothing is rounded away)
 *     d[j][i][p] = ((a_j[i] + prec) >> (32 - (p+1) basebit)) & (base - 1)        -- the digits of the existing key switch
 *     D[i][p](X) = sum_{j < count} d[j][i][p] X^j
 *     packed     = (0, ..., 0, sum_j b_j X^j) - sum_{i, p} D[i][p](X) * row[i][p]
 * in Z[X]/(X^N + 1), wrapping mod 2^32 on all (k+1) N words.  Coefficient j of the phase B - sum_u A_u S_u is the phase
 * of c_j plus noise for j < count, noise only from `count` on.
 * Variance added to every coefficient, to first order -- COMPUTED from the definition, not measured (torus units):
 *     key term       n t count E[d^2] bk_stdev^2,   E[d^2] = (base - 1)(2 base - 1) / 6 for uniform digits
 *     rounding term  (n / 2) prec^2 / 3             (a uniform residue below prec in magnitude on each of the n/2 key bits
 *                                                    that are set, on average; prec as a fraction of the torus)
 * P128 (n = 630, t = 8, base = 4, bk_stdev = 2^-25), count = 1,024: 1.60e-8 + 6.1e-9, sigma = 1.5e-4 -- a gate output
 * stands 1/8 from the decision boundary.  With ks_stdev = 2^-15 in its place the key term alone would be 1.7e-2,
 * sigma = 0.13: about ONE sigma from the boundary, which is why the rows carry bk_stdev.
 *
 * Key generation.  tfhe_hip_new_packing_key draws the noise and the masks from two fresh ChaCha20 streams keyed by the
 * OS, as a new keyset does; tfhe_hip_new_packing_key_seeded from ONE seeded generator (xoshiro256** through splitmix64,
 * as the seeded keysets) started from `seed` for this key alone.  Neither touches the streams a keyset was or will be
 * drawn from: a seeded keyset's words are the same with or without packing keys made from it.  Draw order, both forms:
 * for i < n, for p < t: the k N mask words of row[i][p] (one `torus` draw each), then its N noise samples (one `gauss`
 * draw each).  NULL (and the error set) for a null keyset or a refused decomposition: basebit outside 1..4,
 * t basebit > 32, or t beyond what the kernel's accumulators take (t <= 18 at N = 1024, t <= 16 at N = 2048:
 * peba1_amd/csrc/pack.hpp derives that bound and the CRT bound beside it).  Host only: no GPU is needed to make a
 * key, read its words or decrypt a packed sample.
 * tfhe_hip_new_packing_key_from_words: the cloud side -- a server that received the raw rows builds its key from them
 * (the words are copied).  tfhe_hip_packing_key_words: a read-only view of the raw rows, *count = n t (k+1) N.
 * "Seed-compressed packing keys and ring samples" below: the same key travelling as a mask seed and its bodies. */
typedef struct TfheHipPackingKey TfheHipPackingKey;
TfheHipPackingKey *tfhe_hip_new_packing_key(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t, int32_t pk_basebit);
TfheHipPackingKey *tfhe_hip_new_packing_key_seeded(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t,
                                                   int32_t pk_basebit, uint64_t seed);
TfheHipPackingKey *tfhe_hip_new_packing_key_from_words(const TFheGateBootstrappingParameterSet *params, int32_t pk_t,
                                                       int32_t pk_basebit, const Torus32 *words);
void tfhe_hip_delete_packing_key(TfheHipPackingKey *key);
const Torus32 *tfhe_hip_packing_key_words(const TfheHipPackingKey *key, int64_t *count);
/* the decomposition the key was made with (0, 0 resolved); 0 / -1 */
int tfhe_hip_packing_key_decomposition(const TfheHipPackingKey *key, int32_t *pk_t, int32_t *pk_basebit);
/* Pack samples[0..count) (consecutive elements of one array) under cloud key `bk` of the key's parameter set into the
 * (k+1) N words of out_words.  An observation point like tfhe_hip_export_samples: the pending recorded operations run
 * first, then the pack is enqueued on tfhe_hip_stream(); the host form returns with the words in place.  The device
 * form writes device memory and is stream-ordered like tfhe_hip_export_samples_device_async: it returns with the pack
 * enqueued, and whatever the caller enqueues on that stream afterwards is ordered behind it (tfhe_hip_stream_sync()
 * waits for it).  The key's words and their NTT image (2 n t (k+1) N words: 83 MB at P128, t = 8) reach the device at
 * the first pack; device memory exhausted there is reported like every failure below.
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect: count outside 1..N, a null pointer, a
 * sample this library did not allocate, samples or a cloud key of another parameter set than the packing key's. */
int tfhe_hip_pack_samples(const TfheHipPackingKey *key, const LweSample *samples, int32_t count,
                          const TFheGateBootstrappingCloudKeySet *bk, Torus32 *out_words);
int tfhe_hip_pack_samples_device(const TfheHipPackingKey *key, const LweSample *samples, int32_t count,
                                 const TFheGateBootstrappingCloudKeySet *bk, void *device_words);
/* Decryption of a packed sample ((k+1) N words) on the host: the phases of all N coefficients; the bits (phase > 0) of
 * the first `count`, 1 <= count <= N.  0 / -1. */
int tfhe_hip_packed_phase(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *words, Torus32 *out_phases);
int tfhe_hip_packed_decrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *words, int32_t count,
                                 int32_t *out_bits);
/* host-logic test entry: the two magnitude bounds of the pack kernel (peba1_amd/csrc/pack.hpp) for a chunk of `rows` key rows
 * of ring size N (1024 or 2048) and digits of `basebit` bits (1..4): bit 0 set = the MAC bound refuses it, bit 1 set =
 * the CRT bound refuses it; -1 on bad arguments.  The kernel's chunk is one mask index: rows = t. */
int tfhe_hip_test_pack_bounds(int32_t N, int32_t rows, int32_t basebit);

/* ---- ring-encrypted inputs: ONE TLWE sample under the ring key -> up to N LWE samples under the LWE key ----
 * The way in, as the packing key switch is the way out: a client sends N input bits as one ring sample of (k+1) N words
 * (8 KB at N = 1,024) instead of N LWE samples of n + 1 words (2.5 MB at P128); the server opens it on the device with the
 * sample extract and the key switch every gate ends with.  No key material beyond the cloud key is needed.  k = 1.
 *
 * Ring encryption (host only, no GPU is needed).  out_words is one TLWE sample under the keyset's ring key, laid out as a
 * row of a packing key: the k mask polynomials first, then the body = sum_u mask_u * S_u + mu + e in Z[X]/(X^N + 1),
 * wrapping mod 2^32.  The masks are uniform; the noise e has the set's bk_stdev, the ring's own fresh-sample deviation
 * (the one the packing rows carry).  The _bits forms set mu[j] = +2^29 for a bit of 1 and -2^29 for a bit of 0 for
 * j < count and mu[j] = 0 from `count` on, 1 <= count <= N.  The default forms draw from two fresh ChaCha20 streams keyed
 * by the OS, as a packing key does; the seeded forms from ONE seeded generator (xoshiro256** through splitmix64) started
 * from `seed` for this sample alone.  Draw order, both forms: the k N mask words (one `torus` draw each), then the N
 * noise samples (one `gauss` draw each).  Neither form touches the streams a keyset or a packing key is drawn from.
 * tfhe_hip_packed_phase and tfhe_hip_packed_decrypt_bits above decrypt such a sample: it has the layout and the key of a
 * packed one.  Return 0, or -1 with tfhe_hip_last_error() set and out_words untouched: a null argument, count outside 1..N. */
int tfhe_hip_ring_encrypt(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words);
int tfhe_hip_ring_encrypt_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words,
                                 uint64_t seed);
int tfhe_hip_ring_encrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                               Torus32 *out_words);
int tfhe_hip_ring_encrypt_bits_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                      Torus32 *out_words, uint64_t seed);
/* The unpack.  ring_words holds nring samples of (k+1) N words; index[j] = r N + e names coefficient e of sample r,
 * 0 <= index[j] < nring N; index = NULL means 0, 1, ..., count - 1; an index may repeat and the list may come in any
 * order.  result[j] = KeySwitch(Extract_e(ring sample r)) under the cloud key's own (ks_t, ks_basebit) -- the key switch
 * of every extracted sample, the one a gate ends with -- and Extract_e as defined for the multi-output bootstrap above:
 *     b = B[e],   a_i = A[e - i] for i <= e,   a_i = -A[N + e - i] for i > e,   everything wrapping mod 2^32.
 * Coefficient e of the ring sample's phase is the phase of result[j], plus the key switch's noise.
 * Variance, to first order -- COMPUTED from the definition, not measured (torus units): the ring sample's own, bk_stdev^2
 * for a fresh one, plus the key-switch term of a gate output, N t ks_stdev^2 + (the rounding of the N / 2 key bits that are
 * set on average, (N / 2) prec^2 / 3 with prec = 2^-(1 + basebit t)); there is NO rotation term, nothing was bootstrapped.
 * P128 (N = 1,024, t = 8, ks_stdev = 2^-15, basebit t = 16): key term 7.6e-6, rounding term 9.9e-9, sigma = 2.8e-3.  An
 * operand of a two-input gate may err by 1/16 (its share of the gate's 1/8 margin): 22 sigma.
 *
 * Semantics, as tfhe_hip_import_samples: every result is renamed into a fresh slot; all arguments are checked before
 * anything changes.  A flush in flight is completed first (the key switch's partial-sum scratch belongs to it); recorded
 * operations that have not run stay recorded -- they cannot name the new slots.  The host form returns with the slots
 * written; the device form reads device memory and returns with the work enqueued on tfhe_hip_stream(), like
 * tfhe_hip_import_samples_device_async (the caller keeps device_ring_words until the stream has passed, e.g.
 * tfhe_hip_stream_sync()).  Host mirrors are stale until a decrypt, an export or tfhe_hip_sync_samples; in immediate mode
 * they are refreshed on return.  Work proceeds in chunks of at most 8,192 samples: the extract scratch stays below
 * 8,192 u_stride words whatever `count` is.
 * result: `count` consecutive samples of one array; the scattered form takes `count` sample pointers instead (samples of
 * several arrays, any order; a pointer given twice ends with its last value).
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect (results keep values and slots): a null
 * pointer, count < 1 or nring < 1 (or nring N beyond 2^31 - 1), an index out of range, a result sample this library did
 * not allocate or of another LWE dimension than the key's, count past the end of the result array, a null cloud key, the
 * slot pool exhausted, device memory exhausted (tfhe_hip_test_set_alloc_cap). */
int tfhe_hip_unpack_samples(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                            const int32_t *index, int32_t count, LweSample *result);
int tfhe_hip_unpack_samples_scattered(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                                      const int32_t *index, int32_t count, LweSample *const *result);
int tfhe_hip_unpack_samples_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_words, int32_t nring,
                                   const int32_t *index, int32_t count, LweSample *result);

/* ---- seed-compressed cloud keys: the public masks travel as a 40-byte seed ----
 * More than 90 % of a cloud key's words are public masks: uniform words that carry no information.  A compressed cloud key
 * holds the parameter set, a mask seed of ten words (ChaCha20 key[8], nonce[2]) and the bodies alone:
 *     bk_body[n][(k+1)l][N]        one body polynomial per TGSW row
 *     ksk_body[kN][t][base-1]      one body word per key-switch row of digit v = 1 .. base-1 (the digit-0 row is all zero
 *                                  and is never drawn, as in a plain key)
 * P128: 2,580,480 + 24,576 words = 10,420,224 bytes against the 103,350,272 of a plain cloud key.
 * The stream.  Mask word number m of the key is word 2 (m mod 8) + 1 of ChaCha20 block floor(m / 8) under (key, nonce)
 * (RFC 8439 block function with the 64-bit block counter starting at 0 in words 12, 13 and the nonce in words 14, 15:
 * tfhe_hip_test_chacha20_block) -- what the default generator's mask stream yields on its m-th draw.  Masks are numbered
 * in the order generate_keys draws them: first the BK in [i][row][u < k][j] order (n (k+1)l k N words), then the KSK in
 * [i][j][v = 1 .. base-1][q < n] order.  A sequential host loop and a random-access device kernel give the same words.
 * The expanded key is a cloud key in the plain layouts (bk [n][(k+1)l][k+1][N], ksk [kN][t][base][n+1]) whose mask words
 * are the stream words verbatim and whose bodies are the transmitted ones.
 * The rows.  A plain key adds the gadget term of a TGSW row with bloc < k to a MASK polynomial; a mask that comes from
 * a public seed cannot carry it ("mask + gadget" beside the seed would publish the key bit).  Here, for row = bloc l + jj
 * of BK_i, with mu = lwe_key[i] << (32 - (jj+1) Bgbit), in Z[X]/(X^N + 1) wrapping mod 2^32:
 *     body = sum_u mask_u S_u + e + mu              (on coefficient 0)     for bloc = k
 *     body = sum_u mask_u S_u + e - mu S_bloc(X)                           for bloc < k
 * the same phase body - sum_u mask_u S_u as a plain key's row, not the same words.  KSK rows are a plain key's:
 * body = <mask, lwe_key> + (v S_i << (32 - (j+1) basebit)) + e.
 * tfhe_hip_new_compressed_cloud_key: a fresh cloud key for an existing secret keyset -- noise from a fresh ChaCha20 stream
 * keyed by the OS, the mask seed ten fresh words of OS entropy.  _seeded (fixtures; NOT for keys that protect data): noise
 * from the seeded generator (xoshiro256** through splitmix64) started from noise_seed, N gaussians per BK row, then one
 * per KSK row, as generate_keys orders them; the mask seed as given.  _from_words: the cloud side (everything is copied).
 * NULL and the error set: a null argument, a parameter set the kernels cannot run (the message of a refused keyset).
 * Host only: no GPU is needed to make, read, save or host-expand one.
 * Accessors: the seed (10 words), the two body arrays (*count set), the bytes that travel (40 + 4 * both counts).
 * tfhe_hip_expand_cloud_key_host: a plain cloud keyset, bk and ksk filled on the host from a sequential stream; it reaches
 * the device like any loaded keyset.  The reference, and the way for a caller without a GPU.
 * tfhe_hip_expand_cloud_key: a cloud keyset that holds only seed and bodies.  At its first use the bodies are uploaded
 * (10 MB at P128) and the masks are written on the card, straight into the image the kernels read; device memory
 * exhausted there is recoverable like every key upload.  tfhe_hip_key_bk / _ksk and the cloud-key file export
 * materialise the host words on demand; everything else works on it unchanged.  Both are deleted with
 * delete_gate_bootstrapping_cloud_keyset; the compressed key may be deleted as soon as the call returns.
 * Files: one more kind of the container of tfhe_io.h (parameter record, seed, both body arrays), refused like the other
 * kinds on a wrong magic / version / kind, a declared size that does not match the parameters, or truncation. */
typedef struct TfheHipCompressedCloudKey TfheHipCompressedCloudKey;
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key(const TFheGateBootstrappingSecretKeySet *secret);
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key_seeded(const TFheGateBootstrappingSecretKeySet *secret,
                                                                    uint64_t noise_seed, const uint32_t *mask_seed10);
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key_from_words(const TFheGateBootstrappingParameterSet *params,
                                                                        const uint32_t *mask_seed10, const Torus32 *bk_body,
                                                                        const Torus32 *ksk_body);
void tfhe_hip_delete_compressed_cloud_key(TfheHipCompressedCloudKey *key);
const uint32_t *tfhe_hip_compressed_key_seed(const TfheHipCompressedCloudKey *key);
const Torus32 *tfhe_hip_compressed_key_bk_body(const TfheHipCompressedCloudKey *key, int64_t *count);
const Torus32 *tfhe_hip_compressed_key_ksk_body(const TfheHipCompressedCloudKey *key, int64_t *count);
int64_t tfhe_hip_compressed_key_bytes(const TfheHipCompressedCloudKey *key);
TFheGateBootstrappingCloudKeySet *tfhe_hip_expand_cloud_key_host(const TfheHipCompressedCloudKey *key);
TFheGateBootstrappingCloudKeySet *tfhe_hip_expand_cloud_key(const TfheHipCompressedCloudKey *key);
void tfhe_hip_export_compressed_cloud_key_toFile(FILE *F, const TfheHipCompressedCloudKey *key);
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key_fromFile(FILE *F);
/* test entries.  tfhe_hip_kernel_expand_masks: stream words first_word .. first_word + count - 1 (count in 1 .. 2^24)
 * from the device kernels' block function; 0 / -1.  tfhe_hip_test_key_image: the device BK image (which = 0) or the
 * compact KSK, row padding and zero row included (which = 1), of a keyset -- uploaded now if it was not yet -- copied into
 * out[capacity]; returns the word count (out may be NULL to ask for it), -1 on error.
 * tfhe_hip_last_expand_ms: device time of the two expand kernels of the last device expansion, between two stream events;
 * measured when kernel timing is on (tfhe_hip_set_kernel_timing), -1 before the first. */
int tfhe_hip_kernel_expand_masks(const uint32_t *mask_seed10, int64_t first_word, int32_t count, uint32_t *out);
int64_t tfhe_hip_test_key_image(const TFheGateBootstrappingCloudKeySet *cloud, int which, Torus32 *out, int64_t capacity);
double tfhe_hip_last_expand_ms(void);

/* ---- seed-compressed packing keys and ring samples: everything a client sends is bodies plus seeds ----
 * Half the words of a packing key and of a ring sample are uniform public masks.  Both travel with a mask seed of ten words
 * (ChaCha20 key[8], nonce[2]) in their place; the stream is the compressed cloud key's: mask word m is word 2 (m mod 8) + 1
 * of ChaCha20 block floor(m / 8) under (key, nonce), 64-bit block counter from 0 (tfhe_hip_test_chacha20_block).  k = 1.
 *
 * Compressed packing key.  It holds the parameter set, (pk_t, pk_basebit), the seed and the bodies body[n][t][N]:
 * P128, t = 8: 40 + 20,643,840 bytes against the 41,287,680 of the raw rows.  Masks are numbered in [i][p][j] order: the mask
 * polynomial of row (i, p) is stream words (i t + p) N .. + N - 1, blocks (i t + p) N/8 .. + N/8 - 1.  A row is the plain
 * key's row: body = mask * S + e + mu with mu = lwe_key[i] << (32 - (p+1) pk_basebit) on coefficient 0 and noise e of the
 * set's bk_stdev, in Z[X]/(X^N + 1) wrapping mod 2^32 -- the message sits on the body already, so unlike the cloud key's
 * TGSW rows no new row form is needed.  The expanded key IS a plain packing key: it equals
 * tfhe_hip_new_packing_key_from_words applied to the expanded rows [n][t][k+1][N] (mask = the stream words verbatim, body =
 * the transmitted one), word for word, and the packing definition above applies to it unchanged.
 * tfhe_hip_new_compressed_packing_key: noise from a fresh ChaCha20 stream keyed by the OS, the mask seed ten fresh words of
 * OS entropy.  _seeded (fixtures; NOT for keys that protect data): noise from the seeded generator (xoshiro256** through
 * splitmix64) started from noise_seed, N gaussians per row, rows in [i][p] order; the mask seed as given.  _from_words: the
 * cloud side (everything is copied; body holds n t N words).  pk_t = pk_basebit = 0: the set's own (ks_t, ks_basebit).
 * NULL and the error set, nothing made: a null argument, or a decomposition tfhe_hip_new_packing_key refuses.  None of this
 * touches the streams a keyset, a plain packing key or a compressed cloud key is drawn from.  Host only.
 * Accessors: the seed (10 words), the bodies (*count = n t N), the decomposition, the bytes that travel (40 + 4 * count).
 * tfhe_hip_expand_packing_key_host: a plain packing key with all rows filled on the host from a sequential stream -- the
 * reference, and the way for a caller without a GPU.
 * tfhe_hip_expand_packing_key: a packing key that holds only seed and bodies.  At its first pack the bodies are uploaded
 * (20.6 MB at P128 instead of 41.3 MB) and the masks are written on the card into the staging buffer the NTT transform
 * reads; device memory exhausted there is recoverable as for a plain key (the pack has no effect, nothing is held, a later
 * pack tries again).  tfhe_hip_packing_key_words materialises the host rows on demand; everything else that takes a
 * packing key works on it unchanged.  Both are deleted with tfhe_hip_delete_packing_key; the compressed key may be deleted
 * as soon as the call returns.
 * Files: one more kind of the container of tfhe_io.h (parameter record, decomposition, seed, bodies), refused like the other
 * kinds on a wrong magic / version / kind, a declared size that does not match, a refused decomposition, or truncation. */
typedef struct TfheHipCompressedPackingKey TfheHipCompressedPackingKey;
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t,
                                                                 int32_t pk_basebit);
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key_seeded(const TFheGateBootstrappingSecretKeySet *secret,
                                                                        int32_t pk_t, int32_t pk_basebit, uint64_t noise_seed,
                                                                        const uint32_t *mask_seed10);
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key_from_words(const TFheGateBootstrappingParameterSet *params,
                                                                            int32_t pk_t, int32_t pk_basebit,
                                                                            const uint32_t *mask_seed10, const Torus32 *body);
void tfhe_hip_delete_compressed_packing_key(TfheHipCompressedPackingKey *key);
const uint32_t *tfhe_hip_compressed_packing_key_seed(const TfheHipCompressedPackingKey *key);
const Torus32 *tfhe_hip_compressed_packing_key_body(const TfheHipCompressedPackingKey *key, int64_t *count);
int tfhe_hip_compressed_packing_key_decomposition(const TfheHipCompressedPackingKey *key, int32_t *pk_t, int32_t *pk_basebit);
int64_t tfhe_hip_compressed_packing_key_bytes(const TfheHipCompressedPackingKey *key);
TfheHipPackingKey *tfhe_hip_expand_packing_key_host(const TfheHipCompressedPackingKey *key);
TfheHipPackingKey *tfhe_hip_expand_packing_key(const TfheHipCompressedPackingKey *key);
void tfhe_hip_export_compressed_packing_key_toFile(FILE *F, const TfheHipCompressedPackingKey *key);
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key_fromFile(FILE *F);
/* Compressed ring samples.  A compressed ring sample is TFHE_HIP_RING_COMPRESSED_WORDS(N) = 10 + N words: the mask seed,
 * then the body (4,136 bytes instead of 8,192 at N = 1,024).  Mask word j of the sample is stream word j under that seed;
 * body = mask * S + mu + e with the set's bk_stdev, as tfhe_hip_ring_encrypt defines it.
 * ONE SEED PER SAMPLE: two samples under one key must never share mask words -- their difference would be the difference
 * of their messages plus noise.  The default forms therefore draw ten fresh words of OS entropy for every call (and the
 * noise from a fresh OS-keyed stream), and no entry takes a block offset into a shared stream.  The _compressed_seeded
 * forms (fixtures only) take the seed and draw the N noise samples from xoshiro256** started from noise_seed.
 * tfhe_hip_ring_expand_host: the plain (k+1) N words of a compressed sample of ring size N >= 1 -- the stream words, then
 * the body -- which tfhe_hip_packed_phase / _decrypt_bits decrypt and tfhe_hip_unpack_samples opens.  Needs no key.
 * Return 0, or -1 with tfhe_hip_last_error() set and the output untouched: a null argument, count outside 1..N. */
#define TFHE_HIP_RING_COMPRESSED_WORDS(N) (10 + (N))
int tfhe_hip_ring_encrypt_compressed(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words);
int tfhe_hip_ring_encrypt_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu,
                                            Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed);
int tfhe_hip_ring_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                          Torus32 *out_words);
int tfhe_hip_ring_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits,
                                                 int32_t count, Torus32 *out_words, const uint32_t *mask_seed10,
                                                 uint64_t noise_seed);
int tfhe_hip_ring_expand_host(const Torus32 *compressed_words, int32_t N, Torus32 *out_words);
/* The seeded unpack: tfhe_hip_unpack_samples and its scattered and device forms on nring compressed records of 10 + N words
 * each.  Semantics, argument checks, chunks of 8,192, slot renaming and errors are those of the plain forms; the result
 * words are those of tfhe_hip_unpack_samples on the host-expanded samples, word for word.  The mask polynomial is
 * regenerated on the card inside the extract kernel and never lies in global memory. */
int tfhe_hip_unpack_samples_seeded(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words, int32_t nring,
                                   const int32_t *index, int32_t count, LweSample *result);
int tfhe_hip_unpack_samples_seeded_scattered(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words,
                                             int32_t nring, const int32_t *index, int32_t count, LweSample *const *result);
int tfhe_hip_unpack_samples_seeded_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_compressed_words,
                                          int32_t nring, const int32_t *index, int32_t count, LweSample *result);
/* test entry.  tfhe_hip_test_pack_image: the device NTT image of a packing key (2 n t (k+1) N words) under the twiddles of
 * cloud key `bk` of the same set -- made now if it was not yet -- copied into out[capacity]; returns the word count (out may
 * be NULL to ask for it), -1 on error.  Mirrors tfhe_hip_test_key_image. */
int64_t tfhe_hip_test_pack_image(const TfheHipPackingKey *key, const TFheGateBootstrappingCloudKeySet *bk, Torus32 *out,
                                 int64_t capacity);
/* tfhe_hip_test_extract_rows: the rows of the last extract launch (plain or seeded; of an unpack, its last chunk) as the kernel
 * stored them, [rows][u_stride] with the padding behind word N -- the raw entries above return the rows without it.  Returns
 * the word count (0 before the first launch; out may be NULL to ask for it), copies only if it fits `capacity`; -1 on error. */
int64_t tfhe_hip_test_extract_rows(Torus32 *out, int64_t capacity);

/* ---- seed-compressed LWE sample arrays: what bootsSymEncrypt makes, as one seed and one word per sample ----
 * An LWE sample is n uniform public mask words and one body: 631 words at P128, of which 630 carry no information.  An
 * array of `count` fresh samples travels as ONE record of TFHE_HIP_LWE_COMPRESSED_WORDS(count) = 10 + count words: the
 * mask seed (ChaCha20 key[8], nonce[2]), then body[0 .. count).  1,024 bits at P128: 4,136 bytes against 2,584,576.
 * The stream is the compressed cloud key's.  Mask word i of sample j (i < n) is stream word m = j n + i: word
 * 2 (m mod 8) + 1 of ChaCha20 block floor(m / 8) under (key, nonce), 64-bit block counter from 0
 * (tfhe_hip_test_chacha20_block).  With s the secret LWE key,
 *     body[j] = sum_i a[j][i] s[i] + mu[j] + e[j]   mod 2^32,
 * e[j] gaussian of the set's ks_stdev: the deviation bootsSymEncrypt uses.  Expanded sample j is (a[j][0 .. n), body[j]):
 * exactly a fresh bootsSymEncrypt sample -- no key switch was paid, no cloud key is involved, any parameter set with
 * n <= 1,024 will do -- and word for word what tfhe_hip_import_samples takes.
 * A record holds at most TFHE_HIP_LWE_RECORD_MAX = 2^20 samples; more are refused.  With n <= 2^10 the last stream word
 * index is 2^20 * 2^10 - 1 = 2^30 - 1: every word index, and the end j n + n of every sample's run, stays below 2^31.
 * ONE SEED PER RECORD: two samples under one key must never share mask words -- their difference would be the difference
 * of their messages plus noise.  Within a record distinct samples use disjoint stream words by construction (sample j owns
 * words j n .. j n + n - 1).  The default encryptors therefore draw ten fresh words of OS entropy for every call (and the
 * noise from a fresh OS-keyed stream), and no entry takes an offset into a stream shared between records.  The _seeded
 * forms (fixtures only; NOT for samples that protect data) take the seed and draw the noise from xoshiro256** started from
 * noise_seed, one gaussian per sample in order.
 * tfhe_hip_sym_encrypt_bits_compressed: mu[j] = +-2^29 for bit j, as bootsSymEncrypt.  _torus_compressed: any messages
 * mu[0 .. count), the array twin of tfhe_hip_sym_encrypt_torus.  Host only: neither the device nor the streams of
 * bootsSymEncrypt, a keyset or any other object are touched.
 * tfhe_hip_lwe_expand_host: out_words[j] (n + 1 words) = expanded sample index[j] of a record of record_count samples;
 * index = NULL means 0 .. count - 1; any order, repeats allowed.  Needs no key.  The reference, and the way in for a caller
 * without a GPU.
 * Return 0, or -1 with tfhe_hip_last_error() set and the output untouched: a null argument, count < 1, a record_count (for
 * the encryptors: count) outside 1 .. 2^20, an index outside the record, n outside 1 .. 1,024. */
#define TFHE_HIP_LWE_COMPRESSED_WORDS(count) (10 + (count))
#define TFHE_HIP_LWE_RECORD_MAX (1 << 20)
int tfhe_hip_sym_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                         Torus32 *out_words);
int tfhe_hip_sym_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                                Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed);
int tfhe_hip_sym_encrypt_torus_compressed(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, int32_t count,
                                          Torus32 *out_words);
int tfhe_hip_sym_encrypt_torus_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, int32_t count,
                                                 Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed);
int tfhe_hip_lwe_expand_host(const Torus32 *compressed_words, int32_t n, int32_t record_count, const int32_t *index, int32_t count,
                             Torus32 *out_words);
/* The seeded import: result[j] becomes sample index[j] of the record (index = NULL: 0 .. count - 1; any order, repeats
 * allowed), its masks regenerated on the card straight into the sample's slot -- no expanded array ever lies in global
 * memory, and count words cross the bus instead of count (n + 1).  The result words are those of tfhe_hip_import_samples
 * applied to tfhe_hip_lwe_expand_host of the same record and index, word for word, the slot's padding included.
 * Semantics, as the unpack entries: every argument is checked before the device is looked at and before anything changes;
 * every result is renamed into a fresh slot; a flush in flight is completed first; recorded operations that have not run
 * stay recorded -- they cannot name the new slots.  The host form returns with the slots written (seed, the bodies the
 * index names and the lists went up through the pinned staging area); the device form reads the whole record from device
 * memory and returns with the work enqueued on tfhe_hip_stream() (the caller keeps device_compressed_words until the stream
 * has passed).  Host mirrors are stale until a decrypt, an export or tfhe_hip_sync_samples; in immediate mode they are
 * refreshed on return.  Any count is accepted; work proceeds in chunks of at most 8,192 samples.
 * result: `count` consecutive samples of one array; the scattered form takes `count` sample pointers instead.
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect (results keep values and slots): a null
 * pointer, count < 1, record_count outside 1 .. 2^20, an index outside the record, n above 1,024, a result sample this
 * library did not allocate or of another LWE dimension than the set's, count past the end of the result array, the slot
 * pool exhausted, device memory exhausted while the pool grows (tfhe_hip_test_set_alloc_cap). */
int tfhe_hip_import_samples_seeded(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                   int32_t record_count, const int32_t *index, int32_t count, LweSample *result);
int tfhe_hip_import_samples_seeded_scattered(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                             int32_t record_count, const int32_t *index, int32_t count, LweSample *const *result);
int tfhe_hip_import_samples_seeded_device(const TFheGateBootstrappingParameterSet *params, const void *device_compressed_words,
                                          int32_t record_count, const int32_t *index, int32_t count, LweSample *result);
/* test entries.  tfhe_hip_kernel_lwe_expand: the expand kernel alone, into scratch rows in place of pool slots;
 * out_words[count][n + 1], arguments as for the import; counts its launches.  tfhe_hip_test_expand_slots: the scratch rows of
 * the last such launch (of a call of several chunks, its last) as the kernel stored them, [rows][slot stride] with the
 * padding behind word n.  Returns the word count (0 before the first launch; out may be NULL to ask for it), copies only if
 * it fits `capacity`; -1 on error.  Mirrors tfhe_hip_test_extract_rows. */
int tfhe_hip_kernel_lwe_expand(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words, int32_t record_count,
                               const int32_t *index, int32_t count, Torus32 *out_words);
int64_t tfhe_hip_test_expand_slots(Torus32 *out, int64_t capacity);

/* ---- private selection: a CMUX tree under TGSW-encrypted index bits picks ONE of M resident ring samples ----
 * The leveled half of TFHE (upstream: tGswExternProduct, CMUX) outside a blind rotation.  A client sends d encrypted index
 * bits; the server selects one of up to 2^d ring samples it holds (a gallery of templates, one ring sample each) without
 * learning which, with M - 1 external products.  tfhe_hip_unpack_samples_device then opens the selected sample.  k = 1.
 *
 * TGSW sample of a bit: (k+1) l rows, each a TLWE sample of (k+1) N words under the ring key -- uniform masks, noise of the
 * set's bk_stdev.  Row (u, p), u <= k, p < l, encrypts zero, and bit << (32 - (p+1) Bgbit) is added to coefficient 0 of its
 * polynomial u.  Word order [u l + p][polynomial][N]: exactly one entry i of tfhe_hip_key_bk.  A selector of d bits has the
 * words of a bootstrapping key with n = d, bit 0 first; its device image is the bootstrapping-key image with n = d.
 * External product G (.) c of a TGSW sample G with a ring sample c, Bg = 2^Bgbit, offset = sum_{p < l} (Bg/2) << (32 - (p+1) Bgbit):
 *     dig[u][p][j] = (((c[u][j] + offset) >> (32 - (p+1) Bgbit)) & (Bg - 1)) - Bg/2        signed digits in [-Bg/2, Bg/2)
 *     (G (.) c)[w] = sum_{u, p} dig[u][p](X) * G.row(u, p)[w](X)        in Z[X]/(X^N + 1), wrapping mod 2^32, exact
 * -- the offset decomposition of the blind rotation.  CMUX(G, d1, d0) = d0 + G (.) (d1 - d0), the word-wise wrapping
 * difference taken first: it encrypts the phase of d1 where G encrypts 1 and that of d0 where it encrypts 0.
 * Tree over entries e[0 .. M), 1 <= M <= 2^d, an entry at or past M being the all-zero ring sample: level j = 0 .. d - 1
 * replaces the entries (2i, 2i+1) by CMUX(G_j, e[2i+1], e[2i]).  Bit 0 is the least significant index bit; after d
 * levels the one entry left encrypts the phase polynomial of entry index = sum_j bit_j 2^j, and noise only for an index at or
 * past M.  M = 1 with d = 0 is a copy.
 * Variance added per CMUX to every coefficient, to first order -- COMPUTED from the definition, not measured (torus units):
 *     key term       (k+1) l N E[dig^2] bk_stdev^2 <= (k+1) l N (Bg/2)^2 bk_stdev^2
 *     rounding term  at most (1 + k N) eps^2 / 3,   eps = 2^-(l Bgbit + 1) the precision of the decomposition
 * P128 (l = 3, Bgbit = 7, bk_stdev = 2^-25): 2.2e-8 + 1.9e-11, sigma <= 1.5e-4 per level, 4.7e-4 after ten levels -- beside
 * the 2.8e-3 the unpack's key switch adds and an operand margin of 1/16.  The l = 2, Bgbit = 10 set (bk_stdev = 7.18e-9):
 * 5.5e-8 + 7.8e-11, sigma <= 2.4e-4.  P2048 (l = 3, Bgbit = 6): 1.1e-8 + 2.5e-9, sigma <= 1.2e-4.
 *
 * Client side (host only, no GPU is needed).  tfhe_hip_tgsw_words: (k+1) l (k+1) N, the words of one bit (-1: null set).
 * tfhe_hip_tgsw_encrypt_bits writes count TGSW samples, 1 <= count <= 20, bits[b] != 0 taken as 1, out_words[count][(k+1) l]
 * [k+1][N].  The default form draws from two fresh ChaCha20 streams keyed by the OS, as a ring sample does; the seeded
 * form from ONE seeded generator (xoshiro256** through splitmix64) started from `seed` for this call alone.  Draw order,
 * both forms: for every bit, for every row (u, p) in word order: the k N mask words (one `torus` draw each), then the N
 * noise samples (one `gauss` draw each) -- the order of a bootstrapping key's rows.  0, or -1 with the error set and
 * out_words untouched.  A selector may also travel as a mask seed and its bodies, half the words: "seed-compressed selectors"
 * below.
 *
 * Server side.  tfhe_hip_new_selector copies nbits TGSW samples (0 <= nbits <= 20; nbits = 0 takes no words) of parameter
 * set `params`.  Every argument is checked before the device is looked at; NULL with the error set for a null pointer,
 * nbits out of range, a parameter set a cloud key would be refused for (k != 1, the CRT range, the gadget range of the
 * blind-rotate forms) or a gadget outside the CMUX kernel's own two bounds (peba1_amd/csrc/cmux.hpp: (k+1) l <= 18 at
 * N = 1024, <= 16 at N = 2048, and (k+1) l N (Bg/2) 2^31 below the exact range of the two-prime CRT).  The words and their
 * NTT image reach the device at the first select.
 * tfhe_hip_ring_select: ring_words holds M ring samples of (k+1) N words, 1 <= M <= 2^nbits; out_ring_words receives the
 * (k+1) N words of the tree's result.  The device form reads a gallery resident on the card and leaves the result there
 * (both 16-byte aligned), ready for tfhe_hip_unpack_samples_device.  Both are enqueued on tfhe_hip_stream(): the host form
 * returns with the words in place, the device form with the work enqueued, like tfhe_hip_unpack_samples_device (the
 * caller keeps both buffers until the stream has passed).  A select names no ciphertext slot: recorded operations stay
 * recorded, nothing is flushed, and a flush in flight is not waited for.  One kernel launch per tree level.
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect: a null pointer, a deleted selector, M < 1 or
 * M > 2^nbits, misaligned device words, device memory exhausted.
 * tfhe_hip_last_select_ms: the launches of the last select between two stream events (waits for the second); -1 unless
 * kernel timing (tfhe_hip_set_kernel_timing) was on. */
typedef struct TfheHipSelector TfheHipSelector;
int64_t tfhe_hip_tgsw_words(const TFheGateBootstrappingParameterSet *params);
int tfhe_hip_tgsw_encrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                               Torus32 *out_words);
int tfhe_hip_tgsw_encrypt_bits_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                      Torus32 *out_words, uint64_t seed);
TfheHipSelector *tfhe_hip_new_selector(const TFheGateBootstrappingParameterSet *params, const Torus32 *words, int32_t nbits);
void tfhe_hip_delete_selector(TfheHipSelector *selector);
int32_t tfhe_hip_selector_bits(const TfheHipSelector *selector);
int tfhe_hip_ring_select(const TfheHipSelector *selector, const Torus32 *ring_words, int32_t M, Torus32 *out_ring_words);
int tfhe_hip_ring_select_device(const TfheHipSelector *selector, const void *device_ring_words, int32_t M, void *device_out);
double tfhe_hip_last_select_ms(void);
/* raw test entry: `count` independent CMUXes (1 <= count <= 65,536) under bit bit_index of the selector in ONE launch,
 * out_words[c] = CMUX(G_bit, d1_words[c], d0_words[c]), (k+1) N host words each */
int tfhe_hip_kernel_ring_cmux(const TfheHipSelector *selector, int32_t bit_index, const Torus32 *d1_words, const Torus32 *d0_words,
                              int32_t count, Torus32 *out_words);
/* host-logic test entry: the two magnitude bounds of the CMUX kernel (peba1_amd/csrc/cmux.hpp) for gadget (l, Bgbit) of ring
 * size N (1024 or 2048), k = 1: bit 0 set = the MAC bound refuses it, bit 1 set = the CRT bound refuses it; -1 on bad
 * arguments (Bgbit outside 1..12, l Bgbit > 32). */
int tfhe_hip_test_select_bounds(int32_t N, int32_t l, int32_t Bgbit);

/* ---- private lookup in packed galleries: the tree picks a ring sample, the low index bits rotate it ----
 * The second half of a LUT evaluation with TGSW inputs.  The select's unit is a whole ring sample; an entry here is `width`
 * coefficients of one, so a gallery of 128-bit templates rests at 1 KB per template at N = 1024 instead of 8 KB, and a table
 * of single coefficients can be looked up at all: a public function of d encrypted bits, evaluated without a bootstrap.
 * No new key material: the selector is the select's.  k = 1.
 *
 * Monomial multiple of a ring sample c, 0 <= r < N, on both polynomials u:
 *     (X^(-r) c)[u][j] =  c[u][j + r]          for j + r < N
 *                        -c[u][j + r - N]      otherwise, wrapping mod 2^32
 * -- the convention of a test polynomial's rotation in the blind rotation.
 * Rotation step.  ROT(G, r, c) = CMUX(G, X^(-r) c, c) = c + G (.) (X^(-r) c - c): the CMUX, the external product and the offset
 * decomposition are exactly those of the private selection above, the word-wise wrapping difference taken first.
 * Lookup.  Entries of width w = 2^e coefficients, 1 <= w <= N.  S = N / w entries rest in one ring sample, s = log2 S; entry
 * i sits on coefficients (i mod S) w .. + w - 1 of sample i / S; a gallery of M entries holds R = ceil(M / S) ring samples.
 * The selector has d bits, bit 0 least significant, d >= s and 1 <= M <= 2^d.
 *   1. The tree of the private selection over the R samples under bits s .. d - 1: level j uses G_(s+j), a sample at or
 *      past R is the all-zero sample.
 *   2. For t = 0 .. s - 1 in ascending order: c <- ROT(G_t, w 2^t, c).
 *   3. The result is one ring sample; its coefficients 0 .. w - 1 carry the phase of entry i = sum_t bit_t 2^t.  The other
 *      coefficients carry other entries of the same sample, rotated: they are not part of the result's meaning.
 * w = N is word for word tfhe_hip_ring_select.  An index at or past M inside the last sample gives whatever the gallery
 * holds there; an index in a sample at or past R gives noise near zero.
 * Noise: at most (d - s) + s = d CMUX terms of the per-CMUX variance stated above (sigma <= 1.5e-4 each at P128) --
 * COMPUTED, not measured: a rotation step is a CMUX whose d1 is a monomial multiple of its d0.
 *
 * tfhe_hip_ring_lookup: ring_words holds the R ring samples of (k+1) N words; out_ring_words receives the (k+1) N words of
 * step 3 -- tfhe_hip_unpack_samples[_device] with indices 0 .. width - 1 opens the entry.  The device form reads a gallery
 * resident on the card and leaves the result there (both 16-byte aligned; the result must not overlap the gallery).  Both
 * are enqueued on tfhe_hip_stream() like the select's two forms: one kernel launch per tree level, then one per rotation
 * bit, d in all; the rotation steps go between two scratch samples sized before anything is enqueued, the last launch
 * writes a device destination directly.  The call names no ciphertext slot: recorded operations stay recorded, nothing is
 * flushed, and a flush in flight is not waited for.  tfhe_hip_last_select_ms covers a lookup too.
 * Every argument is checked before the device is looked at.  Return 0, or -1 with tfhe_hip_last_error() set and the call
 * without effect: a null pointer, a deleted selector, width not a power of two in 1 .. N, d < s, M < 1 or M > 2^d,
 * misaligned device words, device memory exhausted. */
int tfhe_hip_ring_lookup(const TfheHipSelector *selector, const Torus32 *ring_words, int32_t M, int32_t width, Torus32 *out_ring_words);
int tfhe_hip_ring_lookup_device(const TfheHipSelector *selector, const void *device_ring_words, int32_t M, int32_t width,
                                void *device_out);
/* raw test entry: `count` independent rotation steps (1 <= count <= 65,536) under bit bit_index of the selector in ONE
 * launch, out_words[c] = ROT(G_bit, rot, d0_words[c]), 1 <= rot < N, (k+1) N host words each */
int tfhe_hip_kernel_ring_cmux_rotate(const TfheHipSelector *selector, int32_t bit_index, int32_t rot, const Torus32 *d0_words,
                                     int32_t count, Torus32 *out_words);

/* ---- encrypted inner products on packed galleries: Hamming 1-to-N by ONE external product per ring sample ----
 * The leveled half computing on templates instead of moving them.  A TGSW sample may encrypt a small-integer POLYNOMIAL
 * instead of a bit; G (.) c is then the negacyclic product of that polynomial with the ring sample's message.  No new key
 * material on the server: the cloud key and the selector object do everything.  k = 1.
 *
 * TGSW sample of a polynomial p in Z[X]/(X^N + 1), given as N int32 coefficients: row (u, r), u <= k, r < l, is a TLWE
 * encryption of zero under the ring key, and p[j] << (32 - (r+1) Bgbit), wrapping, is added to coefficient j of its
 * polynomial u.  Word order and draw order (masks, then noise, row by row) are those of tfhe_hip_tgsw_encrypt_bits[_seeded]:
 * for p = bit (a constant polynomial) under the same seed the words are IDENTICAL to the bit encryptor's.
 * tfhe_hip_tgsw_encrypt_polys[_seeded]: polys[count][N], 1 <= count <= 20, out_words[count][(k+1) l][k+1][N]; host only;
 * 0, or -1 with the error set and out_words untouched.  tfhe_hip_new_selector takes such words unchanged: a selector's
 * samples may be polynomial samples (the tree and the lookup are meaningful for bit samples alone).
 * Product.  G (.) c exactly as defined for the private selection: the offset decomposition of c, signed digits, exact in
 * Z[X]/(X^N + 1) mod 2^32.  The row words of a polynomial sample are arbitrary 32-bit words like any other, so the two
 * bounds of peba1_amd/csrc/cmux.hpp hold unchanged; there is no new bound.
 * Probe layout.  For s_0 .. s_(w-1):  p[0] = s_0,  p[N - i] = -s_i for 1 <= i < w,  0 elsewhere: p = sum_i s_i X^(-i).
 * Why.  Let t be the message of a ring sample in the lookup's layout (S = N / w entries of w coefficients, entry e on
 * coefficients e w .. e w + w - 1).  A term t[j] p[m] of p t lands on coefficient e w iff j + m = e w or j + m = N + e w.
 * With m in {0} u (N - w, N) the first case forces m = 0, j = e w; the second m = N - i, j = e w + i with 1 <= i < w,
 * where the wrap's sign cancels the minus of p[N - i].  So coefficient e w of p t is sum_i s_i t[e w + i], the inner
 * product of the probe with entry e, and nothing of any other entry enters it.
 * Inner.  The gallery is R ring samples holding M <= R S entries in the lookup's layout, R = ceil(M / S):
 *     result[i] = KeySwitch(Extract_((i mod S) w)(G_b (.) c_(i / S)))        for i < M, b = sample_index,
 * Extract and KeySwitch being those of tfhe_hip_unpack_samples.  The product and the S extractions of a ring sample are
 * ONE kernel launch of R workgroups; the key switch is the unpack's.
 * Variance of result[i], to first order -- COMPUTED from the definition, not measured (torus units):
 *     key term       (k+1) l N E[dig^2] bk_stdev^2,  E[dig^2] = Bg^2 / 12 for uniform digits
 *     rounding term  (1 + k N) |p|_2^2 eps^2 / 3,  eps = 2^-(l Bgbit + 1) -- FOR PROBE COEFFICIENTS OF RANDOM SIGNS: the exact
 *                    weight is E_S[|p|_2^2 + |p S|_2^2], which coefficients of one sign (a code of all 0 or all 1, long runs)
 *                    raise to as much as N^3 / 12, 87 times more at w = N ("TGSW products over several ring samples" below,
 *                    peba1_amd.identify.probe_rounding_weight)
 *     input term     |p|_2^2 times the ring sample's variance (bk_stdev^2 for a fresh one)
 *     the unpack's key-switch term, N t ks_stdev^2 + (N / 2) prec^2 / 3
 * P128, w = 128, s_i = +-1 (|p|_2^2 = 128): before the key switch 2.2e-8 (with (Bg/2)^2 in place of E[dig^2], the bound
 * the select states) + 2.5e-9 + 1e-13, sigma ~ 1.6e-4; after it sigma ~ 2.8e-3.
 * The rounding term takes the decomposition's error as zero-mean, AND ON A GALLERY MADE BY PLAIN tfhe_hip_ring_encrypt IT IS
 * NOT.  The offset decomposition KEEPS the top l Bgbit bits of a word, so the error of a word as it arrives lies in
 * [0, 2 eps) with mean eps, and a probe of coefficient sum s = sum_i s_i shifts coefficient e w of the result's phase by
 *     bias[e w] = -(p * eps (1 - ones * S))[e w],    |bias| <= |s| (1 + N / 2) eps to first order,
 * S the ring key, `ones` the all-one polynomial: 1.3e-3 for s = 11 (a random 128-bit probe), 1.6e-2 for 128 equal bits at
 * P128 -- above Delta / 2 = 9.8e-4, so distances from such a gallery are NOT exact to round.
 * tfhe_hip_ring_center_words adds 2^(31 - l Bgbit), wrapping, to `count` words in place (nothing where l Bgbit = 32): applied
 * ONCE to every word of a gallery -- a public operation on ciphertext words, client or server, at enrolment -- it makes the
 * kept bits those of the rounded word and the error the zero-mean [-eps, eps) the term assumes.  Everything stated below for
 * distances assumes a centred gallery.  0, or -1 with the error set and the words untouched: a null pointer, count < 0.
 * tfhe_hip_ring_inner itself computes the product as defined, on the words it is given.
 *
 * Hamming distance on top of this.  The enrolled entry carries a_i Delta, Delta = 2^-(log2 w + 2), so distances stay
 * inside [0, 1/4]; the probe is s_i = 1 - 2 b_i, and inner = (sum_i a_i - 2 sum_i a_i b_i) Delta.  The client also sends
 * ONE LWE sample of (sum_i b_i) Delta (tfhe_hip_sym_encrypt_torus): inner + addend = d Delta, d the Hamming distance.  The
 * server forms (tau + 1/2) Delta - (inner + addend) with tfhe_hip_linear (recorded like any other op) and applies
 * tfhe_hip_lut_bootstrap with tfhe_hip_new_lut_constant(1/8): the output is TRUE iff d <= tau.
 * THIS DECISION IS NOT EXACT NEAR THE THRESHOLD.  The bootstrap's modulus switch adds about (1 + n/2) / (12 (2N)^2)
 * (sigma ~ 2.5e-3 at P128) to the key switch's 2.8e-3: sigma_dec ~ 3.7e-3 in all, 1.9 Delta at w = 128.  The decision is
 * guaranteed only for |d - tau - 1/2| Delta >= 6 sigma_dec (peba1_amd.identify.inner_decision_band computes the band).
 * The distance BEFORE the key switch is exact to round: Delta / 2 = 9.8e-4 is 6 sigma at w = 128.
 * Euclidean distance on 8-bit features does NOT fit the torus (23 bits of range against sigma 1.6e-4): OUT OF SCOPE.
 *
 * tfhe_hip_ring_inner follows tfhe_hip_unpack_samples throughout: every result is renamed into a fresh slot; all arguments
 * are checked before anything changes; a flush in flight is completed first; recorded operations stay recorded; work runs
 * in chunks of at most 8,192 rows; the host form returns with the slots written, the device form (ring words resident on
 * the card, 16-byte aligned) with the work enqueued on tfhe_hip_stream().  tfhe_hip_last_select_ms covers the product
 * launch.  Return 0, or -1 with tfhe_hip_last_error() set and the call without effect (results keep values and slots): a
 * null pointer, a deleted selector, sample_index outside the selector, a selector of another ring (N, k) than the key's --
 * the gadget (l, Bgbit) MAY differ: the product runs under the selector's, the key serves the key switch alone --, width
 * not a power of two in 1 .. N, M < 1, misaligned device words, a result sample this library did not allocate or of another
 * LWE dimension than the key's, M past the end of the result array, the slot pool exhausted, device memory exhausted. */
int tfhe_hip_tgsw_encrypt_polys(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                Torus32 *out_words);
int tfhe_hip_tgsw_encrypt_polys_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                       Torus32 *out_words, uint64_t seed);
int tfhe_hip_ring_center_words(const TFheGateBootstrappingParameterSet *params, Torus32 *words, int64_t count);
int tfhe_hip_ring_inner(const TfheHipSelector *selector, int32_t sample_index, const TFheGateBootstrappingCloudKeySet *bk,
                        const Torus32 *ring_words, int32_t M, int32_t width, LweSample *result);
int tfhe_hip_ring_inner_device(const TfheHipSelector *selector, int32_t sample_index, const TFheGateBootstrappingCloudKeySet *bk,
                               const void *device_ring_words, int32_t M, int32_t width, LweSample *result);
/* raw test entry: out_words[c] = G_bit (.) ring_words[c], the full product, 1 <= count <= 65,536 in ONE launch, (k+1) N
 * host words each */
int tfhe_hip_kernel_ring_product(const TfheHipSelector *selector, int32_t bit_index, const Torus32 *ring_words, int32_t count,
                                 Torus32 *out_words);
/* raw test entry: the extracted rows before the key switch, out_rows[i] (kN+1 words) = Extract_((i mod S) width)(G_bit (.)
 * ring sample i / S) for i < M, (R - 1) S < M <= R S; no slots involved */
int tfhe_hip_kernel_ring_inner_rows(const TfheHipSelector *selector, int32_t bit_index, const Torus32 *ring_words, int32_t R,
                                    int32_t M, int32_t width, Torus32 *out_rows);

/* ---- ring sample times public polynomials: one probe against a CLEAR gallery, or a clear probe against an encrypted one ----
 * The product of a ring sample with a polynomial the server knows needs no gadget, no decomposition and no TGSW sample:
 * q (a, b) = (q a, q b).  No key material at all for the product; the cloud key serves the key switch alone.  k = 1, N = 1024
 * or 2048.
 *
 * Public polynomial.  q is N int32 coefficients with |q[j]| <= T, T = TFHE_HIP_PUBLIC_MAX_COEF(N) the largest power of two
 * with N T 2^31 < CRT_EXACT_LIMIT (peba1_amd/csrc/ntt_field.hpp, 0.36 P0 P1 = 2^52.5): 2^11 at N = 1024, 2^10 at N = 2048
 * (peba1_amd/csrc/ring_public.hpp derives it; a static_assert ties the macro to it).  Worst case, which reaches N T 2^31
 * exactly at coefficient N - 1: all q[j] = -T against words 0x80000000.
 * Product.  (q * c)[u] = q(X) c[u](X) for u = 0 and 1, in Z[X]/(X^N + 1), the words of c taken as signed 32-bit integers,
 * the result wrapping mod 2^32: coefficient m is sum_(i+j=m) q[i] c[u][j] - sum_(i+j=m+N) q[i] c[u][j].  q = 1 is the
 * identity; q = X^r gives (X^r c)[u][j] = c[u][j - r] for j >= r and -c[u][j - r + N] below it -- the private lookup's
 * monomial convention with the sign of the exponent flipped: X^r (X^(-r) c) = c.
 * Inner products.  The layouts are those of the encrypted inner products above: one factor in the lookup's gallery layout
 * (entry e on coefficients e w .. e w + w - 1, S = N / w entries to a polynomial), the other in the probe layout
 * p = sum_i s_i X^(-i).  Coefficient e w of the product is the inner product with entry e alone -- the argument stated
 * there ("Why.") is symmetric in the two factors and holds whichever of them is the ciphertext.
 * In the headline use the PROBE is the ring sample -- the client encrypts the torus polynomial s_i Delta in probe layout,
 * mu[0] = s_0 Delta, mu[N - i] = -s_i Delta, with tfhe_hip_ring_encrypt[_seeded] or its seed-compressed forms (8 KB, or
 * 4,136 bytes, against the 48 KB of a TGSW probe at P128) -- and the GALLERY is R public polynomials of 0/1 coefficients:
 *     result[i] = KeySwitch(Extract_((i mod S) w)(q_(i / S) * c))        for i < M <= R S,
 * Extract and KeySwitch being those of tfhe_hip_unpack_samples, exactly as in tfhe_hip_ring_inner.  The product and the S
 * extractions of a polynomial are ONE kernel launch of ceil(M / S) workgroups; the key switch is the unpack's.
 * Variance before the key switch -- COMPUTED from the definition, not measured (torus units): |q|_2^2 times the ring
 * sample's variance (bk_stdev^2 for a fresh one).  There is no other term, and no bias: nothing is decomposed, nothing is
 * rounded, and there is nothing to centre.  For a 0/1 polynomial |q|_2^2 <= N:
 *     P128 (N = 1024, bk_stdev 2^-25)            at most 2^-40 = 9.1e-13,  sigma <= 9.5e-7
 *     the l = 2 set (N = 1024, bk_stdev 7.18e-9)   at most 5.3e-14,          sigma <= 2.3e-7
 *     P2048 (N = 2048, bk_stdev 2^-25)           at most 2^-39 = 1.8e-12,  sigma <= 1.3e-6
 * (the gadget does not enter; the TGSW route's sigma ~ 1.6e-4 at P128 is about 170 times the first).
 * Hamming decision on top: UNCHANGED.  The same addend sample, tfhe_hip_linear, the constant-1/8 LUT bootstrap and the same
 * peba1_amd.identify.inner_decision_band: the band is set by the key switch and the bootstrap's modulus switch, which this
 * section does not touch.  THIS DOES NOT MAKE THE DECISION EXACT NEAR THE THRESHOLD; only the distance before the key switch
 * gains (Delta / 2 = 9.8e-4 is a thousand sigma here).
 * OUT OF SCOPE: Euclidean distance on 8-bit features (the range argument of the section above stands), an exact decision
 * inside the band, multi-key batching, libpeba1-dist, k > 1, recording these calls in the op graph.
 *
 * tfhe_hip_new_public_gallery copies polys[R][N], 1 <= R <= 2^20; host only -- the device image (the canonical NTT residues
 * under both primes, 8 KB a polynomial) is made once, at the first product, and kept on the card until the gallery is
 * deleted.  Every argument is checked before the device is looked at; NULL with the error set for: a null pointer, k != 1
 * or N outside {1024, 2048}, R out of range, a coefficient past T (the message names the first offending index).
 * tfhe_hip_public_gallery_polys: R, or -1 with the error set for a null or deleted gallery.
 * tfhe_hip_ring_mul_public: out[g] = q_(poly_index + (npolys == 1 ? 0 : g)) * c_(count == 1 ? 0 : g), (k+1) N words each.  npolys == 1 broadcasts one
 * polynomial over `count` samples (the clear probe against an encrypted gallery); count == 1 broadcasts one sample over
 * npolys polynomials; otherwise npolys == count and the product is pairwise: max(npolys, count) products in ONE launch,
 * both at most 65,536.  Enqueued on tfhe_hip_stream() like the select: the call names no ciphertext slot, recorded
 * operations stay recorded, nothing is flushed, a flush in flight is not waited for.  The host form returns with the words
 * in place; the device form (both 16-byte aligned, the destination overlapping no ring word) with the work enqueued.
 * Return 0, or -1 with the error set and the call without effect: a null pointer, a deleted gallery, npolys or count out
 * of range, polynomials outside the gallery, npolys != count with neither 1, misaligned or overlapping device words, device
 * memory exhausted.
 * tfhe_hip_ring_inner_public follows tfhe_hip_ring_inner in every contract: every result is renamed into a fresh slot; all
 * arguments are checked before anything changes; a flush in flight is completed first; recorded operations stay recorded;
 * work runs in chunks of at most 8,192 rows; the host form returns with the slots written, the device form (the probe's
 * (k+1) N words resident on the card, 16-byte aligned) with the work enqueued on tfhe_hip_stream().
 * tfhe_hip_last_select_ms covers the product launch (and that of tfhe_hip_ring_mul_public).  Return 0, or -1 with the error
 * set and the call without effect (results keep values and slots): a null pointer, a deleted gallery, a gallery of another
 * ring (N, k) than the key's, width not a power of two in 1 .. N, M < 1, M past the R S entries of the gallery, misaligned
 * device words, a result sample this library did not allocate or of another LWE dimension than the key's, M past the end of
 * the result array, the slot pool exhausted, device memory exhausted. */
#define TFHE_HIP_PUBLIC_MAX_COEF(N) ((N) == 2048 ? 1024 : (N) == 1024 ? 2048 : 0)
typedef struct TfheHipPublicGallery TfheHipPublicGallery;
TfheHipPublicGallery *tfhe_hip_new_public_gallery(const TFheGateBootstrappingParameterSet *params, const int32_t *polys, int32_t R);
void tfhe_hip_delete_public_gallery(TfheHipPublicGallery *gallery);
int32_t tfhe_hip_public_gallery_polys(const TfheHipPublicGallery *gallery);
int tfhe_hip_ring_mul_public(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t npolys, const Torus32 *ring_words,
                             int32_t count, Torus32 *out_ring_words);
int tfhe_hip_ring_mul_public_device(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t npolys,
                                    const void *device_ring_words, int32_t count, void *device_out);
int tfhe_hip_ring_inner_public(const TfheHipPublicGallery *gallery, const TFheGateBootstrappingCloudKeySet *bk,
                               const Torus32 *probe_ring_words, int32_t M, int32_t width, LweSample *result);
int tfhe_hip_ring_inner_public_device(const TfheHipPublicGallery *gallery, const TFheGateBootstrappingCloudKeySet *bk,
                                      const void *device_probe_ring_words, int32_t M, int32_t width, LweSample *result);
/* raw test entry: the products of tfhe_hip_ring_mul_public's host form, after a flush in flight has completed */
int tfhe_hip_kernel_ring_public_product(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t npolys,
                                        const Torus32 *ring_words, int32_t count, Torus32 *out_words);
/* raw test entry: the extracted rows before the key switch, out_rows[i] (kN+1 words) = Extract_((i mod S) width)(q_(i / S) *
 * probe) for i < M <= R S; no slots involved */
int tfhe_hip_kernel_ring_public_rows(const TfheHipPublicGallery *gallery, const Torus32 *probe_ring_words, int32_t M, int32_t width,
                                     Torus32 *out_rows);
/* host-logic test entry: 0 if coefficients up to T pass the CRT bound N T 2^31 < CRT_EXACT_LIMIT at ring size N, 1 if not;
 * -1 with the error set for N outside {1024, 2048} or T < 1 */
int tfhe_hip_test_public_bounds(int32_t N, int32_t T);

/* ---- public products over several ring samples: long and masked templates ----
 * sum_t q_t * c_t over K = `terms` ring samples c_0 .. c_(K-1): the public product above as a matrix-vector product instead
 * of a diagonal one.  The sum is taken in the NTT domain -- per prime and output polynomial K forward transforms, K
 * products into one 64-bit accumulator, ONE reduction and ONE inverse transform -- followed by one CRT, one extraction and
 * one key switch.  1 <= terms <= TFHE_HIP_PUBLIC_MAX_TERMS = 8: one accumulator takes 14 products at N = 1024 and 13 at
 * N = 2048 before its reduction leaves the inverse transform's 4 P (peba1_amd/csrc/ring_public.hpp MAC bound); 8 is the
 * largest power of two under both, and a static_assert ties the macro to the derivation.  terms = 1 computes the words of
 * the single-term calls.
 *
 * Groups.  The gallery is read as groups of K consecutive polynomials: R = polys / K groups, group g being polynomials
 * g K .. g K + K - 1; the polynomial count must be a multiple of K.  The probe is K ring samples, [K][(k+1) N] words.
 * CRT bound of a group.  N (sum_t max|q_t|) 2^31 < CRT_EXACT_LIMIT: the largest magnitudes of a group's K polynomials sum
 * to at most T = TFHE_HIP_PUBLIC_MAX_COEF(N), what ONE polynomial is held to.  The gallery keeps max|q| of every polynomial
 * from its construction; every group a call uses is checked before the device is touched, and the refusal names the first
 * offending group.  Worst case, which reaches N T 2^31 exactly at coefficient N - 1: all coefficients -T / K against words
 * 0x80000000.
 * Product.  tfhe_hip_ring_mul_public_sum: out[g] = sum_(t < K) q_(poly_index + g K + t) * c_t for g < ngroups, (k+1) N words
 * each, 1 <= ngroups <= 65,536, ONE launch; every other contract is tfhe_hip_ring_mul_public's.
 * Inner products.  tfhe_hip_ring_inner_public_sum:
 *     result[i] = KeySwitch(Extract_((i mod S) w)(sum_(t < K) q_((i / S) K + t) * c_t))        for i < M <= R S,
 * S = N / w: ONE launch of ceil(M / S) workgroups per chunk of 8,192 rows, and the unpack's key switch under the same plans.
 * Every contract is tfhe_hip_ring_inner_public's: all arguments are checked before anything changes; every result is renamed
 * into a fresh slot; a flush in flight is completed first; recorded operations stay recorded; the device form (the probe's
 * K (k+1) N words resident on the card, 16-byte aligned) returns with the work enqueued on tfhe_hip_stream();
 * tfhe_hip_last_select_ms covers the launch.  TfheHipStats has no new field: the key switches count as `keyswitches`.
 * Variance before the key switch -- COMPUTED from the definition, not measured: sum_t |q_t|_2^2 times the ring samples'
 * variance (bk_stdev^2 for fresh ones).  There is no other term.
 *
 * What it is for (peba1_amd.identify).
 * Long templates: an entry of K w bits, term t holding bits t w .. t w + w - 1 in the lookup's layout against K probe samples
 * in probe layout -- an iris code of 2,048 bits at P128 is K = 2, w = 1,024.  The Hamming decision's tail is unchanged, with
 * Delta = 2^-(log2(K w) + 2) and the addend sample.
 * Masked templates: code bits b (probe), g (gallery) and validity masks m, n (1 = valid); s = 1 - 2 b, sigma = 1 - 2 g.  The
 * probe encrypts, per chunk of w bits, the TWO polynomials s_i m_i Delta and m_i Delta in probe layout; the gallery holds,
 * per chunk, -den sigma_i n_i and (den - 2 num) n_i.  The one summed product is D Delta with
 *     D = (den - 2 num) valid - den (agree - disagree) = 2 (den disagree - num valid),
 * valid = sum m n, and disagree / valid <= num / den iff D <= 0.  The server forms Delta / 2 - D Delta with tfhe_hip_linear
 * (a constant alone; there is NO addend sample) and applies the constant-1/8 LUT bootstrap: TRUE iff D <= 0.
 * Delta = 2^-(2 + ceil(log2(den L))), L the entry length, keeps |D| Delta below 1/2.  A masked match is one row, one key
 * switch and one bootstrap per entry: what an unmasked one is.
 * The weights den and den - 2 num live in the gallery polynomials and so are applied BEFORE the key switch, where the noise
 * is the ring sample's: sigma^2 = (den^2 + (den - 2 num)^2) (valid gallery bits) bk_stdev^2 in torus units, 3.6e-5 at P128
 * for 2,048 bits at 8/25 -- against the key switch's 2.8e-3, which enters ONCE.  The two-product route (valid and
 * agree - disagree as two inner products, weighted by tfhe_hip_linear afterwards) multiplies the key switch's sigma by
 * sqrt(den^2 + (den - 2 num)^2) = 26.6 at 8/25, 7.4e-2, at twice the product launches and key switches and with a recorded
 * linear op per entry.  COMPUTED, not measured.
 * THE DECISION IS NOT EXACT INSIDE THE BAND: it is guaranteed only for |D| >= g, g the smallest integer with
 * (g - 1/2) Delta >= 6 sigma_dec (peba1_amd.identify.clear_decision_band; sigma_dec ~ 3.7e-3 at P128 as above).  Computed at
 * P128: long 2,048-bit codes, Delta = 2^-13: g = 184 bits of distance; masked 2,048-bit codes at 8/25, Delta = 2^-18:
 * g = 5,869 in units of D, which is 118 disagreeing bits at full validity (D moves by 2 den = 50 a bit).
 * OUT OF SCOPE: an exact decision inside the band, Euclidean distance, probe hoisting (the K forward transforms of the
 * probe are repeated by every workgroup), multi-key batching, recording these calls in the op graph, libpeba1-dist, k > 1.
 * (The TGSW counterpart, for galleries that rest encrypted, is tfhe_hip_ring_inner_sum below.)
 *
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect (outputs untouched, results keep values and
 * slots): terms outside 1 .. TFHE_HIP_PUBLIC_MAX_TERMS, a polynomial count that is not a multiple of terms, a group past the
 * CRT bound, ngroups outside 1 .. 65,536 or groups outside the gallery, and every refusal of the single-term calls. */
#define TFHE_HIP_PUBLIC_MAX_TERMS 8
int tfhe_hip_ring_mul_public_sum(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t terms, int32_t ngroups,
                                 const Torus32 *ring_words, Torus32 *out_ring_words);
int tfhe_hip_ring_mul_public_sum_device(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t terms, int32_t ngroups,
                                        const void *device_ring_words, void *device_out);
int tfhe_hip_ring_inner_public_sum(const TfheHipPublicGallery *gallery, const TFheGateBootstrappingCloudKeySet *bk,
                                   const Torus32 *probe_ring_words, int32_t terms, int32_t M, int32_t width, LweSample *result);
int tfhe_hip_ring_inner_public_sum_device(const TfheHipPublicGallery *gallery, const TFheGateBootstrappingCloudKeySet *bk,
                                          const void *device_probe_ring_words, int32_t terms, int32_t M, int32_t width,
                                          LweSample *result);
/* raw test entry: the sums of tfhe_hip_ring_mul_public_sum's host form, after a flush in flight has completed */
int tfhe_hip_kernel_ring_public_sum_product(const TfheHipPublicGallery *gallery, int32_t poly_index, int32_t terms, int32_t ngroups,
                                            const Torus32 *ring_words, Torus32 *out_words);
/* raw test entry: the extracted rows before the key switch, out_rows[i] (kN+1 words) = Extract_((i mod S) width)(sum_t
 * q_((i / S) terms + t) * probe_t) for i < M <= R S; no slots involved */
int tfhe_hip_kernel_ring_public_sum_rows(const TfheHipPublicGallery *gallery, const Torus32 *probe_ring_words, int32_t terms,
                                         int32_t M, int32_t width, Torus32 *out_rows);
/* host-logic test entry: 0 if a group of `terms` polynomials whose largest magnitudes sum to coef_sum passes the CRT bound
 * at ring size N (coef_sum <= TFHE_HIP_PUBLIC_MAX_COEF(N)), 1 if not; -1 with the error set for N outside {1024, 2048},
 * terms outside 1 .. TFHE_HIP_PUBLIC_MAX_TERMS or coef_sum < 0 */
int tfhe_hip_test_public_sum_bounds(int32_t N, int32_t terms, int64_t coef_sum);
/* host-logic test entry: the magnitude recurrences of the wave NTT as the library states them, for a transform of 2^logn
 * points (logn = 9, 10, 11) on inputs |x| <= x0.  fwd2 = {pack_forward_bound(logn, x0), br_forms forward_bound(logn, x0 / P,
 * no table)}: |outputs| / P of the forward transform.  plan25 = make_inv_plan(logn): {nsteps, fan[12], renorm[12]}, and
 * *inv_out its out_bound.  -1 with the error set for other arguments. */
int tfhe_hip_test_ntt_bounds(int32_t logn, double x0, double *fwd2, int32_t *plan25, double *inv_out);

/* ---- TGSW products over several ring samples: long and masked templates against an ENCRYPTED gallery ----
 * sum_t G_(b+t) (.) c_(gK+t) over K = `terms` ring samples: tfhe_hip_ring_inner's external product as a matrix-vector
 * product, for the gallery the server must not see.  The K probe polynomials are K samples of ONE selector (plain or
 * seed-compressed: no new key material), the gallery is read as groups of K consecutive ring samples.  The sum is taken in
 * the NTT domain -- per prime K (k+1) l forward transforms into the same two 64-bit accumulators, ONE inverse transform per
 * output polynomial -- followed by one CRT, one extraction and one key switch, where K calls of tfhe_hip_ring_inner take K
 * of each and a recorded linear op per entry.  Exactly, in Z[X]/(X^N + 1) mod 2^32:
 *     out[g] = sum_(t < K) G_(b+t) (.) c_(gK+t),         b = sample_index,
 * G (.) c as defined for the private selection (the offset decomposition of c, signed digits).  terms = 1 computes the
 * words of tfhe_hip_ring_inner and tfhe_hip_kernel_ring_product.
 *
 * Admissible terms (peba1_amd/csrc/ring_inner_sum.hpp derives both bounds and static_asserts them).
 * MAC bound.  One accumulator takes 18 rows (N = 1024) or 16 (N = 2048) before its reduction leaves the inverse transform's
 * 4 P, and a term has (k+1) l rows, 6 at the built-in gadgets.  So the accumulator is FOLDED after every block of 18 (16)
 * rows: y = acc 2^-32 mod P by one Montgomery reduction, then acc = y (2^32 mod P), the same residue again and below
 * 0.102 P^2 -- a sixtieth of one row -- so the block lengths stay 18 and 16 and this side sets no limit on K.  A block
 * boundary may fall inside a term.
 * CRT bound.  K (k+1) l N (Bg/2) 2^31 < CRT_EXACT_LIMIT: K <= 7 at both built-in gadgets, (3, 7) at N = 1024 and (3, 6) at
 * N = 2048.  All digits at -Bg/2 against row words 0x80000000 reach the left side exactly.
 * tfhe_hip_ring_inner_sum_max_terms(params): the largest K both bounds take for that set's gadget, capped at
 * TFHE_HIP_INNER_MAX_TERMS = 8 -- 7 at both built-in sets; -1 with the error set for a null set or a gadget outside the
 * CMUX kernel's own two bounds (cmux_gadget_error of peba1_amd/csrc/cmux.hpp).  It does not look at what else
 * tfhe_hip_new_selector refuses a set for (a set no cloud key is accepted with): no selector exists for such a set.
 *
 * Product.  tfhe_hip_ring_mul_tgsw_sum: ring_words [ngroups][terms][(k+1) N], out [ngroups][(k+1) N], 1 <= ngroups <=
 * 65,536, ONE launch; names no pool slot, completes no flight; the device form (words resident, 16-byte aligned, the
 * destination apart from the source) returns with the work enqueued on tfhe_hip_stream().
 * Inner products.  tfhe_hip_ring_inner_sum: the gallery is R groups holding M <= R S entries, S = N / w, R = ceil(M / S);
 * entry i spans the K samples of group i / S, term t holding its coefficients t w .. t w + w - 1 in the lookup's layout:
 *     result[i] = KeySwitch(Extract_((i mod S) w)(sum_(t < K) G_(b+t) (.) c_((i / S) K + t)))        for i < M.
 * Every contract is tfhe_hip_ring_inner's: all arguments are checked before anything changes; a flush in flight is completed
 * first; every result is renamed into a fresh slot; recorded operations stay recorded; work runs in chunks of at most 8,192
 * rows; tfhe_hip_last_select_ms covers the launch; TfheHipStats has no new field: the key switches count as `keyswitches`.
 * Variance before the key switch -- COMPUTED from the definition, not measured -- is the sum over the K terms of
 * tfhe_hip_ring_inner's three terms (torus units):
 *     key term       K (k+1) l N E[dig^2] bk_stdev^2
 *     rounding term  (sum_t W(p_t)) eps^2 / 3,  eps = 2^-(l Bgbit + 1), ON A CENTRED GALLERY,  W(p) = E_S[|p|_2^2 + |p S|_2^2]
 *     input term     (sum_t |p_t|_2^2) times the ring samples' variance
 * and the gallery must be centred with tfhe_hip_ring_center_words exactly as for tfhe_hip_ring_inner: without it every
 * term carries that call's bias.  W(p) over a uniform binary key S is |p|_2^2 (1 + N / 4) + sum_j sigma_j^2 / 4, sigma_j the
 * signed coefficient sum of p = sum_i v_i X^(-i) split at the wrap of coefficient j.  For coefficients of random signs that is
 * (1 + N / 2) |p|_2^2, inside the (1 + k N) |p|_2^2 tfhe_hip_ring_inner states.  FOR COEFFICIENTS OF ONE SIGN IT IS NOT: the
 * mask polynomial m of a masked probe has sigma_j up to its coefficient sum, W = N^3 / 12 = 9.0e7 at 1,024 valid bits against
 * (1 + N) |p|_2^2 = 1.0e6, sigma 1.3e-3 a polynomial at P128 (peba1_amd.identify.probe_rounding_weight; the masked decrypt
 * test prints the phase error it sees beside it).  The weights of a masked gallery are in the MESSAGES of the ring samples, so they enter
 * none of the three terms: the product's noise grows with the probe's |p|_2^2 alone.
 *
 * What it is for (peba1_amd.identify).
 * Long templates: an entry of K w bits against K probe polynomials in probe layout, Delta = 2^-(log2(K w) + 2), the
 * addend sample and the Hamming decision's tail unchanged (pack_gallery_inner_long, hamming_probe_long,
 * match_by_inner_long).  A 2,048-bit iris code at P128 is K = 2, w = 1,024: one launch, one key switch and one bootstrap an
 * entry, where the single-term call needs two of the first two and a linear op.
 * Masked templates at num / den: the probe is, per chunk, the TWO 0/+-1 polynomials s_i m_i and m_i; the encrypted gallery
 * holds, per chunk, -den sigma_i n_i Delta and (den - 2 num) n_i Delta (notation of the public sum above).  ONE summed
 * product is D Delta, D = 2 (den disagree - num valid); the server forms Delta / 2 - D Delta (a constant alone, no addend
 * sample) and applies the constant-1/8 LUT bootstrap: TRUE iff D <= 0.  The weights are applied before the key switch,
 * whose sigma enters once -- not times sqrt(den^2 + (den - 2 num)^2) = 26.6 at 8/25 as on the two-product route
 * (masked_gallery_inner, masked_probe_tgsw, match_by_inner_masked).  2,048 bits at 8/25 are two chunks of 1,024: K = 4.
 * THE DECISION IS NOT EXACT INSIDE THE BAND: it is guaranteed only for |D| >= g (D = d - tau for a long template), g the
 * smallest integer with (g - 1/2) Delta >= 6 sigma, sigma^2 = sigma_dec^2 + the variance above at |p_t|_2^2 = N and
 * (Bg/2)^2 for E[dig^2] (peba1_amd.identify.inner_sum_decision_band, masked_inner_band).  COMPUTED at P128, not measured:
 * long 2,048-bit codes, Delta = 2^-13, K = 2: g = 185 bits of distance FOR PROBE CODES WHOSE BITS LOOK RANDOM -- the server
 * cannot see the probe; a client whose code is all 0, all 1 or has long runs has s_i of one sign and takes its band from
 * the rounding weight of its own probe (identify.hamming_probe_rounding_weight): 206 bits for an all-zero code; masked 2,048-bit codes at 8/25, Delta = 2^-18, K = 4,
 * the two mask polynomials at W = N^3 / 12: sigma before the key switch 1.9e-3, g = 6,571 in units of D, 132 disagreeing bits
 * at full validity (D moves by 2 den = 50 a bit) -- against 5,869 for the clear gallery, whose product has no rounding.
 * OUT OF SCOPE: an exact decision inside the band, probe hoisting, multi-key batching, recording these calls in the op
 * graph, libpeba1-dist, k > 1.
 *
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect (outputs untouched, results keep values and
 * slots): terms outside 1 .. tfhe_hip_ring_inner_sum_max_terms, sample_index + terms past the selector's samples, ngroups
 * outside 1 .. 65,536, a device destination that overlaps the ring words, and every refusal of tfhe_hip_ring_inner. */
#define TFHE_HIP_INNER_MAX_TERMS 8
int32_t tfhe_hip_ring_inner_sum_max_terms(const TFheGateBootstrappingParameterSet *params);
int tfhe_hip_ring_mul_tgsw_sum(const TfheHipSelector *selector, int32_t sample_index, int32_t terms, int32_t ngroups,
                               const Torus32 *ring_words, Torus32 *out_ring_words);
int tfhe_hip_ring_mul_tgsw_sum_device(const TfheHipSelector *selector, int32_t sample_index, int32_t terms, int32_t ngroups,
                                      const void *device_ring_words, void *device_out);
int tfhe_hip_ring_inner_sum(const TfheHipSelector *selector, int32_t sample_index, int32_t terms,
                            const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t M, int32_t width,
                            LweSample *result);
int tfhe_hip_ring_inner_sum_device(const TfheHipSelector *selector, int32_t sample_index, int32_t terms,
                                   const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_words, int32_t M,
                                   int32_t width, LweSample *result);
/* raw test entry: the sums of tfhe_hip_ring_mul_tgsw_sum's host form, after a flush in flight has completed */
int tfhe_hip_kernel_ring_inner_sum_product(const TfheHipSelector *selector, int32_t sample_index, int32_t terms, int32_t ngroups,
                                           const Torus32 *ring_words, Torus32 *out_words);
/* raw test entry: the extracted rows before the key switch, out_rows[i] (kN+1 words) = Extract_((i mod S) width)(the sum of
 * group i / S) for i < M, (G - 1) S < M <= G S, ring_words [G][terms][(k+1) N]; no slots involved */
int tfhe_hip_kernel_ring_inner_sum_rows(const TfheHipSelector *selector, int32_t sample_index, int32_t terms,
                                        const Torus32 *ring_words, int32_t G, int32_t M, int32_t width, Torus32 *out_rows);
/* host-logic test entry: bit 0 set if `terms` terms of gadget (l, Bgbit) at ring size N fail the MAC bound (the block the
 * kernel folds after, or the whole sum where it is shorter), bit 1 if they fail the CRT bound; -1 with the error set for N
 * outside {1024, 2048}, a gadget whose digits do not fit (Bgbit outside 1 .. 12, l Bgbit > 32) or terms outside
 * 1 .. TFHE_HIP_INNER_MAX_TERMS */
int tfhe_hip_test_inner_sum_bounds(int32_t N, int32_t l, int32_t Bgbit, int32_t terms);
/* host-logic test entry: the rows between two folds of the accumulator at ring size N (18, 16); -1 for another N */
int32_t tfhe_hip_test_inner_sum_block_rows(int32_t N);

/* ---- ring LUT bootstrap: blind-rotate an ENCRYPTED ring sample by an LWE sample under the cloud key ----
 * The ring operations above take their control input from the client (TGSW samples, ring samples).  This one takes it from
 * an LWE sample the SERVER computed -- a gate output, a tfhe_hip_linear combination, a tfhe_hip_lut_bootstrap digit -- and
 * needs no key material beyond the cloud key: the TFHE paper's other LUT form, a blind rotation whose accumulator starts
 * from an encrypted ring sample (a packed table, the result of tfhe_hip_pack_samples) in place of a public test polynomial.
 * The rotation adds the same noise whatever the accumulator starts as, so the budget is the gate bootstrap's plus the
 * table's own.  The programmable bootstrap with the noiseless table (0, v) is the special case c = (0, v).
 * Exactly, with k = 1, N = 1,024 or 2,048, c = (a, b) a ring sample of (k+1) N words and (alpha_0 .. alpha_(n-1), beta) an
 * LWE sample under the cloud key's LWE key:
 *     abar_i = round(alpha_i 2N / 2^32) mod 2N, bbar = round(beta 2N / 2^32) mod 2N
 *              -- the modulus switch of the gate path and of tfhe_hip_lut_bootstrap, ((x + 2^(31 - log2(2N))) >> (32 - log2(2N)))
 *              on the unsigned word (the oracle's orc_modswitch)
 *     ACC_0     = X^(-bbar) c                                   on both polynomials
 *     ACC_(i+1) = CMUX(BK_i, X^(abar_i) ACC_i, ACC_i)          for i = 0 .. n - 1
 *     out       = ACC_n
 * (X^(-r) c)[u][j] = c[u][(j + r) mod 2N] where that index is below N and -c[u][index - N] from N on, for every r in
 * [0, 2N): the rotation convention of the private lookup continued past N, where it negates the whole sample; X^(abar) is
 * X^(-(2N - abar)).  CMUX(G, d1, d0) = d0 + G (.) (d1 - d0) is the external product of the private selection: the same
 * offset decomposition into signed digits, the same exact negacyclic product mod 2^32, BK_i the rows of the cloud key's
 * bootstrapping key for LWE index i.  A step with abar_i = 0 is SKIPPED; computed it would leave the same words (the
 * difference is zero, the digits of the offset alone are zero).  The row of a result is Extract_0(ACC_n) in the layout of
 * the unpack (a_0 = A[0], a_i = -A[N - i], b = B[0]).
 *
 * tfhe_hip_ring_blind_rotate: ring_in holds nring ring samples, rotation j < count turns sample ring_index[j] (NULL: j) by
 * index_samples[j] -- many samples may rotate one table -- and writes ACC_n to ring_out[j (k+1) N].  ONE launch, one
 * workgroup a rotation (peba1_amd/csrc/ring_rotate.hip), the cloud key's resident image read as it rests.  The index
 * samples are LweSamples of this library; if one of them is the result of a recorded operation the recording is flushed
 * first, otherwise what is recorded stays recorded.  The call names no pool slot of its own and completes no flight.  The
 * device form (ring words resident, 16-byte aligned, the destination apart from the source) returns with the work enqueued
 * on tfhe_hip_stream().
 * tfhe_hip_ring_lut_bootstrap: out[j] = KeySwitch(Extract_0(ACC_n of rotation j)) -- rotation, extraction and the
 * planner's key switch, in chunks of at most 8,192 rows.  Like the unpack it completes a flush in flight, renames every
 * result into a fresh slot and, in immediate mode, refreshes the host mirrors; the recording is flushed only if an input
 * depends on it.  out may be `in`.  TfheHipStats has no new field: the key switches count as `keyswitches`.
 * tfhe_hip_last_ring_rotate_ms: the rotation launches of the last of these calls between two stream events (waits for the
 * second); -1 unless kernel timing is on.
 * Variance of a result's phase -- COMPUTED from the definition, not measured -- is the table sample's own plus the gate
 * bootstrap's: n CMUX terms ((k+1) l N (Bg/2)^2 bk_stdev^2 + (1 + k N) eps^2 / 3 apiece, eps = 2^-(l Bgbit + 1)), the key
 * switch's.  In front of them stands the rounding of the modulus switch, which moves the ROTATION, not the phase: each of
 * the n / 2 + 1 rounded words that count errs uniformly within half a step of 1 / 2N, sigma = sqrt((1 + n / 2) / 12)
 * coefficients (5.1 at n = 630) on top of the index sample's own noise times 2N -- a table entry must span enough
 * coefficients for that, exactly as a public LUT's sector must.
 * OUT OF SCOPE: recording these calls in the op graph, multi-key batching, libpeba1-dist, k > 1, circuit bootstrapping
 * proper (server-made TGSW samples), any change to the tuned 4- and 8-wave rotation kernels.
 *
 * Return 0, or -1 with tfhe_hip_last_error() set and the call without effect, each decided on the host before the device is
 * looked at: a null argument, count outside 1 .. 65,536, nring < 1, a ring_index outside 0 .. nring - 1 (or, ring_index
 * NULL, count > nring), a cloud key with k != 1 or N outside {1024, 2048} or a gadget outside the CMUX kernel's two bounds,
 * samples of another LWE dimension than the cloud key's or of the pool of another ciphertext shape, foreign samples,
 * device words that are not 16-byte aligned, a device destination that overlaps the ring words. */
int tfhe_hip_ring_blind_rotate(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_in, int32_t nring,
                               const int32_t *ring_index, const LweSample *index_samples, int32_t count, Torus32 *ring_out);
int tfhe_hip_ring_blind_rotate_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_in, int32_t nring,
                                      const int32_t *ring_index, const LweSample *index_samples, int32_t count,
                                      void *device_ring_out);
int tfhe_hip_ring_lut_bootstrap(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_tables, int32_t ntables,
                                const int32_t *ring_index, const LweSample *in, int32_t count, LweSample *out);
int tfhe_hip_ring_lut_bootstrap_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_tables,
                                       int32_t ntables, const int32_t *ring_index, const LweSample *in, int32_t count,
                                       LweSample *out);
double tfhe_hip_last_ring_rotate_ms(void);
/* raw test entry: the launch on caller words, after a flush in flight has completed.  ring_words [nring][(k+1) N],
 * lwe_words [count][n + 1] (rotation j by sample j), ring_index as above.  out_ring_words (or NULL) [count][(k+1) N]: ACC_n;
 * out_rows (or NULL) [count][kN + 1]: Extract_0(ACC_n) before the key switch, from a launch of its own; no slots involved */
int tfhe_hip_kernel_ring_rotate(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                                const int32_t *ring_index, const Torus32 *lwe_words, int32_t count, Torus32 *out_ring_words,
                                Torus32 *out_rows);

/* ---- seed-compressed selectors: index bits and TGSW probes travel as bodies plus one seed ----
 * Half the words of every TGSW row are a uniform public mask.  A record of `count` TGSW samples, 1 <= count <= 20, is
 * TFHE_HIP_TGSW_COMPRESSED_WORDS(k, l, N, count) = 10 + count (k+1) l N words: the mask seed (ChaCha20 key[8], nonce[2]), then
 * the bodies body[count][(k+1) l][N].  P128: one bit is 6,154 words against the 12,288 of tfhe_hip_tgsw_words; ten index bits
 * are 245,800 bytes against 491,520.  tfhe_hip_tgsw_compressed_words gives the same count from a parameter set (-1 with the
 * error set: a null set, a negative count).  The stream is the compressed cloud key's.
 * Masks.  Mask word m of the record is stream word m of the seed: word 2 (m mod 8) + 1 of ChaCha20 block floor(m / 8) under
 * (key, nonce), 64-bit block counter from 0 (tfhe_hip_test_chacha20_block).  Masks are numbered in [sample][row][u < k][j]
 * order, the bootstrapping key's: polynomial u of row r of sample b is stream words ((b (k+1) l + r) k + u) N .. + N - 1.
 * Rows.  A seeded mask cannot carry a gadget term, so every row's term is on its body, as in a compressed bootstrapping key.
 * Row (u, p), u <= k, p < l, of a sample with message polynomial m (the constant bit for a bit sample), g_p = 2^(32 - (p+1)
 * Bgbit), a_u' the row's masks, s_u' the ring key's polynomials, e gaussian of the set's bk_stdev, everything in
 * Z[X]/(X^N + 1) wrapping mod 2^32:
 *     body = sum_u' a_u' s_u' + e + g_p m            for u = k
 *     body = sum_u' a_u' s_u' + e - g_p (m s_u)      for u < k
 * The phase body - sum a s of the row is e + g_p m resp. e - g_p m s_u: that of the plain row, whose term sits on mask
 * polynomial u.  The expanded sample -- masks = the stream words verbatim, bodies = the transmitted ones, in the layout
 * [count][(k+1) l][k+1][N] -- is therefore a VALID TGSW sample of the same message and the same noise, and everything stated
 * for the private selection, the lookup and the inner products holds for it unchanged.  IT IS NOT the words
 * tfhe_hip_tgsw_encrypt_bits[_seeded] or _polys would give: there the term is on a mask polynomial, here no mask word
 * depends on the message.
 * ONE SEED PER RECORD: two records under one key must never share mask words -- the difference of two rows with equal masks
 * is the difference of their gadget terms plus noise.  Within a record distinct rows own disjoint stream words by
 * construction.  The default encryptors therefore draw ten fresh words of OS entropy for every call (and the noise from a
 * fresh OS-keyed stream), and no entry takes an offset into a stream shared between records.
 * tfhe_hip_tgsw_encrypt_bits_compressed / _polys_compressed: arguments, count limit and -- for polynomials -- the
 * coefficient contract of tfhe_hip_tgsw_encrypt_bits / _polys; out_words receives the record.  Noise draws: N gaussians per
 * row, rows in word order.  The _seeded forms (fixtures only; NOT for samples that protect data) start ONE seeded generator
 * (xoshiro256** through splitmix64) from `seed` for this record alone: its first ten `torus` draws are the seed words, the
 * noise follows from the same generator.  Host only.  0, or -1 with the error set and out_words untouched: a null argument,
 * count outside 1..20.
 * tfhe_hip_tgsw_expand_host: out_words[count][(k+1) l][k+1][N], the plain words of the record's `count` samples -- what
 * tfhe_hip_new_selector takes -- the masks drawn from one sequential stream.  Needs no key.  The reference, and the way in
 * for a caller without a GPU.  0, or -1 with the error set and out_words untouched: a null argument, count outside 1..20.
 * tfhe_hip_new_selector_compressed: a selector of the first nbits samples, 0 <= nbits <= count, of a record of `count`
 * samples; it copies the seed and nbits (k+1) l N body words and can be made and deleted on a machine without a GPU.  At its
 * first use the bodies alone are copied to the card (through the pinned staging area) and the masks are written there into
 * the staging rows the NTT transform reads: the image is word for word that of tfhe_hip_new_selector over
 * tfhe_hip_tgsw_expand_host of the same record.  Every entry that takes a selector takes it unchanged (tfhe_hip_ring_select,
 * tfhe_hip_ring_lookup, tfhe_hip_ring_inner, their device forms, the raw tfhe_hip_kernel_ring_* entries,
 * tfhe_hip_selector_bits, tfhe_hip_delete_selector).  NULL with the error set for what tfhe_hip_new_selector refuses, in its
 * words (a null set, nbits outside 0..20, a parameter set or gadget it refuses), for null words, count outside 1..20 and
 * nbits above count.
 * tfhe_hip_selector_upload_bytes: the bytes the selector's image copied to the card when it was made -- nbits (k+1) l N * 4
 * for a compressed selector, twice that (k = 1) for a plain one -- or 0 before the first use; -1 with the error set for a null
 * or deleted selector. */
#define TFHE_HIP_TGSW_COMPRESSED_WORDS(k, l, N, count) (10 + (int64_t)(count) * ((k) + 1) * (l) * (N))
int64_t tfhe_hip_tgsw_compressed_words(const TFheGateBootstrappingParameterSet *params, int32_t count);
int tfhe_hip_tgsw_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                          Torus32 *out_words);
int tfhe_hip_tgsw_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                                 Torus32 *out_words, uint64_t seed);
int tfhe_hip_tgsw_encrypt_polys_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                           Torus32 *out_words);
int tfhe_hip_tgsw_encrypt_polys_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                                  Torus32 *out_words, uint64_t seed);
int tfhe_hip_tgsw_expand_host(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words, int32_t count,
                              Torus32 *out_words);
TfheHipSelector *tfhe_hip_new_selector_compressed(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                                  int32_t count, int32_t nbits);
int64_t tfhe_hip_selector_upload_bytes(const TfheHipSelector *selector);

/* ---- kernel-level entry points (K2/K3 parity tests against the oracle) ---- */
/* exact negacyclic products res[c] = ip[c] * tp[c] mod (X^N+1) mod 2^32 through
 * the device NTT (two 27-bit primes + CRT); |ip| must be < 2^12 */
int tfhe_hip_kernel_negacyclic(const TFheGateBootstrappingCloudKeySet *bk, const int32_t *ip,
                               const Torus32 *tp, Torus32 *res, int32_t count);
/* modswitch + blind rotate + extract of `count` linear combinations lin[c]
 * (n+1 words each): u_out[c] (kN+1 words) and, if acc_out != NULL, the raw
 * accumulator ((k+1)N words) */
int tfhe_hip_kernel_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin,
                                   int32_t count, Torus32 *u_out, Torus32 *acc_out);
/* the same from caller-supplied test polynomials: combination c starts from polys[lut_index[c]] (polys: npolys x N words; an
 * index below 0: the constant test vector of the entry above).  Runs whatever kernel form the tunings select. */
int tfhe_hip_kernel_lut_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                       const int32_t *lut_index, const Torus32 *polys, int32_t npolys, Torus32 *u_out,
                                       Torus32 *acc_out);
/* the same with extract specs: combination c leaves through specs[spec_index[c]] (an index below 0: the extract at index 0;
 * lut_index as above).  specs: nspecs records of TFHE_HIP_EXTRACT_SPEC_WORDS words {nout, ntaps[4], out_c0[4], index[4][8],
 * weight[4][8]}, checked against the limits.  u_out[count][4][kN+1]: output m of combination c at [c][m] (a plain extract at
 * [c][0]), the rest untouched; on the device the outputs of all combinations lie back to back.  acc_out as above. */
#define TFHE_HIP_EXTRACT_SPEC_WORDS 73
int tfhe_hip_kernel_lut_bootstrap_multi_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                             const int32_t *lut_index, const Torus32 *polys, int32_t npolys,
                                             const int32_t *spec_index, const int32_t *specs, int32_t nspecs, Torus32 *u_out,
                                             Torus32 *acc_out);
/* key switch of `count` extracted samples u[c] (kN+1 words) -> out[c] (n+1 words) */
int tfhe_hip_kernel_keyswitch(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *u,
                              int32_t count, Torus32 *out);
/* the same rows through the matrix key switch alone, whatever their count (keys with ks_t = 8, ks_basebit = 2 and k N a
 * multiple of 256; -1 otherwise, or where the device has no room for the key's byte-plane image) */
int tfhe_hip_kernel_keyswitch_matrix(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *u,
                                     int32_t count, Torus32 *out);
/* the pack of `count` caller-supplied samples sample_words[count][n+1] (crafted operands; no slots involved) under
 * `key`, the twiddles of `bk`; idx_per_wg = mask indices per workgroup, 0 = what tfhe_hip_pack_samples uses */
int tfhe_hip_kernel_pack(const TfheHipPackingKey *key, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *sample_words,
                         int32_t count, int32_t idx_per_wg, Torus32 *out_words);
/* the extract kernel's output alone: u_out[j] (kN+1 words) = Extract_e(ring sample r) for index[j] = r N + e, arguments as
 * for tfhe_hip_unpack_samples (index = NULL: 0 .. count - 1); no key switch, no slots involved */
int tfhe_hip_kernel_ring_extract(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                                 const int32_t *index, int32_t count, Torus32 *u_out);
/* the same rows from nring seed-compressed records of 10 + N words through the seeded extract kernel */
int tfhe_hip_kernel_ring_extract_seeded(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words, int32_t nring,
                                        const int32_t *index, int32_t count, Torus32 *u_out);

#ifdef __cplusplus
}
#endif
#endif
