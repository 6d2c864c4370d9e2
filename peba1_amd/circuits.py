"""Python plumbing for libpeba1-circuits.so (include/peba1_circuits.h): the reference's
encrypted circuits and protocol function f (Math.cpp:27-417) over the boots* gate API."""
import ctypes as C
import os

import numpy as np

from . import api
from . import lib as _l

_circ = None


def load():
    global _circ
    if _circ is None:
        _l.load()   # provider of the boots* symbols first (RTLD_GLOBAL)
        if not os.path.exists(_l.CIRCUITS_PATH):
            raise RuntimeError(f"{_l.CIRCUITS_PATH} is missing: run __graft_entry__.build()")
        Lc = C.CDLL(_l.CIRCUITS_PATH)
        LS, CK = _l.LS, _l.CK
        LSP = C.POINTER(LS)
        sig = {
            "peba1_add_1bit": [LS, LS, LS, LS, CK],
            "peba1_add_nbit": [LS, LS, LS, LS, C.c_int, CK],
            "peba1_twos_complement": [LS, LS, C.c_int, CK],
            "peba1_abs": [LS, LS, C.c_int, CK],
            "peba1_sub_nbit": [LS, LS, LS, C.c_int, CK],
            "peba1_shift_left": [LS, LS, C.c_int, C.c_int, CK],
            "peba1_shift_right": [LS, LS, C.c_int, C.c_int, CK],
            "peba1_shift_left_inplace": [LS, C.c_int, C.c_int, CK],
            "peba1_multiply": [LS, LS, LS, C.c_int, CK],
            "peba1_compare_bit": [LS, LS, LS, LS, LS, CK],
            "peba1_minimum": [LS, LS, LS, LS, C.c_int, CK],
            "peba1_euclidean_distance": [LS, LSP, LSP, C.c_int, C.c_int, CK],
            "peba1_function_f": [LS, LSP, LSP, C.c_int, LS, C.c_int, CK],
            "peba1_function_g": [LS, LS, LS, LS, C.c_int, CK],
            "peba1_euclidean_distance_fast": [LS, LSP, LSP, C.c_int, C.c_int, CK],
            "peba1_function_f_fast": [LS, LSP, LSP, C.c_int, LS, C.c_int, CK],
            "peba1_partial_distance": [LS, LSP, LSP, C.c_int, C.c_int, CK],
            "peba1_combine_and_compare": [LS, LSP, C.c_int, LS, CK],
            "peba1_combine_and_compare_fast": [LS, LSP, C.c_int, LS, CK],
            "peba1_hamming_distance": [LS, LS, LS, C.c_int, CK],
            "peba1_hamming_match": [LS, LS, LS, C.c_int, LS, CK],
            "peba1_function_f_fast3": [LS, LSP, LSP, C.c_int, LS, C.c_int, CK],
            "peba1_hamming_distance_csa": [LS, LS, LS, C.c_int, CK],
            "peba1_hamming_match_csa": [LS, LS, LS, C.c_int, LS, CK],
        }
        for name, args in sig.items():
            f = getattr(Lc, name)
            f.restype = None
            f.argtypes = args
        Lc.peba1_function_f_batch.restype = C.c_int
        Lc.peba1_function_f_batch.argtypes = [LSP, C.POINTER(LSP), C.POINTER(LSP), C.c_int, C.c_int, LSP, C.c_int,
                                              C.POINTER(CK), C.c_int]
        Lc.peba1_hamming_match_batch.restype = C.c_int
        Lc.peba1_hamming_match_batch.argtypes = [LSP, LSP, LSP, C.c_int, C.c_int, LSP, C.POINTER(CK)]
        Lc.peba1_hamming_match_csa_batch.restype = C.c_int
        Lc.peba1_hamming_match_csa_batch.argtypes = Lc.peba1_hamming_match_batch.argtypes
        Lc.peba1_hamming_count_bits.restype = C.c_int
        Lc.peba1_hamming_count_bits.argtypes = [C.c_int]
        _circ = Lc
    return _circ


def _ptr_array(arrays):
    arr = (_l.LS * len(arrays))()
    for i, a in enumerate(arrays):
        arr[i] = a.ptr
    return arr


class EncryptedVector:
    """A template / sample: nslots features of `bitsize` bits, one LweSample array per slot
    (the reference's std::vector<LweSample*>, main.cpp:53-70)."""

    def __init__(self, params, values, bitsize, key):
        self.slots = []
        for v in values:
            a = api.CiphertextArray(params, bitsize)
            a.encrypt([(int(v) >> j) & 1 for j in range(bitsize)], key)
            self.slots.append(a)

    def to_device(self):
        for a in self.slots:
            a.set_words(a.words())
        return self

    @classmethod
    def from_ring(cls, params, words, nslots, bitsize, key):
        """The server side of ring_encrypt_vector: the nslots arrays of `bitsize` samples of a template that arrived as ONE
        ring sample of (k+1) N words, through a single scattered unpack (api.unpack).  Bit j of slot s is coefficient
        s * bitsize + j.  key: the keyset whose cloud key evaluates."""
        if nslots * bitsize > params.N:
            raise ValueError("a ring sample of this parameter set carries %d bits" % params.N)
        self = cls.__new__(cls)
        self.slots = [api.CiphertextArray(params, bitsize) for _ in range(nslots)]
        # a seed-compressed record (10 + N words: ring_encrypt_vector(compressed=True)) is told from a plain sample by its size
        seeded = np.asarray(words).size == 10 + params.N
        (api.unpack_seeded if seeded else api.unpack)(words, key, [a.at(j) for a in self.slots for j in range(bitsize)],
                                                      count=nslots * bitsize)
        return self

    @classmethod
    def from_seeded_lwe(cls, params, words, nslots, bitsize):
        """The server side of seeded_lwe_encrypt_vector: the nslots arrays of `bitsize` samples of a template that arrived
        as ONE seed-compressed LWE record of 10 + nslots * bitsize words, through a single scattered seeded import
        (api.import_seeded).  Bit j of slot s is sample s * bitsize + j.  Needs no key: the samples are fresh encryptions."""
        if np.asarray(words).size != 10 + nslots * bitsize:
            raise ValueError("a record of %d samples has %d words" % (nslots * bitsize, 10 + nslots * bitsize))
        self = cls.__new__(cls)
        self.slots = [api.CiphertextArray(params, bitsize) for _ in range(nslots)]
        api.import_seeded(words, params, [a.at(j) for a in self.slots for j in range(bitsize)])
        return self


def seeded_lwe_encrypt_vector(values, bitsize, key, seed=None, mask_seed=None):
    """The client side of EncryptedVector.from_seeded_lwe: len(values) features of `bitsize` bits as ONE seed-compressed
    record of fresh LWE samples under the secret keyset `key` -- bit j of value s is sample s * bitsize + j (4,136 bytes for
    128 x 8 bits, where the samples of an EncryptedVector are 2.5 MB at P128)."""
    bits = [(int(v) >> j) & 1 for v in values for j in range(bitsize)]
    return api.encrypt_bits_compressed(bits, key, seed=seed, mask_seed=mask_seed)


def ring_encrypt_vector(values, bitsize, key, seed=None, compressed=False, mask_seed=None):
    """The client side of EncryptedVector.from_ring: len(values) features of `bitsize` bits as ONE ring sample under the
    secret keyset `key` -- bit j of value s at coefficient s * bitsize + j (8 KB for 128 x 8 bits at N = 1,024, where the
    samples of an EncryptedVector are 2.5 MB).  compressed: as a seed-compressed sample, 10 + N words (4,136 bytes)."""
    bits = [(int(v) >> j) & 1 for v in values for j in range(bitsize)]
    return api.ring_encrypt_bits(bits, key, seed=seed, compressed=compressed, mask_seed=mask_seed)


def encrypt_number(params, value, bits, key):
    a = api.CiphertextArray(params, bits)
    return a.encrypt([(int(value) >> j) & 1 for j in range(bits)], key)


def decrypt_number(arr, key, bits=None):
    d = arr.decrypt(key)
    bits = len(d) if bits is None else bits
    return sum(int(d[i]) << i for i in range(bits))


def function_f(result_b, sample, template, bound, bitsize, key):
    """Function_f(result_b, a=sample, b=template, bound, bitsize, cloud_key), Math.cpp:379."""
    load().peba1_function_f(result_b.ptr, _ptr_array(sample.slots), _ptr_array(template.slots), len(sample.slots),
                            bound.ptr, bitsize, key.cloud)


def function_f_fast(result_b, sample, template, bound, bitsize, key):
    """Same result as function_f through the optimised DAG of circuits_fast.cpp (not the
    reference's gate sequence; about 8x fewer bootstraps, 5x less depth)."""
    load().peba1_function_f_fast(result_b.ptr, _ptr_array(sample.slots), _ptr_array(template.slots),
                                 len(sample.slots), bound.ptr, bitsize, key.cloud)


def function_f_fast3(result_b, sample, template, bound, bitsize, key):
    """function_f_fast's DAG with its full adders as XOR3 + MAJ3 (tfhe_hip_gate3: 2 bootstraps at depth 1 each)."""
    load().peba1_function_f_fast3(result_b.ptr, _ptr_array(sample.slots), _ptr_array(template.slots),
                                  len(sample.slots), bound.ptr, bitsize, key.cloud)


def euclidean_distance_fast(result, sample, template, bitsize, key):
    load().peba1_euclidean_distance_fast(result.ptr, _ptr_array(sample.slots), _ptr_array(template.slots),
                                         len(sample.slots), bitsize, key.cloud)


def function_g(result, result_b, r0, r1, bitsize, key):
    """Function_g(result, result_b, r0, r1, bitsize, cloud_key), Math.cpp:390: (1-b)*r0 + b*r1 on
    `bitsize`-sample numbers (the reference's heap overflow, SURVEY D4, fixed)."""
    load().peba1_function_g(result.ptr, result_b.ptr, r0.ptr, r1.ptr, bitsize, key.cloud)


def euclidean_distance(result, sample, template, bitsize, key):
    load().peba1_euclidean_distance(result.ptr, _ptr_array(sample.slots), _ptr_array(template.slots),
                                    len(sample.slots), bitsize, key.cloud)


def partial_distance(partial, sample_slots, template_slots, bitsize, key):
    load().peba1_partial_distance(partial.ptr, _ptr_array(sample_slots), _ptr_array(template_slots),
                                  len(sample_slots), bitsize, key.cloud)


def combine_and_compare(result_b, partials, bound, key):
    load().peba1_combine_and_compare(result_b.ptr, _ptr_array(partials), len(partials), bound.ptr, key.cloud)


def hamming_match(result_b, a, b, nbits, bound, key):
    """result_b[0] = (popcount(a XOR b) > bound); a, b: CiphertextArray of nbits samples."""
    load().peba1_hamming_match(result_b.ptr, a.ptr, b.ptr, nbits, bound.ptr, key.cloud)


def hamming_distance(count, a, b, nbits, key):
    load().peba1_hamming_distance(count.ptr, a.ptr, b.ptr, nbits, key.cloud)


def hamming_match_csa(result_b, a, b, nbits, bound, key):
    """hamming_match through a carry-save compressor of three-input full adders: same result, a quarter of the
    bootstraps."""
    load().peba1_hamming_match_csa(result_b.ptr, a.ptr, b.ptr, nbits, bound.ptr, key.cloud)


def hamming_distance_csa(count, a, b, nbits, key):
    load().peba1_hamming_distance_csa(count.ptr, a.ptr, b.ptr, nbits, key.cloud)


def hamming_count_bits(nbits):
    return load().peba1_hamming_count_bits(nbits)


def _cloud_array(keys):
    arr = (_l.CK * len(keys))()
    for i, k in enumerate(keys):
        arr[i] = k.cloud
    return arr


def function_f_batch(results_b, samples, templates, bounds, bitsize, keys, fast=False):
    """Function_f for K clients in ONE flush, client c under its own key keys[c] (peba1_function_f_batch: multi-key
    flushes, include/tfhe_hip.h "batch_keys").  Lists of K each; returns the flush's level count.  fast: False, True
    (function_f_fast's DAG) or 2 (function_f_fast3's)."""
    k = len(keys)
    assert len(results_b) == len(samples) == len(templates) == len(bounds) == k
    nslots = len(samples[0].slots)
    assert all(len(s.slots) == nslots and len(t.slots) == nslots for s, t in zip(samples, templates))
    sa = [_ptr_array(s.slots) for s in samples]
    ta = [_ptr_array(t.slots) for t in templates]
    LSP = C.POINTER(_l.LS)
    sp, tp = (LSP * k)(*[C.cast(x, LSP) for x in sa]), (LSP * k)(*[C.cast(x, LSP) for x in ta])
    rc = load().peba1_function_f_batch(_ptr_array(results_b), sp, tp, k, nslots, _ptr_array(bounds), bitsize,
                                       _cloud_array(keys), 2 if fast == 2 else 1 if fast else 0)
    if rc < 0:
        raise RuntimeError(api.last_error())
    return rc


def hamming_match_batch(results_b, a, b, nbits, bounds, keys, csa=False):
    """peba1_hamming_match (csa: peba1_hamming_match_csa) for K clients in ONE flush, client c under keys[c]; returns
    the flush's level count."""
    k = len(keys)
    assert len(results_b) == len(a) == len(b) == len(bounds) == k
    entry = load().peba1_hamming_match_csa_batch if csa else load().peba1_hamming_match_batch
    rc = entry(_ptr_array(results_b), _ptr_array(a), _ptr_array(b), k, nbits,
                                          _ptr_array(bounds), _cloud_array(keys))
    if rc < 0:
        raise RuntimeError(api.last_error())
    return rc


# ---- tree LUT: a function of two small digits by S + 1 rotations and one pack (include/tfhe_hip.h "ring LUT bootstrap") ----
def digit_phase(m, S):
    """The torus word of digit m < S: phase (m + 1/2) / (2 S), the centre of block m on the negacyclic half torus."""
    return ((2 * int(m) + 1) << 32) // (4 * S)


def tree_lut_variance(params, pk_t=None, pk_basebit=None):
    """COMPUTED variance (torus units) of a tree_lut result's phase: a block value carries one gate bootstrap's output
    variance V (rotation and key switch, the typical-case formula of the noise tests: digits uniform, E[dig^2] = Bg^2 / 12)
    and the packing key switch's first-order variance for the N samples of one pack (the header's: n t N E[d^2] bk_stdev^2 +
    (n / 2) prec^2 / 3); the rotation by x_hi and its key switch add V again: 2 V + pack.  It does not depend on S: the N / S copies of an entry are the SAME sample, so a block is
    constant, noise included."""
    tg = params.ptr.contents.tgsw_params.contents
    ks_stdev, bk = params.ptr.contents.in_out_params.contents.alpha_min, tg.tlwe_params.contents.alpha_min
    n, N, k, l, Bg = params.n, params.N, params.k, params.l, float(1 << params.Bgbit)
    eps, delta = 2.0 ** -(l * params.Bgbit + 1), 2.0 ** -(params.ks_t * params.ks_basebit + 1)
    rot = n * (k + 1) * l * N * (Bg ** 2 / 12) * bk ** 2 + n * (1 + k * N / 2) * eps ** 2 / 3 + (n / 2) * (N * eps) ** 2 / 12
    ks = k * N * params.ks_t * (1 - 2.0 ** -params.ks_basebit) * ks_stdev ** 2 + k * N / 2 * delta ** 2 / 3
    t, bb = params.ks_t if pk_t is None else pk_t, params.ks_basebit if pk_basebit is None else pk_basebit
    base = 2 ** bb
    pack = n * t * N * ((base - 1) * (2 * base - 1) / 6.0) * bk ** 2 + (n / 2.0) * (2.0 ** -(1 + bb * t)) ** 2 / 3.0
    return 2 * (rot + ks) + pack


def tree_lut(tables, x_hi, x_lo, key, pkey, result=None):
    """result[i] = tables[hi_i][lo_i] for digits hi_i, lo_i < S carried by the samples x_hi[i], x_lo[i] at digit_phase(m, S)
    (CiphertextArrays of equal count); `tables` is an S x S integer table of 2-bit output digits v, returned at phase
    (2 v + 1) / 16.  S a power of two, 2 <= S <= 8.
      1. S LUT bootstraps of x_lo against the PUBLIC test polynomials of the rows: row h gives tables[h][lo]
         (api.lut_bootstrap_batch, recorded into one level);
      2. per i, api.pack of N samples -- N / S COPIES (bootsCOPY: handles, no arithmetic) of each of the S results, so that
         entry h fills the block of N / S equal coefficients from h N / S -- into ONE ring sample under the packing key `pkey`;
      3. api.ring_lut_bootstrap of the packed samples by x_hi: the block of hi, extracted and key-switched.
    S + 1 rotations and one pack per pair of digits.  Noise: tree_lut_variance -- a block is constant (the copies are one
    sample), each value carrying its bootstrap's variance and the pack's; sigma 4.9e-3 at P128, six of them 0.029 against the half sector 1/16.
    The other way to fill a block -- packing each result once and multiplying by the public polynomial 1 + X + .. +
    X^(N/S - 1) -- is NOT built: it needs the results N / S coefficients apart, which a pack of consecutive samples does not
    give, and it multiplies the results' noise by sqrt(N / S) = 16 at S = 4 (sigma 0.056, six of them far past the half sector)."""
    params = key.params
    N, S = params.N, len(tables)
    if S < 2 or S > 8 or S & (S - 1) or any(len(row) != S for row in tables):
        raise ValueError("tables is an S x S table, S a power of two in 2..8")
    if any(not 0 <= int(v) < 4 for row in tables for v in row):
        raise ValueError("the output digits are 2-bit values")
    count = x_lo.count
    if x_hi.count != count:
        raise ValueError("x_hi and x_lo hold one digit each per lookup")
    result = api.CiphertextArray(params, count) if result is None else result
    L = _l.load()
    luts = [api.Lut(params, np.array([(2 * int(row[j * S // N]) + 1) << 28 for j in range(N)], dtype=np.int64).astype(np.int32))
            for row in tables]
    rows = [api.CiphertextArray(params, count) for _ in range(S)]
    block = api.CiphertextArray(params, N)
    was = api.get_deferred()
    api.set_deferred(True)
    try:
        for lut, row in zip(luts, rows):
            api.lut_bootstrap_batch(lut, row, [x_lo], [1], 0, key)
        packed = np.zeros((count, (params.k + 1) * N), dtype=np.int32)
        for i in range(count):
            for j in range(N):
                L.bootsCOPY(block.at(j), rows[j * S // N].at(i), key.cloud)
            packed[i] = api.pack(pkey, block, N, key)                     # (its flush runs the S bootstraps at i = 0)
        api.ring_lut_bootstrap(packed, x_hi, key, result, count=count)
    finally:
        api.set_deferred(was)
        for o in luts + rows + [block]:
            o.close()
    return result
