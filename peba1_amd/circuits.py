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
