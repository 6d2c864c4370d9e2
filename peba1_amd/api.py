"""Thin Python mirror of the tfhe gate API as served by libtfhe-hip.so.

Names follow the reference's vocabulary (parameter set, secret/cloud keyset,
LweSample arrays, boots* gates; /root/reference/src/Math.cpp, src/main.cpp).
Everything here is plumbing over the C ABI; the arithmetic is in the HIP kernels.
"""
import ctypes as C

import numpy as np

from . import lib as _l

GATE_CODES = {"NAND": 0, "OR": 1, "AND": 2, "NOR": 3, "XOR": 4, "XNOR": 5,
              "ANDNY": 6, "ANDYN": 7, "ORNY": 8, "ORYN": 9}
# three-input gates (tfhe_hip_gate3; not in upstream's API): t = s (+-A +- B +- C) with s = GATE3_LIN[name]
GATE3_CODES = {"MAJ3": 0, "XOR3": 1, "XNOR3": 2}
GATE3_LIN = {"MAJ3": 1, "XOR3": -2, "XNOR3": 2}


def _i32p(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_l.I32P)


def last_error():
    return _l.load().tfhe_hip_last_error().decode()


class _CFile:
    """A C FILE* for the tfhe_io.h entry points."""
    _libc = None

    def __init__(self, path, mode):
        if _CFile._libc is None:
            libc = C.CDLL(None)
            libc.fopen.restype = C.c_void_p
            libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
            libc.fclose.argtypes = [C.c_void_p]
            _CFile._libc = libc
        self.fp = _CFile._libc.fopen(str(path).encode(), mode.encode())
        if not self.fp:
            raise OSError("cannot open %s" % path)

    def __enter__(self):
        return self.fp

    def __exit__(self, *exc):
        _CFile._libc.fclose(self.fp)
        self.fp = None


class ParameterSet:
    """new_default_gate_bootstrapping_parameters (main.cpp:21) or an explicit tuple."""

    def __init__(self, minimum_lambda=128, custom=None, p2048=False, _ptr=None):
        L = _l.load()
        if _ptr is not None:
            self.ptr = _ptr
        elif custom is not None:
            self.ptr = L.tfhe_hip_new_parameters(*custom)
        elif p2048:
            self.ptr = L.tfhe_hip_new_p2048_parameters()
        else:
            self.ptr = L.new_default_gate_bootstrapping_parameters(minimum_lambda)
        if not self.ptr:
            raise ValueError("parameter set rejected: " + last_error())
        self.n = self.ptr.contents.in_out_params.contents.n
        tg = self.ptr.contents.tgsw_params.contents
        self.N = tg.tlwe_params.contents.N
        self.k = tg.tlwe_params.contents.k
        self.l, self.Bgbit = tg.l, tg.Bgbit
        self.ks_t, self.ks_basebit = self.ptr.contents.ks_t, self.ptr.contents.ks_basebit
        self.words = self.n + 1

    def save(self, path):
        with _CFile(path, "wb") as fp:
            _l.load().export_tfheGateBootstrappingParameterSet_toFile(fp, self.ptr)

    @classmethod
    def load(cls, path):
        with _CFile(path, "rb") as fp:
            ptr = _l.load().new_tfheGateBootstrappingParameterSet_fromFile(fp)
        if not ptr:
            raise ValueError("cannot load a parameter set from %s: %s" % (path, last_error()))
        return cls(_ptr=ptr)


class SecretKeySet:
    """new_random_gate_bootstrapping_secret_keyset (main.cpp:22) with an explicit seed."""

    def __init__(self, params, seed, device=True, _ptr=None):
        L = _l.load()
        self.params = params
        if _ptr is not None:
            self.ptr = _ptr
        else:
            f = L.tfhe_hip_new_secret_keyset_seeded if device else L.tfhe_hip_new_secret_keyset_seeded_host
            self.ptr = f(params.ptr, seed)
        if not self.ptr:
            raise RuntimeError("keygen failed: " + last_error())
        self.cloud = C.pointer(self.ptr.contents.cloud)   # &key->cloud, main.cpp:23

    def save(self, path):
        """export_tfheGateBootstrappingSecretKeySet_toFile (tfhe_io.h)."""
        with _CFile(path, "wb") as fp:
            _l.load().export_tfheGateBootstrappingSecretKeySet_toFile(fp, self.ptr)

    def save_cloud(self, path):
        """export_tfheGateBootstrappingCloudKeySet_toFile of &key->cloud: what the server gets."""
        with _CFile(path, "wb") as fp:
            _l.load().export_tfheGateBootstrappingCloudKeySet_toFile(fp, self.cloud)

    @classmethod
    def load(cls, path):
        with _CFile(path, "rb") as fp:
            ptr = _l.load().new_tfheGateBootstrappingSecretKeySet_fromFile(fp)
        if not ptr:
            raise ValueError("cannot load a secret keyset from %s: %s" % (path, last_error()))
        return cls(ParameterSet(_ptr=C.cast(ptr.contents.params, _l.PS)), None, _ptr=ptr)

    def close(self):
        if self.ptr:
            _l.load().delete_gate_bootstrapping_secret_keyset(self.ptr)
            self.ptr = None

    def _arr(self, f, owner):
        cnt = C.c_int64()
        p = f(owner, C.byref(cnt))
        return np.ctypeslib.as_array(p, shape=(cnt.value,))

    def lwe_key(self):
        return self._arr(_l.load().tfhe_hip_key_lwe, self.ptr)

    def tlwe_key(self):
        return self._arr(_l.load().tfhe_hip_key_tlwe, self.ptr)

    def bk(self):
        return self._arr(_l.load().tfhe_hip_key_bk, self.cloud)

    def ksk(self):
        return self._arr(_l.load().tfhe_hip_key_ksk, self.cloud)


class CloudKeySet(SecretKeySet):
    """A cloud keyset on its own (new_tfheGateBootstrappingCloudKeySet_fromFile): evaluates
    gates, cannot encrypt or decrypt."""

    def __init__(self, ptr):
        self.ptr = None
        self.cloud = ptr
        self.params = ParameterSet(_ptr=C.cast(ptr.contents.params, _l.PS))

    @classmethod
    def load(cls, path):
        with _CFile(path, "rb") as fp:
            ptr = _l.load().new_tfheGateBootstrappingCloudKeySet_fromFile(fp)
        if not ptr:
            raise ValueError("cannot load a cloud keyset from %s: %s" % (path, last_error()))
        return cls(ptr)

    def save(self, path):
        with _CFile(path, "wb") as fp:
            _l.load().export_tfheGateBootstrappingCloudKeySet_toFile(fp, self.cloud)

    save_cloud = save

    def close(self):
        if self.cloud:
            _l.load().delete_gate_bootstrapping_cloud_keyset(self.cloud)
            self.cloud = None

    def lwe_key(self):
        raise TypeError("a cloud keyset holds no secret key")

    tlwe_key = lwe_key


class CompressedCloudKey:
    """A seed-compressed cloud key (include/tfhe_hip.h): a 40-byte mask seed and the bodies -- what a client sends in place
    of a cloud-key file.  expand() gives a cloud keyset whose masks are made on the device at its first use, expand_host()
    one expanded on the CPU; both are CloudKeySets (close() them)."""

    def __init__(self, ptr, params):
        if not ptr:
            raise RuntimeError("compressed cloud key refused: " + last_error())
        self.ptr, self.params = ptr, params

    @classmethod
    def generate(cls, secret):
        return cls(_l.load().tfhe_hip_new_compressed_cloud_key(secret.ptr), secret.params)

    @classmethod
    def generate_seeded(cls, secret, noise_seed, mask_seed):
        seed = np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10)
        return cls(_l.load().tfhe_hip_new_compressed_cloud_key_seeded(secret.ptr, noise_seed, seed.ctypes.data_as(_l.U32P)),
                   secret.params)

    @classmethod
    def from_words(cls, params, mask_seed, bk_body, ksk_body):
        seed = np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10)
        base = (1 << params.ks_basebit) - 1
        bk = np.ascontiguousarray(bk_body, dtype=np.int32).reshape(params.n * (params.k + 1) * params.l * params.N)
        ksk = np.ascontiguousarray(ksk_body, dtype=np.int32).reshape(params.k * params.N * params.ks_t * base)
        return cls(_l.load().tfhe_hip_new_compressed_cloud_key_from_words(params.ptr, seed.ctypes.data_as(_l.U32P), _i32p(bk),
                                                                          _i32p(ksk)), params)

    def seed(self):
        return np.ctypeslib.as_array(_l.load().tfhe_hip_compressed_key_seed(self.ptr), shape=(10,)).copy()

    def _body(self, f):
        cnt = C.c_int64()
        p = f(self.ptr, C.byref(cnt))
        return np.ctypeslib.as_array(p, shape=(cnt.value,))

    def bk_body(self):
        """int32 [n (k+1)l N]: a view of the key's words (valid until close())"""
        return self._body(_l.load().tfhe_hip_compressed_key_bk_body)

    def ksk_body(self):
        """int32 [kN t (base-1)]: likewise"""
        return self._body(_l.load().tfhe_hip_compressed_key_ksk_body)

    @property
    def nbytes(self):
        """the bytes that travel: the seed and both body arrays"""
        return int(_l.load().tfhe_hip_compressed_key_bytes(self.ptr))

    def expand(self):
        ptr = _l.load().tfhe_hip_expand_cloud_key(self.ptr)
        if not ptr:
            raise RuntimeError("expand failed: " + last_error())
        return CloudKeySet(ptr)

    def expand_host(self):
        ptr = _l.load().tfhe_hip_expand_cloud_key_host(self.ptr)
        if not ptr:
            raise RuntimeError("expand_host failed: " + last_error())
        return CloudKeySet(ptr)

    def save(self, path):
        with _CFile(path, "wb") as fp:
            _l.load().tfhe_hip_export_compressed_cloud_key_toFile(fp, self.ptr)

    @classmethod
    def load(cls, path):
        with _CFile(path, "rb") as fp:
            ptr = _l.load().tfhe_hip_new_compressed_cloud_key_fromFile(fp)
        if not ptr:
            raise ValueError("cannot load a compressed cloud key from %s: %s" % (path, last_error()))
        return cls(ptr, None)       # (the parameter set is in the file: expand().params has it)

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_compressed_cloud_key(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kernel_expand_masks(mask_seed, first_word, count):
    """stream words first_word .. first_word + count - 1 from the device kernels' block function (uint32 [count])"""
    seed = np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10)
    out = np.zeros(count, dtype=np.uint32)
    rc = _l.load().tfhe_hip_kernel_expand_masks(seed.ctypes.data_as(_l.U32P), first_word, count, out.ctypes.data_as(_l.U32P))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def key_image(key, which):
    """the device BK image (which = 0) or the compact KSK with padding and zero row (which = 1) of a keyset, int32"""
    L = _l.load()
    L.tfhe_hip_clear_error()
    words = L.tfhe_hip_test_key_image(key.cloud, which, None, 0)
    if words < 0:
        raise RuntimeError(last_error())
    out = np.zeros(words, dtype=np.int32)
    if L.tfhe_hip_test_key_image(key.cloud, which, _i32p(out), words) != words:
        raise RuntimeError(last_error())
    return out


def ks_matrix_stats():
    """ks_matrix_launches (tfhe_hip_get_ks_matrix_stats)"""
    s = _l.KsMatrixStats()
    _l.load().tfhe_hip_get_ks_matrix_stats(C.byref(s))
    return {"ks_matrix_launches": s.ks_matrix_launches}


def expand_stats():
    """expanded_keys, expand_launches (tfhe_hip_get_expand_stats)"""
    s = _l.ExpandStats()
    _l.load().tfhe_hip_get_expand_stats(C.byref(s))
    return {f: getattr(s, f) for f in _l.EXPAND_STATS_FIELDS}


class CiphertextArray:
    """new_gate_bootstrapping_ciphertext_array / delete_... (Math.cpp:28-30,47-49)."""

    def __init__(self, params, count):
        self.params, self.count = params, count
        self.ptr = _l.load().new_gate_bootstrapping_ciphertext_array(count, params.ptr)

    def close(self):
        if self.ptr:
            _l.load().delete_gate_bootstrapping_ciphertext_array(self.count, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def at(self, i):
        return C.cast(C.addressof(self.ptr.contents) + i * C.sizeof(_l.LweSample), _l.LS)

    def encrypt(self, bits, key):
        L = _l.load()
        for i, b in enumerate(bits):
            L.bootsSymEncrypt(self.at(i), int(b), key.ptr)
        return self

    def decrypt(self, key):
        L = _l.load()
        return np.array([L.bootsSymDecrypt(self.at(i), key.ptr) for i in range(self.count)], dtype=np.int32)

    def save(self, path):
        """count x export_gate_bootstrapping_ciphertext_toFile into one file."""
        L = _l.load()
        with _CFile(path, "wb") as fp:
            for i in range(self.count):
                L.export_gate_bootstrapping_ciphertext_toFile(fp, self.at(i), self.params.ptr)

    def load(self, path):
        L = _l.load()
        with _CFile(path, "rb") as fp:
            for i in range(self.count):
                L.tfhe_hip_clear_error()
                L.import_gate_bootstrapping_ciphertext_fromFile(fp, self.at(i), self.params.ptr)
                if last_error():
                    raise ValueError("cannot load ciphertext %d from %s: %s" % (i, path, last_error()))
        return self

    def words(self):
        out = np.zeros((self.count, self.params.words), dtype=np.int32)
        rc = _l.load().tfhe_hip_export_samples(self.ptr, self.count, self.params.ptr, _i32p(out))
        if rc != 0:
            raise RuntimeError(last_error())
        return out

    def set_words(self, w):
        w = np.ascontiguousarray(w, dtype=np.int32).reshape(self.count, self.params.words)
        rc = _l.load().tfhe_hip_import_samples(self.ptr, self.count, self.params.ptr, _i32p(w))
        if rc != 0:
            raise RuntimeError(last_error())
        return self


def gate_batch(name, result, a, b, key):
    rc = _l.load().tfhe_hip_gate_batch(GATE_CODES[name], result.ptr, a.ptr, b.ptr, result.count, key.cloud)
    if rc != 0:
        raise RuntimeError(last_error())


def gate3(name, result, a, b, c, key, negate_mask=0):
    """result = name(a, b, c), each an LweSample pointer (CiphertextArray.at); bit i of negate_mask negates operand i.
    Errors go to last_error() and leave the result untouched, as for the boots* entries."""
    _l.load().tfhe_hip_gate3(GATE3_CODES[name], int(negate_mask), result, a, b, c, key.cloud)


def gate3_batch(name, result, a, b, c, key, negate_mask=0):
    rc = _l.load().tfhe_hip_gate3_batch(GATE3_CODES[name], int(negate_mask), result.ptr, a.ptr, b.ptr, c.ptr, result.count,
                                        key.cloud)
    if rc != 0:
        raise RuntimeError(last_error())


class Lut:
    """A caller-supplied test polynomial (tfhe_hip_new_lut): N torus words bound to a parameter set.  The bootstrap of a
    phase p (in 1/2N-ths of the torus) returns v[p] below N and -v[p - N] from N on; the words are defined in
    include/tfhe_hip.h."""

    def __init__(self, params, words):
        w = np.ascontiguousarray(words, dtype=np.int32)
        if w.shape != (params.N,):
            raise ValueError("a LUT of this parameter set holds %d words" % params.N)
        self._take(params, _l.load().tfhe_hip_new_lut(params.ptr, _i32p(w)))

    def _take(self, params, ptr):
        self.params, self.ptr = params, ptr
        if not ptr:
            raise ValueError("LUT rejected: " + last_error())

    @classmethod
    def constant(cls, params, mu):
        """v[j] = mu: upstream's tfhe_bootstrap test vector; mu = 2^29 is the one every gate uses."""
        self = cls.__new__(cls)
        self._take(params, _l.load().tfhe_hip_new_lut_constant(params.ptr, int(mu)))
        return self

    @classmethod
    def from_table(cls, params, values):
        """v[j] = values[j * len(values) / N]; len(values) must divide N."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        self = cls.__new__(cls)
        self._take(params, _l.load().tfhe_hip_new_lut_from_table(params.ptr, _i32p(v), len(v)))
        return self

    def words(self):
        cnt = C.c_int32()
        p = _l.load().tfhe_hip_lut_words(self.ptr, C.byref(cnt))
        return np.ctypeslib.as_array(p, shape=(cnt.value,)).copy()

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_lut(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lut_bootstrap(lut, result, inputs, coefs, c0, key):
    """result = LUT bootstrap of (0, c0) + sum coefs[i] inputs[i]; result and inputs are LweSample pointers
    (CiphertextArray.at), one to three inputs.  Errors go to last_error() and leave the result untouched."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*inputs)
    cf = np.ascontiguousarray(coefs, dtype=np.int32)
    assert len(cf) == n
    _l.load().tfhe_hip_lut_bootstrap(lut.ptr if lut is not None else None, result, n, ins, _i32p(cf), int(c0), key.cloud)


def lut_bootstrap_batch(lut, result, inputs, coefs, c0, key):
    """result[i] = LUT bootstrap of (0, c0) + sum coefs[k] inputs[k][i]: CiphertextArrays of result.count samples."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*[a.ptr for a in inputs])
    cf = np.ascontiguousarray(coefs, dtype=np.int32)
    assert len(cf) == n
    rc = _l.load().tfhe_hip_lut_bootstrap_batch(lut.ptr if lut is not None else None, result.ptr, n, ins, _i32p(cf), int(c0),
                                                result.count, key.cloud)
    if rc != 0:
        raise RuntimeError(last_error())


class LutMulti:
    """A test polynomial with an extract spec (tfhe_hip_new_lut_multi): one blind rotation, several outputs.  `outputs` is
    a list of (taps, out_c0) with taps = [(index, weight), ...]; output m is (0, out_c0) + sum weight * Extract_index(ACC),
    key-switched -- the integers are in include/tfhe_hip.h."""

    def __init__(self, lut, outputs):
        ntaps = np.array([len(t) for t, _ in outputs], dtype=np.int32)
        idx = np.array([i for t, _ in outputs for i, _ in t] or [0], dtype=np.int32)
        wgt = np.array([w for t, _ in outputs for _, w in t] or [0], dtype=np.int32)
        c0 = np.array([_wrap32(c) for _, c in outputs] or [0], dtype=np.int32)
        self._take(lut.params, _l.load().tfhe_hip_new_lut_multi(lut.ptr, len(outputs), _i32p(ntaps), _i32p(idx), _i32p(wgt),
                                                               _i32p(c0)))

    def _take(self, params, ptr):
        self.params, self.ptr = params, ptr
        if not ptr:
            raise ValueError("multi-output LUT rejected: " + last_error())

    @classmethod
    def from_tables(cls, params, step, levels):
        """For an input phase in sector s of the half torus (len(levels[m]) sectors) output m has phase step * levels[m][s]."""
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        assert lv.ndim == 2
        self = cls.__new__(cls)
        self._take(params, _l.load().tfhe_hip_new_lut_multi_from_tables(params.ptr, _wrap32(step), lv.shape[1], lv.shape[0],
                                                                        _i32p(lv)))
        return self

    @property
    def nout(self):
        return _l.load().tfhe_hip_lut_multi_nout(self.ptr)

    def outputs(self):
        """[(taps, out_c0)] as the object holds them."""
        out = []
        for m in range(self.nout):
            idx, wgt, c0 = np.zeros(8, np.int32), np.zeros(8, np.int32), C.c_int32()
            n = _l.load().tfhe_hip_lut_multi_output(self.ptr, m, _i32p(idx), _i32p(wgt), C.byref(c0))
            out.append(([(int(i), int(w)) for i, w in zip(idx[:n], wgt[:n])], c0.value))
        return out

    def words(self):
        cnt = C.c_int32()
        p = _l.load().tfhe_hip_lut_multi_words(self.ptr, C.byref(cnt))
        return np.ctypeslib.as_array(p, shape=(cnt.value,)).copy()

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_lut_multi(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _wrap32(x):
    x = int(x) & 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def lut_bootstrap_multi(mo, results, inputs, coefs, c0, key):
    """results[m] = output m of the multi-output LUT bootstrap of (0, c0) + sum coefs[i] inputs[i]; results and inputs are
    LweSample pointers, a result of None is not wanted.  Errors go to last_error() and leave the results untouched."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*inputs)
    res = (_l.LS * max(len(results), 4))(*results)
    cf = np.ascontiguousarray(coefs, dtype=np.int32)
    assert len(cf) == n
    _l.load().tfhe_hip_lut_bootstrap_multi(mo.ptr if mo is not None else None, res, n, ins, _i32p(cf), _wrap32(c0), key.cloud)


def lut_bootstrap_multi_batch(mo, results, inputs, coefs, c0, key):
    """results[m][i] = output m for inputs[k][i]: CiphertextArrays of equal count (a result of None is not wanted)."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*[a.ptr for a in inputs])
    res = (_l.LS * max(len(results), 4))(*[r.ptr if r is not None else None for r in results])
    cf = np.ascontiguousarray(coefs, dtype=np.int32)
    assert len(cf) == n
    count = next(r.count for r in results if r is not None)
    rc = _l.load().tfhe_hip_lut_bootstrap_multi_batch(mo.ptr if mo is not None else None, res, n, ins, _i32p(cf), _wrap32(c0),
                                                      count, key.cloud)
    if rc != 0:
        raise RuntimeError(last_error())


class PackingKey:
    """A packing key (tfhe_hip_new_packing_key*): rows [n][t][k+1][N] under the keyset's ring key that turn up to N LWE
    samples into one ring sample -- the integers are in include/tfhe_hip.h.  t = basebit = 0: the set's own key-switch
    decomposition.  seed: the reproducible form (tests); None draws from the OS-keyed streams."""

    def __init__(self, secret, t=0, basebit=0, seed=None):
        L = _l.load()
        if seed is None:
            ptr = L.tfhe_hip_new_packing_key(secret.ptr, int(t), int(basebit))
        else:
            ptr = L.tfhe_hip_new_packing_key_seeded(secret.ptr, int(t), int(basebit), int(seed))
        self._take(secret.params, ptr)

    def _take(self, params, ptr):
        self.params, self.ptr = params, ptr
        if not ptr:
            raise ValueError("packing key rejected: " + last_error())
        t, b = C.c_int32(), C.c_int32()
        _l.load().tfhe_hip_packing_key_decomposition(ptr, C.byref(t), C.byref(b))
        self.t, self.basebit = t.value, b.value

    @classmethod
    def from_words(cls, params, t, basebit, words):
        """The cloud side: a key from the raw rows it received (n t (k+1) N words, copied)."""
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        tt, bb = (int(t), int(basebit)) if (t or basebit) else (params.ks_t, params.ks_basebit)
        if w.size != params.n * tt * (params.k + 1) * params.N:
            raise ValueError("a packing key of this set and decomposition holds %d words" % (params.n * tt * (params.k + 1) * params.N))
        self = cls.__new__(cls)
        self._take(params, _l.load().tfhe_hip_new_packing_key_from_words(params.ptr, int(t), int(basebit), _i32p(w)))
        return self

    def words(self):
        """The raw rows, [n][t][k+1][N] (a copy)."""
        cnt = C.c_int64()
        p = _l.load().tfhe_hip_packing_key_words(self.ptr, C.byref(cnt))
        pp = self.params
        return np.ctypeslib.as_array(p, shape=(cnt.value,)).copy().reshape(pp.n, self.t, pp.k + 1, pp.N)

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_packing_key(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _taken_packing_key(params, ptr):
    self = PackingKey.__new__(PackingKey)
    self._take(params, ptr)
    return self


class CompressedPackingKey:
    """A seed-compressed packing key (include/tfhe_hip.h): a 40-byte mask seed and the bodies [n][t][N] -- what a client
    sends in place of the raw rows, half their bytes.  expand() gives a PackingKey whose masks are made on the device at
    its first pack, expand_host() one expanded on the CPU; close() both."""

    def __init__(self, ptr, params):
        if not ptr:
            raise ValueError("compressed packing key rejected: " + last_error())
        self.ptr, self.params = ptr, params
        t, b = C.c_int32(), C.c_int32()
        _l.load().tfhe_hip_compressed_packing_key_decomposition(ptr, C.byref(t), C.byref(b))
        self.t, self.basebit = t.value, b.value

    @classmethod
    def generate(cls, secret, t=0, basebit=0):
        return cls(_l.load().tfhe_hip_new_compressed_packing_key(secret.ptr, int(t), int(basebit)), secret.params)

    @classmethod
    def generate_seeded(cls, secret, noise_seed, mask_seed, t=0, basebit=0):
        seed = np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10)
        return cls(_l.load().tfhe_hip_new_compressed_packing_key_seeded(secret.ptr, int(t), int(basebit), int(noise_seed),
                                                                        seed.ctypes.data_as(_l.U32P)), secret.params)

    @classmethod
    def from_words(cls, params, t, basebit, mask_seed, body):
        """The cloud side: a key from the seed and the bodies it received (n t N words, copied)."""
        seed = np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10)
        w = np.ascontiguousarray(body, dtype=np.int32).reshape(-1)
        tt = int(t) if (t or basebit) else params.ks_t
        if tt >= 1 and w.size != params.n * tt * params.N:
            raise ValueError("a compressed packing key of this set and decomposition holds %d body words" % (params.n * tt * params.N))
        return cls(_l.load().tfhe_hip_new_compressed_packing_key_from_words(params.ptr, int(t), int(basebit),
                                                                            seed.ctypes.data_as(_l.U32P), _i32p(w)), params)

    def seed(self):
        return np.ctypeslib.as_array(_l.load().tfhe_hip_compressed_packing_key_seed(self.ptr), shape=(10,)).copy()

    def body(self):
        """int32 [n t N]: a view of the key's words (valid until close())"""
        cnt = C.c_int64()
        p = _l.load().tfhe_hip_compressed_packing_key_body(self.ptr, C.byref(cnt))
        return np.ctypeslib.as_array(p, shape=(cnt.value,))

    @property
    def nbytes(self):
        """the bytes that travel: the seed and the bodies"""
        return int(_l.load().tfhe_hip_compressed_packing_key_bytes(self.ptr))

    def _params(self):
        if self.params is None:
            raise ValueError("a key loaded from a file carries no ParameterSet object: pass params= to load()")
        return self.params

    def expand(self):
        return _taken_packing_key(self._params(), _l.load().tfhe_hip_expand_packing_key(self.ptr))

    def expand_host(self):
        return _taken_packing_key(self._params(), _l.load().tfhe_hip_expand_packing_key_host(self.ptr))

    def save(self, path):
        with _CFile(path, "wb") as fp:
            _l.load().tfhe_hip_export_compressed_packing_key_toFile(fp, self.ptr)

    @classmethod
    def load(cls, path, params=None):
        """params: the ParameterSet the key belongs to (the file holds its record; expand() hands it to the PackingKey)"""
        with _CFile(path, "rb") as fp:
            ptr = _l.load().tfhe_hip_new_compressed_packing_key_fromFile(fp)
        if not ptr:
            raise ValueError("cannot load a compressed packing key from %s: %s" % (path, last_error()))
        return cls(ptr, params)

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_compressed_packing_key(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_image(pkey, key):
    """the device NTT image of a packing key under the twiddles of `key`'s cloud key (made now if it was not yet), int32"""
    L = _l.load()
    L.tfhe_hip_clear_error()
    words = L.tfhe_hip_test_pack_image(pkey.ptr, key.cloud, None, 0)
    if words < 0:
        raise RuntimeError(last_error())
    out = np.zeros(words, dtype=np.int32)
    if L.tfhe_hip_test_pack_image(pkey.ptr, key.cloud, _i32p(out), words) != words:
        raise RuntimeError(last_error())
    return out


def seeded_stats():
    """expanded_packing_keys, packing_expand_launches, seeded_unpacked_samples, seeded_unpack_launches"""
    s = _l.SeededStats()
    _l.load().tfhe_hip_get_seeded_stats(C.byref(s))
    return {f: getattr(s, f) for f in _l.SEEDED_STATS_FIELDS}


def pack(pkey, samples, count, key, first=0):
    """The (k+1) N words of samples[first .. first + count) packed under `pkey` (tfhe_hip_pack_samples); `samples` is a
    CiphertextArray, `key` the keyset whose cloud key evaluates.  Pending operations run first."""
    p = pkey.params
    out = np.zeros((p.k + 1) * p.N, dtype=np.int32)
    rc = _l.load().tfhe_hip_pack_samples(pkey.ptr, samples.at(first), int(count), key.cloud, _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def pack_device(pkey, samples, count, key, device_ptr, first=0):
    """The same into device memory at `device_ptr` ((k+1) N int32 words), stream-ordered on tfhe_hip_stream()."""
    rc = _l.load().tfhe_hip_pack_samples_device(pkey.ptr, samples.at(first), int(count), key.cloud, C.c_void_p(int(device_ptr)))
    if rc != 0:
        raise RuntimeError(last_error())


def packed_phases(words, key):
    """The phases of all N coefficients of a packed sample under the secret keyset `key` (host)."""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    out = np.zeros(key.params.N, dtype=np.int32)
    if _l.load().tfhe_hip_packed_phase(key.ptr, _i32p(w), _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def packed_decrypt(words, count, key):
    """The bits (phase > 0) of the first `count` coefficients of a packed sample (host)."""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    out = np.zeros(max(int(count), 1), dtype=np.int32)
    if _l.load().tfhe_hip_packed_decrypt_bits(key.ptr, _i32p(w), int(count), _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out[:count]


def kernel_pack(pkey, key, sample_words, idx_per_wg=0):
    """The pack of caller-supplied sample words [count][n+1] (tfhe_hip_kernel_pack: crafted operands, no slots)."""
    p = pkey.params
    sw = np.ascontiguousarray(sample_words, dtype=np.int32).reshape(-1, p.words)
    out = np.zeros((p.k + 1) * p.N, dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_pack(pkey.ptr, key.cloud, _i32p(sw), sw.shape[0], int(idx_per_wg), _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def _ring_words(words, p):
    return np.ascontiguousarray(words, dtype=np.int32).reshape(-1, (p.k + 1) * p.N)


def _compressed_fixture(seed, mask_seed):
    """(mask seed as uint32 [10] or None, noise seed) of a compressed ring encryption: both given, or neither"""
    if (seed is None) != (mask_seed is None):
        raise ValueError("the reproducible compressed form takes both seed (the noise) and mask_seed (ten words)")
    return (None, 0) if seed is None else (np.ascontiguousarray(mask_seed, dtype=np.uint32).reshape(10), int(seed))


def ring_encrypt(mu, key, seed=None, compressed=False, mask_seed=None):
    """One ring (TLWE) sample, (k+1) N words, encrypting the N torus words `mu` under the ring key of the secret keyset
    `key` (tfhe_hip_ring_encrypt; host only).  seed: the reproducible form (tests); None draws from OS-keyed streams.
    packed_phases / packed_decrypt decrypt it.
    compressed: the 10 + N words of a seed-compressed sample instead (mask seed, body), a fresh seed per call; its
    reproducible form takes seed (the noise) and mask_seed.  ring_expand gives the plain words, unpack_seeded opens it."""
    p = key.params
    m = np.ascontiguousarray([_wrap32(x) for x in np.asarray(mu).reshape(-1)], dtype=np.int32)
    if m.shape != (p.N,):
        raise ValueError("a ring sample of this parameter set carries %d words" % p.N)
    L = _l.load()
    if compressed:
        ms, ns = _compressed_fixture(seed, mask_seed)
        out = np.zeros(10 + p.N, dtype=np.int32)
        rc = (L.tfhe_hip_ring_encrypt_compressed(key.ptr, _i32p(m), _i32p(out)) if ms is None
              else L.tfhe_hip_ring_encrypt_compressed_seeded(key.ptr, _i32p(m), _i32p(out), ms.ctypes.data_as(_l.U32P), ns))
    else:
        out = np.zeros((p.k + 1) * p.N, dtype=np.int32)
        rc = (L.tfhe_hip_ring_encrypt(key.ptr, _i32p(m), _i32p(out)) if seed is None
              else L.tfhe_hip_ring_encrypt_seeded(key.ptr, _i32p(m), _i32p(out), int(seed)))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_encrypt_bits(bits, key, seed=None, compressed=False, mask_seed=None):
    """The same for 1..N bits: coefficient j carries +-2^29 for bit j, coefficients from len(bits) on carry 0."""
    p = key.params
    b = np.ascontiguousarray(bits, dtype=np.int32).reshape(-1)
    L = _l.load()
    if compressed:
        ms, ns = _compressed_fixture(seed, mask_seed)
        out = np.zeros(10 + p.N, dtype=np.int32)
        rc = (L.tfhe_hip_ring_encrypt_bits_compressed(key.ptr, _i32p(b), len(b), _i32p(out)) if ms is None
              else L.tfhe_hip_ring_encrypt_bits_compressed_seeded(key.ptr, _i32p(b), len(b), _i32p(out),
                                                                  ms.ctypes.data_as(_l.U32P), ns))
    else:
        out = np.zeros((p.k + 1) * p.N, dtype=np.int32)
        rc = (L.tfhe_hip_ring_encrypt_bits(key.ptr, _i32p(b), len(b), _i32p(out)) if seed is None
              else L.tfhe_hip_ring_encrypt_bits_seeded(key.ptr, _i32p(b), len(b), _i32p(out), int(seed)))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_expand(words, N):
    """The plain 2 N words of every seed-compressed sample in `words` ([nring][10 + N]): the stream words of its seed, then
    its body (tfhe_hip_ring_expand_host; host only, no key) -> int32 [nring][2 N]"""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, 10 + N)
    out = np.zeros((w.shape[0], 2 * N), dtype=np.int32)
    for r in range(w.shape[0]):
        if _l.load().tfhe_hip_ring_expand_host(_i32p(w[r]), int(N), _i32p(out[r])) != 0:
            raise RuntimeError(last_error())
    return out


def _unpack_index(index, count):
    if index is None:
        if count is None:
            raise ValueError("unpack needs an index list or a count")
        return None, int(count)
    idx = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
    if count is not None and int(count) != len(idx):
        raise ValueError("count differs from the length of the index list")
    return idx, len(idx)


def unpack(words, key, result, index=None, count=None, first=0):
    """Opens ring samples on the device (tfhe_hip_unpack_samples): words holds nring samples of (k+1) N words, index[j] =
    r N + e names coefficient e of sample r (None: 0 .. count - 1), and the key switch of Extract_e lands in a fresh slot
    of result[first + j].  result: a CiphertextArray, or a list of LweSample pointers (CiphertextArray.at) for the
    scattered form.  key: the keyset whose cloud key evaluates.  Recorded operations stay recorded."""
    p = key.params
    w = _ring_words(words, p)
    idx, n = _unpack_index(index, count)
    L = _l.load()
    if isinstance(result, CiphertextArray):
        rc = L.tfhe_hip_unpack_samples(key.cloud, _i32p(w), w.shape[0], _i32p(idx) if idx is not None else None, n, result.at(first))
    else:
        if len(result) - first < n:
            raise ValueError("fewer result samples than indices")
        ptrs = (_l.LS * max(len(result) - first, 1))(*result[first:])
        rc = L.tfhe_hip_unpack_samples_scattered(key.cloud, _i32p(w), w.shape[0], _i32p(idx) if idx is not None else None, n, ptrs)
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def unpack_device(device_ptr, nring, key, result, index=None, count=None, first=0):
    """The same from device memory at `device_ptr` (nring (k+1) N int32 words), stream-ordered on tfhe_hip_stream(): the
    call returns with the work enqueued; keep the memory until the stream has passed."""
    idx, n = _unpack_index(index, count)
    rc = _l.load().tfhe_hip_unpack_samples_device(key.cloud, C.c_void_p(int(device_ptr)), int(nring),
                                                  _i32p(idx) if idx is not None else None, n, result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def unpack_seeded(words, key, result, index=None, count=None, first=0):
    """unpack() of seed-compressed ring samples (tfhe_hip_unpack_samples_seeded): words holds nring records of 10 + N
    words; the mask of each is regenerated on the device.  The result words are those of unpack() on ring_expand(words)."""
    p = key.params
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, 10 + p.N)
    idx, n = _unpack_index(index, count)
    ip = _i32p(idx) if idx is not None else None
    L = _l.load()
    if isinstance(result, CiphertextArray):
        rc = L.tfhe_hip_unpack_samples_seeded(key.cloud, _i32p(w), w.shape[0], ip, n, result.at(first))
    else:
        if len(result) - first < n:
            raise ValueError("fewer result samples than indices")
        ptrs = (_l.LS * max(len(result) - first, 1))(*result[first:])
        rc = L.tfhe_hip_unpack_samples_seeded_scattered(key.cloud, _i32p(w), w.shape[0], ip, n, ptrs)
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def unpack_seeded_device(device_ptr, nring, key, result, index=None, count=None, first=0):
    """The same from device memory at `device_ptr` (nring (10 + N) int32 words), stream-ordered like unpack_device."""
    idx, n = _unpack_index(index, count)
    rc = _l.load().tfhe_hip_unpack_samples_seeded_device(key.cloud, C.c_void_p(int(device_ptr)), int(nring),
                                                         _i32p(idx) if idx is not None else None, n, result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_extract_seeded(key, words, index=None, count=None):
    """The seeded extract kernel's rows alone (tfhe_hip_kernel_ring_extract_seeded): u[count][N+1], no key switch."""
    p = key.params
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, 10 + p.N)
    idx, n = _unpack_index(index, count)
    u = np.zeros((n, p.k * p.N + 1), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_ring_extract_seeded(key.cloud, _i32p(w), w.shape[0], _i32p(idx) if idx is not None else None,
                                                       n, _i32p(u))
    if rc != 0:
        raise RuntimeError(last_error())
    return u


def extract_rows(u_stride):
    """the rows of the last extract launch as the kernel stored them, padding included: int32 [rows][u_stride]"""
    L = _l.load()
    words = L.tfhe_hip_test_extract_rows(None, 0)
    out = np.zeros(max(words, 0), dtype=np.int32)
    if words < 0 or (words and L.tfhe_hip_test_extract_rows(_i32p(out), words) != words):
        raise RuntimeError(last_error())
    return out.reshape(-1, u_stride)


def kernel_ring_extract(key, words, index=None, count=None):
    """The extract kernel's rows alone (tfhe_hip_kernel_ring_extract): u[count][kN+1], no key switch."""
    p = key.params
    w = _ring_words(words, p)
    idx, n = _unpack_index(index, count)
    u = np.zeros((n, p.k * p.N + 1), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_ring_extract(key.cloud, _i32p(w), w.shape[0], _i32p(idx) if idx is not None else None, n, _i32p(u))
    if rc != 0:
        raise RuntimeError(last_error())
    return u


def tgsw_words(params):
    """The words of one TGSW-encrypted bit: (k+1) l (k+1) N (tfhe_hip_tgsw_words)."""
    return int(_l.load().tfhe_hip_tgsw_words(params.ptr))


def tgsw_encrypt_bits(bits, key, seed=None):
    """TGSW samples of 1..20 index bits under the ring key of the secret keyset `key` (tfhe_hip_tgsw_encrypt_bits; host
    only) -> int32 [len(bits)][(k+1) l][k+1][N], the words of a bootstrapping key with n = len(bits).  bits[0] is the least
    significant index bit.  seed: the reproducible form (tests); None draws from OS-keyed streams."""
    p = key.params
    b = np.ascontiguousarray(bits, dtype=np.int32).reshape(-1)
    out = np.zeros((max(len(b), 1), (p.k + 1) * p.l, p.k + 1, p.N), dtype=np.int32)
    L = _l.load()
    rc = (L.tfhe_hip_tgsw_encrypt_bits(key.ptr, _i32p(b), len(b), _i32p(out)) if seed is None
          else L.tfhe_hip_tgsw_encrypt_bits_seeded(key.ptr, _i32p(b), len(b), _i32p(out), int(seed)))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


class Selector:
    """The server's copy of d TGSW-encrypted index bits (tfhe_hip_new_selector): `words` is what tgsw_encrypt_bits made,
    [d][(k+1) l][k+1][N]; d = 0 (no words) selects from a gallery of one.  The integers are in include/tfhe_hip.h."""

    def __init__(self, params, words=None):
        w = np.zeros(0, dtype=np.int32) if words is None else np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        per_bit = tgsw_words(params)
        if per_bit <= 0 or w.size % per_bit:
            raise ValueError("a selector of this parameter set holds %d words per bit" % per_bit)
        self.params, self.nbits = params, w.size // per_bit
        self.ptr = _l.load().tfhe_hip_new_selector(params.ptr, _i32p(w) if w.size else None, self.nbits)
        if not self.ptr:
            raise ValueError("selector rejected: " + last_error())

    @classmethod
    def from_compressed(cls, params, words, nbits=None):
        """The server's copy of a seed-compressed record (tgsw_encrypt_bits_compressed / _polys_compressed): seed and bodies
        are kept, only the bodies are copied to the card at first use and the masks are written there
        (tfhe_hip_new_selector_compressed).  nbits: the first nbits samples of the record (default: all)."""
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        per_bit = tgsw_compressed_words(params, 1) - 10
        if w.size <= 10 or (w.size - 10) % per_bit:
            raise ValueError("a compressed record of this parameter set holds 10 + %d words per sample" % per_bit)
        count = (w.size - 10) // per_bit
        self = cls.__new__(cls)
        self.params, self.nbits = params, count if nbits is None else int(nbits)
        self.ptr = _l.load().tfhe_hip_new_selector_compressed(params.ptr, _i32p(w), count, self.nbits)
        if not self.ptr:
            raise ValueError("selector rejected: " + last_error())
        return self

    def upload_bytes(self):
        """The bytes the image's upload copied to the card; 0 before the first use (tfhe_hip_selector_upload_bytes)."""
        return int(_l.load().tfhe_hip_selector_upload_bytes(self.ptr))

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_selector(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ring_select(selector, gallery, device=False):
    """The CMUX tree of `selector` over a gallery of M ring samples, 1 <= M <= 2^nbits: the (k+1) N words that encrypt the
    phase polynomial of entry index = sum_j bit_j 2^j (tfhe_hip_ring_select).  Recorded operations stay recorded.
    device=False: gallery is [M][(k+1) N] host words and the result a numpy array.  device=True: gallery is an int32 torch
    tensor resident on the engine's device (written before the call: synchronise torch's stream first) and the result a
    new tensor there, stream-ordered on tfhe_hip_stream() -- ready for unpack_device; wait (tfhe_hip_stream_sync) before
    reading it through torch, and keep both tensors until then."""
    p = selector.params
    sw = (p.k + 1) * p.N
    L = _l.load()
    if device:
        import torch
        if gallery.dtype != torch.int32 or not gallery.is_contiguous() or gallery.numel() == 0 or gallery.numel() % sw:
            raise ValueError("a device gallery is a contiguous int32 tensor of M (k+1) N words")
        out = torch.empty(sw, dtype=torch.int32, device=gallery.device)
        rc = L.tfhe_hip_ring_select_device(selector.ptr, C.c_void_p(gallery.data_ptr()), gallery.numel() // sw, C.c_void_p(out.data_ptr()))
    else:
        g = _ring_words(gallery, p)
        out = np.zeros(sw, dtype=np.int32)
        rc = L.tfhe_hip_ring_select(selector.ptr, _i32p(g), g.shape[0], _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_cmux(selector, bit, d1, d0):
    """CMUX(G_bit, d1[c], d0[c]) of caller-supplied ring samples [count][(k+1) N] in one launch (tfhe_hip_kernel_ring_cmux)."""
    p = selector.params
    a, b = _ring_words(d1, p), _ring_words(d0, p)
    if a.shape != b.shape:
        raise ValueError("d1 and d0 hold the same number of ring samples")
    out = np.zeros_like(a)
    if _l.load().tfhe_hip_kernel_ring_cmux(selector.ptr, int(bit), _i32p(a), _i32p(b), a.shape[0], _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def last_select_ms():
    """The launches of the last ring_select or ring_lookup between two stream events, in ms; -1 unless kernel timing was on."""
    return _l.load().tfhe_hip_last_select_ms()


def lookup_samples(params, M, width):
    """R = ceil(M / S): the ring samples a packed gallery of M entries of `width` coefficients holds, S = N / width each."""
    N = params.N
    if width < 1 or width > N or width & (width - 1):
        raise ValueError("width must be a power of two in 1..%d" % N)
    return -(-int(M) // (N // width))


def ring_lookup(selector, gallery, M, width, device=False):
    """The packed lookup (tfhe_hip_ring_lookup): `gallery` holds M entries of `width` = 2^e coefficients, S = N / width per
    ring sample, entry i on coefficients (i mod S) width .. of sample i / S.  The tree of `selector` over the samples under
    its high bits, then one rotation step per low bit: coefficients 0 .. width - 1 of the (k+1) N result words carry the
    phase of entry index = sum_j bit_j 2^j.  width = N is ring_select.  Host and device forms as for ring_select."""
    p = selector.params
    sw = (p.k + 1) * p.N
    R = lookup_samples(p, M, width)
    L = _l.load()
    if device:
        import torch
        if gallery.dtype != torch.int32 or not gallery.is_contiguous() or gallery.numel() != R * sw:
            raise ValueError("a device gallery of %d entries is a contiguous int32 tensor of %d (k+1) N words" % (M, R))
        out = torch.empty(sw, dtype=torch.int32, device=gallery.device)
        rc = L.tfhe_hip_ring_lookup_device(selector.ptr, C.c_void_p(gallery.data_ptr()), int(M), int(width), C.c_void_p(out.data_ptr()))
    else:
        g = _ring_words(gallery, p)
        if g.shape[0] != R:
            raise ValueError("a gallery of %d entries of width %d holds %d ring samples" % (M, width, R))
        out = np.zeros(sw, dtype=np.int32)
        rc = L.tfhe_hip_ring_lookup(selector.ptr, _i32p(g), int(M), int(width), _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_cmux_rotate(selector, bit, rot, d0):
    """ROT(G_bit, rot, d0[c]) = CMUX(G_bit, X^(-rot) d0[c], d0[c]) of caller-supplied ring samples [count][(k+1) N] in one
    launch (tfhe_hip_kernel_ring_cmux_rotate)."""
    a = _ring_words(d0, selector.params)
    out = np.zeros_like(a)
    if _l.load().tfhe_hip_kernel_ring_cmux_rotate(selector.ptr, int(bit), int(rot), _i32p(a), a.shape[0], _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def _ring_index(ring_index, count):
    if ring_index is None:
        return None, None
    idx = np.ascontiguousarray(ring_index, dtype=np.int32).reshape(-1)
    if len(idx) != count:
        raise ValueError("ring_index names one ring sample per rotation")
    return idx, _i32p(idx)


def _rotation_tables(tables, p, device):
    """(pointer argument, the number of ring samples, what keeps the words alive)"""
    sw = (p.k + 1) * p.N
    if device:
        import torch
        if tables.dtype != torch.int32 or not tables.is_contiguous() or tables.numel() == 0 or tables.numel() % sw:
            raise ValueError("device ring samples are a contiguous int32 tensor of (k+1) N words each")
        return C.c_void_p(tables.data_ptr()), tables.numel() // sw, tables
    t = _ring_words(tables, p)
    return _i32p(t), t.shape[0], t


def ring_blind_rotate(tables, index, key, count=None, ring_index=None, first=0, device=False):
    """The blind rotation of encrypted ring samples by LWE samples (tfhe_hip_ring_blind_rotate): rotation j < count turns
    ring sample ring_index[j] (None: j) of `tables` [nring][(k+1) N] by index[first + j], a sample of a CiphertextArray the
    server computed, under the cloud key of `key` -> ACC_n of every rotation, int32 [count][(k+1) N] (host), or with
    device=True (`tables` an int32 torch tensor on the card) a tensor there, the work enqueued.  A recording the index
    samples depend on is flushed first; otherwise it stays recorded."""
    p = key.params
    sw = (p.k + 1) * p.N
    count = (len(ring_index) if ring_index is not None else index.count - first) if count is None else int(count)
    keep, idxp = _ring_index(ring_index, count)
    ptr, nring, alive = _rotation_tables(tables, p, device)
    L = _l.load()
    if device:
        import torch
        out = torch.empty(max(count, 1) * sw, dtype=torch.int32, device=alive.device)
        rc = L.tfhe_hip_ring_blind_rotate_device(key.cloud, ptr, nring, idxp, index.at(first), count, C.c_void_p(out.data_ptr()))
    else:
        out = np.zeros((max(count, 1), sw), dtype=np.int32)
        rc = L.tfhe_hip_ring_blind_rotate(key.cloud, ptr, nring, idxp, index.at(first), count, _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_lut_bootstrap(tables, index, key, result, count=None, ring_index=None, first=0, result_first=0, device=False):
    """The ring LUT bootstrap (tfhe_hip_ring_lut_bootstrap): result[result_first + j] receives, in a fresh slot, the key
    switch of Extract_0 of ring sample ring_index[j] (None: j) of `tables` blind-rotated by index[first + j] -- an ENCRYPTED
    table looked up under an index the server computed.  Host and device forms of the tables as for ring_blind_rotate; the
    device form returns with the work enqueued.  Operations recorded earlier and not involved stay recorded."""
    p = key.params
    count = (len(ring_index) if ring_index is not None else index.count - first) if count is None else int(count)
    keep, idxp = _ring_index(ring_index, count)
    ptr, nring, alive = _rotation_tables(tables, p, device)
    L = _l.load()
    fn = L.tfhe_hip_ring_lut_bootstrap_device if device else L.tfhe_hip_ring_lut_bootstrap
    if fn(key.cloud, ptr, nring, idxp, index.at(first), count, result.at(result_first)) != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_rotate(key, tables, lwe, ring_index=None, rows=False):
    """The raw launch (tfhe_hip_kernel_ring_rotate): ring samples `tables` [nring][(k+1) N] and LWE words `lwe` [count][n + 1],
    caller words both, rotation j of sample ring_index[j] (None: j) by sample j under the cloud key of `key` -> ACC_n
    [count][(k+1) N], or with rows=True the rows Extract_0(ACC_n) [count][kN + 1] before the key switch."""
    p = key.params
    t = _ring_words(tables, p)
    w = np.ascontiguousarray(lwe, dtype=np.int32).reshape(-1, p.n + 1)
    keep, idxp = _ring_index(ring_index, len(w))
    out = np.zeros((len(w), p.k * p.N + 1 if rows else (p.k + 1) * p.N), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_ring_rotate(key.cloud, _i32p(t), t.shape[0], idxp, _i32p(w), len(w), None if rows else _i32p(out),
                                               _i32p(out) if rows else None)
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def last_ring_rotate_ms():
    """The rotation launches of the last ring_blind_rotate / ring_lut_bootstrap between two stream events, in ms; -1 unless
    kernel timing was on."""
    return _l.load().tfhe_hip_last_ring_rotate_ms()


def tgsw_encrypt_polys(polys, key, seed=None):
    """TGSW samples of 1..20 small-integer polynomials [count][N] under the ring key of the secret keyset `key`
    (tfhe_hip_tgsw_encrypt_polys; host only) -> int32 [count][(k+1) l][k+1][N], words a Selector takes like those of bits.
    A constant polynomial 0 / 1 under a seed gives the words of tgsw_encrypt_bits under that seed."""
    p = key.params
    q = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, p.N)
    out = np.zeros((max(len(q), 1), (p.k + 1) * p.l, p.k + 1, p.N), dtype=np.int32)
    L = _l.load()
    rc = (L.tfhe_hip_tgsw_encrypt_polys(key.ptr, _i32p(q), len(q), _i32p(out)) if seed is None
          else L.tfhe_hip_tgsw_encrypt_polys_seeded(key.ptr, _i32p(q), len(q), _i32p(out), int(seed)))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def tgsw_compressed_words(params, count):
    """The words of a seed-compressed record of `count` TGSW samples: 10 + count (k+1) l N (tfhe_hip_tgsw_compressed_words)."""
    n = int(_l.load().tfhe_hip_tgsw_compressed_words(params.ptr, int(count)))
    if n < 0:
        raise ValueError(last_error())
    return n


def _tgsw_compressed(plain, seeded, values, count, key, seed):
    out = np.zeros(tgsw_compressed_words(key.params, max(count, 1)), dtype=np.int32)
    rc = plain(key.ptr, _i32p(values), count, _i32p(out)) if seed is None else seeded(key.ptr, _i32p(values), count, _i32p(out), int(seed))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def tgsw_encrypt_bits_compressed(bits, key, seed=None):
    """tgsw_encrypt_bits as ONE seed-compressed record (tfhe_hip_tgsw_encrypt_bits_compressed; host only) -> int32
    [10 + len(bits) (k+1) l N]: a fresh mask seed, then the bodies; half the words.  Selector.from_compressed takes it,
    tgsw_expand gives the plain words -- which are a valid TGSW sample, NOT those of tgsw_encrypt_bits.  seed: the
    reproducible form (tests): seed words and noise from one seeded generator."""
    L = _l.load()
    b = np.ascontiguousarray(bits, dtype=np.int32).reshape(-1)
    return _tgsw_compressed(L.tfhe_hip_tgsw_encrypt_bits_compressed, L.tfhe_hip_tgsw_encrypt_bits_compressed_seeded, b, len(b), key, seed)


def tgsw_encrypt_polys_compressed(polys, key, seed=None):
    """tgsw_encrypt_polys as ONE seed-compressed record (tfhe_hip_tgsw_encrypt_polys_compressed), as above."""
    L = _l.load()
    q = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, key.params.N)
    return _tgsw_compressed(L.tfhe_hip_tgsw_encrypt_polys_compressed, L.tfhe_hip_tgsw_encrypt_polys_compressed_seeded, q, len(q), key, seed)


def tgsw_expand(words, params):
    """The plain words [count][(k+1) l][k+1][N] of a seed-compressed record: the stream words of its seed as masks, its
    bodies (tfhe_hip_tgsw_expand_host; host only, no key)."""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    per_bit = tgsw_compressed_words(params, 1) - 10
    if w.size <= 10 or (w.size - 10) % per_bit:
        raise ValueError("a compressed record of this parameter set holds 10 + %d words per sample" % per_bit)
    count = (w.size - 10) // per_bit
    out = np.zeros((count, (params.k + 1) * params.l, params.k + 1, params.N), dtype=np.int32)
    if _l.load().tfhe_hip_tgsw_expand_host(params.ptr, _i32p(w), count, _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def ring_inner(selector, sample, gallery, M, width, key, result, first=0, device=False):
    """The encrypted inner products (tfhe_hip_ring_inner): `gallery` holds M entries of `width` coefficients in ring_lookup's
    layout, sample `sample` of `selector` is the TGSW sample of a probe polynomial (sum_i s_i X^(-i)), and result[first + i]
    receives, in a fresh slot, the key switch of coefficient (i mod S) width of G (.) c_(i / S): the inner product of the
    probe with entry i.  key: the keyset whose cloud key evaluates.  Host and device forms of the gallery as for
    ring_lookup; the device form returns with the work enqueued.  Recorded operations stay recorded."""
    p = selector.params
    sw = (p.k + 1) * p.N
    R = lookup_samples(p, M, width)
    L = _l.load()
    if device:
        import torch
        if gallery.dtype != torch.int32 or not gallery.is_contiguous() or gallery.numel() != R * sw:
            raise ValueError("a device gallery of %d entries is a contiguous int32 tensor of %d (k+1) N words" % (M, R))
        rc = L.tfhe_hip_ring_inner_device(selector.ptr, int(sample), key.cloud, C.c_void_p(gallery.data_ptr()), int(M), int(width),
                                          result.at(first))
    else:
        g = _ring_words(gallery, p)
        if g.shape[0] != R:
            raise ValueError("a gallery of %d entries of width %d holds %d ring samples" % (M, width, R))
        rc = L.tfhe_hip_ring_inner(selector.ptr, int(sample), key.cloud, _i32p(g), int(M), int(width), result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_product(selector, bit, ring):
    """G_bit (.) ring[c], the full products of caller-supplied ring samples [count][(k+1) N] in one launch of the
    product-and-extract kernel (tfhe_hip_kernel_ring_product)."""
    a = _ring_words(ring, selector.params)
    out = np.zeros_like(a)
    if _l.load().tfhe_hip_kernel_ring_product(selector.ptr, int(bit), _i32p(a), a.shape[0], _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_inner_rows(selector, bit, ring, M, width):
    """The rows ring_inner key-switches, before the key switch (tfhe_hip_kernel_ring_inner_rows): int32 [M][kN+1]."""
    p = selector.params
    a = _ring_words(ring, p)
    u = np.zeros((int(M), p.k * p.N + 1), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_inner_rows(selector.ptr, int(bit), _i32p(a), a.shape[0], int(M), int(width), _i32p(u)) != 0:
        raise RuntimeError(last_error())
    return u


INNER_MAX_TERMS = 8      # TFHE_HIP_INNER_MAX_TERMS (include/tfhe_hip.h)


def inner_sum_max_terms(params):
    """The most terms ring_inner_sum takes under a selector of this parameter set's gadget
    (tfhe_hip_ring_inner_sum_max_terms): 7 at both built-in sets, from the CRT bound."""
    k = _l.load().tfhe_hip_ring_inner_sum_max_terms(params.ptr)
    if k < 0:
        raise ValueError(last_error())
    return k


def _sum_ring_words(ring, params, terms, groups=None):
    """host words [groups][terms][(k+1) N] of a gallery read as groups of `terms` ring samples"""
    a = _ring_words(ring, params)
    terms = max(int(terms), 1)            # (a term count below 1 is the library's to refuse)
    if a.shape[0] % terms or (groups is not None and a.shape[0] != groups * terms):
        raise ValueError("the gallery holds %d ring samples, not %sgroups of %d" % (a.shape[0], "" if groups is None else "%d " % groups, terms))
    return a


def ring_mul_tgsw_sum(selector, sample, terms, ring, ngroups=None, device=False):
    """sum_t G_(sample + t) (.) c_(g terms + t) for g < ngroups (tfhe_hip_ring_mul_tgsw_sum): `ring` holds ngroups groups of
    `terms` ring samples (host words [ngroups terms][(k+1) N], or an int32 torch tensor resident on the device), the
    selector's samples sample .. sample + terms - 1 are TGSW samples; ONE launch.  Returns the sums [ngroups][(k+1) N]: a
    numpy array, or a device tensor for the device form (which returns with the work enqueued)."""
    p = selector.params
    sw = (p.k + 1) * p.N
    terms = int(terms)
    L = _l.load()
    if device:
        import torch
        if ring.dtype != torch.int32 or not ring.is_contiguous() or terms < 1 or ring.numel() % (terms * sw):
            raise ValueError("a device gallery is a contiguous int32 tensor of groups of %d (k+1) N words" % terms)
        ngroups = ring.numel() // (terms * sw) if ngroups is None else int(ngroups)
        if ngroups * terms * sw > ring.numel():
            raise ValueError("ngroups runs past the gallery")
        out = torch.empty((ngroups, sw), dtype=torch.int32, device=ring.device)
        rc = L.tfhe_hip_ring_mul_tgsw_sum_device(selector.ptr, int(sample), terms, ngroups, C.c_void_p(ring.data_ptr()), C.c_void_p(out.data_ptr()))
    else:
        a = _sum_ring_words(ring, p, terms, ngroups)
        ngroups = a.shape[0] // max(terms, 1)
        out = np.zeros((ngroups, sw), dtype=np.int32)
        rc = L.tfhe_hip_ring_mul_tgsw_sum(selector.ptr, int(sample), terms, ngroups, _i32p(a), _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_inner_sum(selector, sample, terms, gallery, M, width, key, result, first=0, device=False):
    """ring_inner over groups of `terms` ring samples (tfhe_hip_ring_inner_sum): entry i < M of the gallery spans the `terms`
    samples of group i / S (S = N / width), and result[first + i] receives, in a fresh slot, the key switch of coefficient
    (i mod S) width of sum_t G_(sample + t) (.) c_((i / S) terms + t) -- ONE product launch, one key switch per entry.
    Host and device forms of the gallery as for ring_inner."""
    p = selector.params
    sw = (p.k + 1) * p.N
    G = lookup_samples(p, M, width)
    terms = int(terms)
    L = _l.load()
    if device:
        import torch
        if gallery.dtype != torch.int32 or not gallery.is_contiguous() or gallery.numel() != G * terms * sw:
            raise ValueError("a device gallery of %d entries is a contiguous int32 tensor of %d groups of %d (k+1) N words" % (M, G, terms))
        rc = L.tfhe_hip_ring_inner_sum_device(selector.ptr, int(sample), terms, key.cloud, C.c_void_p(gallery.data_ptr()), int(M), int(width),
                                              result.at(first))
    else:
        g = _sum_ring_words(gallery, p, terms, G)
        rc = L.tfhe_hip_ring_inner_sum(selector.ptr, int(sample), terms, key.cloud, _i32p(g), int(M), int(width), result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_inner_sum_product(selector, sample, terms, ring):
    """ring_mul_tgsw_sum's host form through the raw test entry (tfhe_hip_kernel_ring_inner_sum_product)."""
    a = _sum_ring_words(ring, selector.params, terms)
    ngroups = a.shape[0] // max(int(terms), 1)
    out = np.zeros((ngroups, a.shape[1]), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_inner_sum_product(selector.ptr, int(sample), int(terms), ngroups, _i32p(a), _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_inner_sum_rows(selector, sample, terms, ring, M, width):
    """The rows ring_inner_sum key-switches, before the key switch (tfhe_hip_kernel_ring_inner_sum_rows): int32 [M][kN+1]."""
    p = selector.params
    a = _sum_ring_words(ring, p, terms)
    u = np.zeros((int(M), p.k * p.N + 1), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_inner_sum_rows(selector.ptr, int(sample), int(terms), _i32p(a), a.shape[0] // max(int(terms), 1), int(M), int(width),
                                                     _i32p(u)) != 0:
        raise RuntimeError(last_error())
    return u


def public_max_coef(N):
    """T = TFHE_HIP_PUBLIC_MAX_COEF(N): the largest coefficient magnitude of a public polynomial (2^11 at N = 1024, 2^10
    at N = 2048; include/tfhe_hip.h)"""
    return {1024: 2048, 2048: 1024}.get(int(N), 0)


class PublicGallery:
    """R public small-integer polynomials [R][N], |coefficient| <= public_max_coef(N), that ring samples are multiplied by
    (tfhe_hip_new_public_gallery): a clear gallery in ring_lookup's layout for ring_inner_public, or clear probes, weights
    or projections for ring_mul_public.  The device image is made at the first product and kept until close()."""

    def __init__(self, params, polys):
        q = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, params.N)
        self.params, self.count = params, q.shape[0]
        self.ptr = _l.load().tfhe_hip_new_public_gallery(params.ptr, _i32p(q) if q.size else None, self.count)
        if not self.ptr:
            raise ValueError("public gallery rejected: " + last_error())

    def close(self):
        if self.ptr:
            _l.load().tfhe_hip_delete_public_gallery(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _public_counts(gallery, first, npolys, count):
    npolys = gallery.count - int(first) if npolys is None else int(npolys)
    if npolys != 1 and count != 1 and npolys != count:
        raise ValueError("npolys and the number of ring samples must be equal unless one of them is 1")
    return npolys, max(npolys, count)


def ring_mul_public(gallery, ring, first=0, npolys=None, device=False):
    """q * c for public polynomials of `gallery` and ring samples `ring` (tfhe_hip_ring_mul_public): polynomials first ..
    first + npolys - 1 (default: to the gallery's end).  One polynomial is broadcast over all samples, one sample over all
    polynomials, otherwise the product is pairwise -> [max(npolys, count)][(k+1) N].  Recorded operations stay recorded.
    device=False: host words in, a numpy array out.  device=True: `ring` is an int32 torch tensor resident on the engine's
    device and the result a new tensor there, stream-ordered on tfhe_hip_stream()."""
    p = gallery.params
    sw = (p.k + 1) * p.N
    L = _l.load()
    if device:
        import torch
        if ring.dtype != torch.int32 or not ring.is_contiguous() or ring.numel() == 0 or ring.numel() % sw:
            raise ValueError("device ring words are a contiguous int32 tensor of count (k+1) N words")
        count = ring.numel() // sw
        npolys, total = _public_counts(gallery, first, npolys, count)
        out = torch.empty(total * sw, dtype=torch.int32, device=ring.device)
        rc = L.tfhe_hip_ring_mul_public_device(gallery.ptr, int(first), npolys, C.c_void_p(ring.data_ptr()), count, C.c_void_p(out.data_ptr()))
    else:
        c = _ring_words(ring, p)
        npolys, total = _public_counts(gallery, first, npolys, c.shape[0])
        out = np.zeros((total, sw), dtype=np.int32)
        rc = L.tfhe_hip_ring_mul_public(gallery.ptr, int(first), npolys, _i32p(c), c.shape[0], _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_inner_public(gallery, probe_ring, M, width, key, result, first=0, device=False):
    """The inner products of ONE encrypted probe with a clear gallery (tfhe_hip_ring_inner_public): `gallery` holds M
    entries of `width` coefficients in ring_lookup's layout as public polynomials, `probe_ring` is the ring sample of the
    probe polynomial sum_i s_i Delta X^(-i), and result[first + i] receives, in a fresh slot, the key switch of coefficient
    (i mod S) width of q_(i / S) * probe.  key: the keyset whose cloud key evaluates.  device=True: the probe's (k+1) N words
    are an int32 torch tensor on the engine's device; the call returns with the work enqueued."""
    p = gallery.params
    sw = (p.k + 1) * p.N
    L = _l.load()
    if device:
        import torch
        if probe_ring.dtype != torch.int32 or not probe_ring.is_contiguous() or probe_ring.numel() != sw:
            raise ValueError("a device probe is a contiguous int32 tensor of (k+1) N words")
        rc = L.tfhe_hip_ring_inner_public_device(gallery.ptr, key.cloud, C.c_void_p(probe_ring.data_ptr()), int(M), int(width), result.at(first))
    else:
        c = _ring_words(probe_ring, p)
        if c.shape[0] != 1:
            raise ValueError("the probe is ONE ring sample of (k+1) N words")
        rc = L.tfhe_hip_ring_inner_public(gallery.ptr, key.cloud, _i32p(c), int(M), int(width), result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_public_product(gallery, ring, first=0, npolys=None):
    """ring_mul_public's host form through the raw test entry (tfhe_hip_kernel_ring_public_product)."""
    p = gallery.params
    c = _ring_words(ring, p)
    npolys, total = _public_counts(gallery, first, npolys, c.shape[0])
    out = np.zeros((total, (p.k + 1) * p.N), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_public_product(gallery.ptr, int(first), npolys, _i32p(c), c.shape[0], _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_public_rows(gallery, probe_ring, M, width):
    """The rows ring_inner_public key-switches, before the key switch (tfhe_hip_kernel_ring_public_rows): int32 [M][kN+1]."""
    p = gallery.params
    c = _ring_words(probe_ring, p)
    u = np.zeros((int(M), p.k * p.N + 1), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_public_rows(gallery.ptr, _i32p(c), int(M), int(width), _i32p(u)) != 0:
        raise RuntimeError(last_error())
    return u


PUBLIC_MAX_TERMS = 8     # TFHE_HIP_PUBLIC_MAX_TERMS (include/tfhe_hip.h)


def _sum_groups(gallery, first, terms, ngroups):
    terms = int(terms)
    if terms < 1:
        raise ValueError("terms must be at least 1")
    return terms, (gallery.count - int(first)) // terms if ngroups is None else int(ngroups)


def ring_mul_public_sum(gallery, ring, terms, first=0, ngroups=None, device=False):
    """sum_t q_(first + g terms + t) * c_t for g < ngroups (tfhe_hip_ring_mul_public_sum): `ring` holds the `terms` ring
    samples c_t, the gallery is read as groups of `terms` consecutive polynomials (default: every group from `first` to
    its end) -> [ngroups][(k+1) N], ONE launch.  Recorded operations stay recorded.  device=False: host words in, a numpy
    array out.  device=True: `ring` is an int32 torch tensor resident on the engine's device and the result a new tensor
    there, stream-ordered on tfhe_hip_stream()."""
    p = gallery.params
    sw = (p.k + 1) * p.N
    L = _l.load()
    terms, ngroups = _sum_groups(gallery, first, terms, ngroups)
    if device:
        import torch
        if ring.dtype != torch.int32 or not ring.is_contiguous() or ring.numel() != terms * sw:
            raise ValueError("device ring words are a contiguous int32 tensor of terms (k+1) N words")
        out = torch.empty(max(ngroups, 1) * sw, dtype=torch.int32, device=ring.device)
        rc = L.tfhe_hip_ring_mul_public_sum_device(gallery.ptr, int(first), terms, ngroups, C.c_void_p(ring.data_ptr()), C.c_void_p(out.data_ptr()))
    else:
        c = _ring_words(ring, p)
        if c.shape[0] != terms:
            raise ValueError("the ring words are `terms` samples of (k+1) N words")
        out = np.zeros((max(ngroups, 1), sw), dtype=np.int32)
        rc = L.tfhe_hip_ring_mul_public_sum(gallery.ptr, int(first), terms, ngroups, _i32p(c), _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def ring_inner_public_sum(gallery, probe_ring, terms, M, width, key, result, first=0, device=False):
    """The inner products of ONE encrypted probe of `terms` ring samples with a clear gallery of groups of `terms`
    polynomials (tfhe_hip_ring_inner_public_sum): result[first + i] receives, in a fresh slot, the key switch of coefficient
    (i mod S) width of sum_t q_((i / S) terms + t) * probe_t.  key: the keyset whose cloud key evaluates.  device=True: the
    probe's terms (k+1) N words are an int32 torch tensor on the engine's device; the call returns with the work enqueued."""
    p = gallery.params
    sw = (p.k + 1) * p.N
    L = _l.load()
    terms = int(terms)
    if device:
        import torch
        if probe_ring.dtype != torch.int32 or not probe_ring.is_contiguous() or probe_ring.numel() != terms * sw:
            raise ValueError("a device probe is a contiguous int32 tensor of terms (k+1) N words")
        rc = L.tfhe_hip_ring_inner_public_sum_device(gallery.ptr, key.cloud, C.c_void_p(probe_ring.data_ptr()), terms, int(M), int(width),
                                                     result.at(first))
    else:
        c = _ring_words(probe_ring, p)
        if c.shape[0] != terms:
            raise ValueError("the probe is `terms` ring samples of (k+1) N words")
        rc = L.tfhe_hip_ring_inner_public_sum(gallery.ptr, key.cloud, _i32p(c), terms, int(M), int(width), result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def kernel_ring_public_sum_product(gallery, ring, terms, first=0, ngroups=None):
    """ring_mul_public_sum's host form through the raw test entry (tfhe_hip_kernel_ring_public_sum_product)."""
    p = gallery.params
    c = _ring_words(ring, p)
    terms, ngroups = _sum_groups(gallery, first, terms, ngroups)
    if c.shape[0] != terms:
        raise ValueError("the ring words are `terms` samples of (k+1) N words")
    out = np.zeros((max(ngroups, 1), (p.k + 1) * p.N), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_public_sum_product(gallery.ptr, int(first), terms, ngroups, _i32p(c), _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def kernel_ring_public_sum_rows(gallery, probe_ring, terms, M, width):
    """The rows ring_inner_public_sum key-switches, before the key switch (tfhe_hip_kernel_ring_public_sum_rows): int32
    [M][kN+1]."""
    p = gallery.params
    c = _ring_words(probe_ring, p)
    if c.shape[0] != int(terms):
        raise ValueError("the probe is `terms` ring samples of (k+1) N words")
    u = np.zeros((int(M), p.k * p.N + 1), dtype=np.int32)
    if _l.load().tfhe_hip_kernel_ring_public_sum_rows(gallery.ptr, _i32p(c), int(terms), int(M), int(width), _i32p(u)) != 0:
        raise RuntimeError(last_error())
    return u


def ring_trivial(params, values):
    """The noiseless ring sample (0, values): a zero mask and the 1..N torus words `values` as the body (zero behind them).
    It decrypts to `values` under every key, so a gallery of such samples is a PUBLIC table, and ring_lookup over it
    evaluates a public function of the selector's encrypted bits."""
    v = np.ascontiguousarray([_wrap32(x) for x in np.asarray(values).reshape(-1)], dtype=np.int32)
    if not 1 <= v.size <= params.N:
        raise ValueError("a ring sample of this parameter set carries 1..%d words" % params.N)
    out = np.zeros((params.k + 1) * params.N, dtype=np.int32)
    out[params.k * params.N:params.k * params.N + v.size] = v
    return out


def _lwe_record(words):
    """a record as int32 [10 + record_count] and its record_count"""
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    if w.size < 11:
        raise ValueError("a seed-compressed LWE record is ten seed words and at least one body")
    return w, w.size - 10


def _encrypt_compressed(plain, fixture, key, values, seed, mask_seed):
    ms, ns = _compressed_fixture(seed, mask_seed)
    v = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
    out = np.zeros(10 + len(v), dtype=np.int32)
    rc = (plain(key.ptr, _i32p(v), len(v), _i32p(out)) if ms is None
          else fixture(key.ptr, _i32p(v), len(v), _i32p(out), ms.ctypes.data_as(_l.U32P), ns))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def encrypt_bits_compressed(bits, key, seed=None, mask_seed=None):
    """len(bits) fresh bootsSymEncrypt samples as ONE seed-compressed record of 10 + len(bits) words: a fresh mask seed, then
    one body per bit (tfhe_hip_sym_encrypt_bits_compressed; host only).  The reproducible form (tests) takes seed (the
    noise) and mask_seed (ten words).  lwe_expand gives the plain samples, import_seeded opens the record on the device."""
    L = _l.load()
    return _encrypt_compressed(L.tfhe_hip_sym_encrypt_bits_compressed, L.tfhe_hip_sym_encrypt_bits_compressed_seeded, key, bits,
                               seed, mask_seed)


def encrypt_torus_compressed(mu, key, seed=None, mask_seed=None):
    """The same for any torus messages mu (tfhe_hip_sym_encrypt_torus_compressed)."""
    L = _l.load()
    return _encrypt_compressed(L.tfhe_hip_sym_encrypt_torus_compressed, L.tfhe_hip_sym_encrypt_torus_compressed_seeded, key,
                               [_wrap32(x) for x in np.asarray(mu).reshape(-1)], seed, mask_seed)


def lwe_expand(words, n, index=None, count=None):
    """Samples index[j] (None: 0 .. count - 1, by default the whole record) of a seed-compressed record as plain words
    (tfhe_hip_lwe_expand_host; host only, no key) -> int32 [count][n + 1], what CiphertextArray.set_words takes."""
    w, rc_ = _lwe_record(words)
    idx, cnt = _unpack_index(index, rc_ if index is None and count is None else count)
    out = np.zeros((cnt, n + 1), dtype=np.int32)
    if _l.load().tfhe_hip_lwe_expand_host(_i32p(w), int(n), rc_, _i32p(idx) if idx is not None else None, cnt, _i32p(out)) != 0:
        raise RuntimeError(last_error())
    return out


def import_seeded(words, params, result, index=None, count=None, first=0):
    """Opens a seed-compressed LWE record on the device (tfhe_hip_import_samples_seeded): result[first + j] becomes sample
    index[j] of the record (None: 0 .. count - 1, by default the whole record), its mask regenerated on the card inside its
    slot.  result: a CiphertextArray, or a list of LweSample pointers (CiphertextArray.at) for the scattered form.  The
    result words are those of set_words(lwe_expand(words, n, index)).  Recorded operations stay recorded."""
    w, rc_ = _lwe_record(words)
    idx, cnt = _unpack_index(index, rc_ if index is None and count is None else count)
    ip = _i32p(idx) if idx is not None else None
    L = _l.load()
    if isinstance(result, CiphertextArray):
        rc = L.tfhe_hip_import_samples_seeded(params.ptr, _i32p(w), rc_, ip, cnt, result.at(first))
    else:
        if len(result) - first < cnt:
            raise ValueError("fewer result samples than indices")
        ptrs = (_l.LS * max(len(result) - first, 1))(*result[first:])
        rc = L.tfhe_hip_import_samples_seeded_scattered(params.ptr, _i32p(w), rc_, ip, cnt, ptrs)
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def import_seeded_device(device_ptr, record_count, params, result, index=None, count=None, first=0):
    """The same from device memory at `device_ptr` (10 + record_count int32 words), stream-ordered on tfhe_hip_stream():
    the call returns with the work enqueued; keep the memory until the stream has passed."""
    idx, cnt = _unpack_index(index, int(record_count) if index is None and count is None else count)
    rc = _l.load().tfhe_hip_import_samples_seeded_device(params.ptr, C.c_void_p(int(device_ptr)), int(record_count),
                                                         _i32p(idx) if idx is not None else None, cnt, result.at(first))
    if rc != 0:
        raise RuntimeError(last_error())
    return result


def seeded_lwe_stats():
    """seeded_imported_samples, seeded_import_launches"""
    s = _l.SeededLweStats()
    _l.load().tfhe_hip_get_seeded_lwe_stats(C.byref(s))
    return {f: getattr(s, f) for f in _l.SEEDED_LWE_STATS_FIELDS}


def kernel_lwe_expand(params, words, index=None, count=None):
    """The expand kernel's rows alone (tfhe_hip_kernel_lwe_expand), written into scratch rows: int32 [count][n + 1]."""
    w, rc_ = _lwe_record(words)
    idx, cnt = _unpack_index(index, rc_ if index is None and count is None else count)
    out = np.zeros((cnt, params.n + 1), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_lwe_expand(params.ptr, _i32p(w), rc_, _i32p(idx) if idx is not None else None, cnt, _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def expand_slots(stride):
    """the scratch rows of the last kernel_lwe_expand launch as the kernel stored them, padding included: int32 [rows][stride]"""
    L = _l.load()
    words = L.tfhe_hip_test_expand_slots(None, 0)
    out = np.zeros(max(words, 0), dtype=np.int32)
    if words < 0 or (words and L.tfhe_hip_test_expand_slots(_i32p(out), words) != words):
        raise RuntimeError(last_error())
    return out.reshape(-1, stride)


LINEAR_MAX_IN = 16


def linear(result, inputs, coefs, c0, key):
    """result = (0, c0) + sum coefs[i] inputs[i], wrapping mod 2^32 on all n + 1 words (tfhe_hip_linear): no bootstrap, no
    key switch.  result and inputs are LweSample pointers (CiphertextArray.at), 1 to 16 inputs, any int32 coefficients.
    Errors go to last_error() and leave the result untouched."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*inputs)
    cf = np.ascontiguousarray([_wrap32(c) for c in coefs] or [0], dtype=np.int32)
    assert len(coefs) == n
    _l.load().tfhe_hip_linear(result, n, ins, _i32p(cf), _wrap32(c0), key.cloud)


def linear_batch(result, inputs, coefs, c0, key):
    """result[i] = (0, c0) + sum coefs[k] inputs[k][i]: CiphertextArrays of result.count samples."""
    n = len(inputs)
    ins = (_l.LS * max(n, 1))(*[a.ptr for a in inputs])
    cf = np.ascontiguousarray([_wrap32(c) for c in coefs] or [0], dtype=np.int32)
    assert len(coefs) == n
    rc = _l.load().tfhe_hip_linear_batch(result.ptr, n, ins, _i32p(cf), _wrap32(c0), result.count, key.cloud)
    if rc != 0:
        raise RuntimeError(last_error())


def encrypt_torus(sample, mu, key):
    """sample = a fresh encryption of the torus message mu (tfhe_hip_sym_encrypt_torus): bootsSymEncrypt with mu in place
    of +-2^29."""
    _l.load().tfhe_hip_sym_encrypt_torus(sample, _wrap32(mu), key.ptr)


def phase(sample, key):
    """b - <a, s> mod 2^32 of the sample as a signed word (tfhe_hip_sym_phase); pending operations run first."""
    return int(_l.load().tfhe_hip_sym_phase(sample, key.ptr))


def set_deferred(on):
    _l.load().tfhe_hip_set_deferred(1 if on else 0)


def get_deferred():
    return bool(_l.load().tfhe_hip_get_deferred())


def flush():
    return _l.load().tfhe_hip_flush()


def flush_async():
    """Enqueue the pending gates and return while the device works (tfhe_hip_flush_async); wait() completes it."""
    return _l.load().tfhe_hip_flush_async()


def wait():
    return _l.load().tfhe_hip_wait()


def set_tuning(name, value):
    if _l.load().tfhe_hip_set_tuning(name.encode(), int(value)) != 0:
        raise ValueError(last_error())


def stats():
    s = _l.StatsWhole()
    _l.load().tfhe_hip_get_stats(C.byref(s))
    return {f: getattr(s, f) for f in _l.STATS_FIELDS}


def unpack_stats():
    """The counters of the ring-encrypted inputs at the end of TfheHipStats: unpacked_samples, unpack_launches."""
    s = _l.StatsWhole()
    _l.load().tfhe_hip_get_stats(C.byref(s))
    return {f: getattr(s, f) for f in _l.UNPACK_STATS_FIELDS}


def last_flush_keys():
    """Distinct cloud keys the last executed flush ran under (tuning "batch_keys")."""
    return _l.load().tfhe_hip_last_flush_keys()


def reset_stats():
    _l.load().tfhe_hip_reset_stats()


def kernel_negacyclic(key, ip, tp):
    ip = np.ascontiguousarray(ip, dtype=np.int32)
    tp = np.ascontiguousarray(tp, dtype=np.int32)
    res = np.zeros_like(tp)
    rc = _l.load().tfhe_hip_kernel_negacyclic(key.cloud, _i32p(ip), _i32p(tp), _i32p(res), ip.shape[0])
    if rc != 0:
        raise RuntimeError(last_error())
    return res


def kernel_bootstrap_woks(key, lin, want_acc=False):
    p = key.params
    lin = np.ascontiguousarray(lin, dtype=np.int32).reshape(-1, p.words)
    u = np.zeros((lin.shape[0], p.k * p.N + 1), dtype=np.int32)
    acc = np.zeros((lin.shape[0], (p.k + 1) * p.N), dtype=np.int32) if want_acc else None
    rc = _l.load().tfhe_hip_kernel_bootstrap_woks(key.cloud, _i32p(lin), lin.shape[0], _i32p(u),
                                                  _i32p(acc) if want_acc else None)
    if rc != 0:
        raise RuntimeError(last_error())
    return (u, acc) if want_acc else u


def kernel_lut_bootstrap_woks(key, lin, lut_index, polys, want_acc=False):
    """kernel_bootstrap_woks from test polynomials: combination c starts from polys[lut_index[c]] (index < 0: the constant
    test vector)."""
    p = key.params
    lin = np.ascontiguousarray(lin, dtype=np.int32).reshape(-1, p.words)
    idx = np.ascontiguousarray(lut_index, dtype=np.int32).reshape(lin.shape[0])
    polys = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, p.N)
    u = np.zeros((lin.shape[0], p.k * p.N + 1), dtype=np.int32)
    acc = np.zeros((lin.shape[0], (p.k + 1) * p.N), dtype=np.int32) if want_acc else None
    rc = _l.load().tfhe_hip_kernel_lut_bootstrap_woks(key.cloud, _i32p(lin), lin.shape[0], _i32p(idx), _i32p(polys),
                                                      polys.shape[0], _i32p(u), _i32p(acc) if want_acc else None)
    if rc != 0:
        raise RuntimeError(last_error())
    return (u, acc) if want_acc else u


EXTRACT_SPEC_WORDS = 73


def pack_extract_specs(specs):
    """[[(taps, out_c0), ...], ...] -> the records of kernel_lut_bootstrap_multi_woks: {nout, ntaps[4], out_c0[4],
    index[4][8], weight[4][8]} per spec."""
    out = np.zeros((len(specs), EXTRACT_SPEC_WORDS), dtype=np.int32)
    for rec, outputs in zip(out, specs):
        rec[0] = len(outputs)
        for m, (taps, c0) in enumerate(outputs):
            rec[1 + m] = len(taps)
            rec[5 + m] = _wrap32(c0)
            for t, (i, w) in enumerate(taps):
                rec[9 + 8 * m + t] = i
                rec[41 + 8 * m + t] = w
    return out


def kernel_lut_bootstrap_multi_woks(key, lin, lut_index, polys, spec_index, specs, want_acc=False):
    """kernel_lut_bootstrap_woks with extract specs: combination c leaves through specs[spec_index[c]] (index < 0: the
    extract at index 0).  Returns u[count][4][kN+1] -- output m of combination c at [c][m], zeros where there is none --
    and, if asked, the raw accumulators."""
    p = key.params
    lin = np.ascontiguousarray(lin, dtype=np.int32).reshape(-1, p.words)
    idx = np.ascontiguousarray(lut_index, dtype=np.int32).reshape(lin.shape[0])
    sidx = np.ascontiguousarray(spec_index, dtype=np.int32).reshape(lin.shape[0])
    polys = np.ascontiguousarray(polys, dtype=np.int32).reshape(-1, p.N)
    recs = pack_extract_specs(specs)
    u = np.zeros((lin.shape[0], 4, p.k * p.N + 1), dtype=np.int32)
    acc = np.zeros((lin.shape[0], (p.k + 1) * p.N), dtype=np.int32) if want_acc else None
    rc = _l.load().tfhe_hip_kernel_lut_bootstrap_multi_woks(key.cloud, _i32p(lin), lin.shape[0], _i32p(idx), _i32p(polys),
                                                            polys.shape[0], _i32p(sidx), _i32p(recs), recs.shape[0], _i32p(u),
                                                            _i32p(acc) if want_acc else None)
    if rc != 0:
        raise RuntimeError(last_error())
    return (u, acc) if want_acc else u


def kernel_keyswitch(key, u):
    p = key.params
    u = np.ascontiguousarray(u, dtype=np.int32).reshape(-1, p.k * p.N + 1)
    out = np.zeros((u.shape[0], p.words), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_keyswitch(key.cloud, _i32p(u), u.shape[0], _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out


def kernel_keyswitch_matrix(key, u):
    """the rows u through the matrix key switch alone (tfhe_hip_kernel_keyswitch_matrix)"""
    p = key.params
    u = np.ascontiguousarray(u, dtype=np.int32).reshape(-1, p.k * p.N + 1)
    out = np.zeros((u.shape[0], p.words), dtype=np.int32)
    rc = _l.load().tfhe_hip_kernel_keyswitch_matrix(key.cloud, _i32p(u), u.shape[0], _i32p(out))
    if rc != 0:
        raise RuntimeError(last_error())
    return out
