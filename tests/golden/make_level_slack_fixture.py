#!/usr/bin/env python3
"""tests/golden/level_slack_function_f.npz, the oracle side of tests/test_level_slack_gpu.py: an 8-slot Function_f on 4-bit
values through the CPU oracle's own boots* provider and the same circuit library (oracle/liboracle_boots.so), under the small
parameter set of tests/test_gpu_recorded_programs.py (n = 16, N = 1024, k = 1, l = 3, Bgbit = 7, ks 8 x 2: P128's ring,
gadget and key switch with a 16-step blind rotation -- results are words, no decrypt claim is made at n = 16).  The
values have 4 bits; the circuit runs at bitsize 8, the one size peba1_euclidean_distance admits: like the reference it
accumulates in 24 samples whatever the bitsize, so its distance array must be 3 x 8 long.  Holds the input ciphertext
words (per slot template then probe, then the bound) and the 24 result ciphertexts.

    python tests/golden/make_level_slack_fixture.py [--threads T]
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as O   # noqa: E402
import ks_common as K              # noqa: E402

KEY_SEED, ENC_SEED = 0x51A7, 0x1E7E1
N_LWE, NSLOTS, BITS = 16, 8, 8
TEMPLATE = [(5 * i + 3) % 16 for i in range(NSLOTS)]
PROBE = [(t + 1 + i % 3) % 16 for i, t in enumerate(TEMPLATE)]
BOUND = 20


def main():
    threads = int(sys.argv[sys.argv.index("--threads") + 1]) if "--threads" in sys.argv else 4
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    B = C.CDLL(os.path.join(ROOT, "oracle", "liboracle_boots.so"))
    V = C.c_void_p
    B.orc_keygen.restype = V
    B.orc_keygen.argtypes = [C.POINTER(O.OrcParams), C.c_uint64]
    B.orc_boots_bind.argtypes = [V, C.c_uint64]
    B.orc_boots_params.restype = V
    B.orc_boots_cloud.restype = V
    B.orc_boots_gate_count.restype = C.c_longlong
    B.new_gate_bootstrapping_ciphertext_array.restype = V
    B.new_gate_bootstrapping_ciphertext_array.argtypes = [C.c_int32, V]
    B.bootsSymEncrypt.argtypes = [V, C.c_int32, V]
    B.orc_boots_export.argtypes = [V, C.c_int32, V]
    B.peba1_function_f.argtypes = [V, V, V, C.c_int, V, C.c_int, V]
    p = O.custom_params(n=N_LWE, N=1024, l=K.GADGET[0], Bgbit=K.GADGET[1], ks_t=8, ks_basebit=2, ks_stdev=K.STDEVS[0],
                        bk_stdev=K.STDEVS[1])
    ks = B.orc_keygen(C.byref(p), KEY_SEED)
    B.orc_boots_bind(ks, ENC_SEED)
    B.orc_boots_set_recording(threads)
    params, cloud, SZ = B.orc_boots_params(), B.orc_boots_cloud(), 24

    def enc(v, nb):
        a = B.new_gate_bootstrapping_ciphertext_array(nb, params)
        for i in range(nb):
            B.bootsSymEncrypt(a + i * SZ, (v >> i) & 1, None)
        return a

    def words_of(arr, count):
        w = np.zeros((count, p.n + 1), dtype=np.int32)
        B.orc_boots_export(arr, count, w.ctypes.data_as(V))
        return w

    T, S = [], []
    for t, s in zip(TEMPLATE, PROBE):
        T.append(enc(t, BITS))
        S.append(enc(s, BITS))
    bound = enc(BOUND, 3 * BITS)
    inputs = {"template": np.stack([words_of(a, BITS) for a in T]), "probe": np.stack([words_of(a, BITS) for a in S]),
              "bound": words_of(bound, 3 * BITS)}
    rb = B.new_gate_bootstrapping_ciphertext_array(3 * BITS, params)
    t0 = time.time()
    B.peba1_function_f(rb, (V * NSLOTS)(*S), (V * NSLOTS)(*T), NSLOTS, bound, BITS, cloud)
    result = words_of(rb, 3 * BITS)
    gates = int(B.orc_boots_gate_count())
    dst = os.path.join(ROOT, "tests", "golden", "level_slack_function_f.npz")
    np.savez_compressed(dst, key_seed=np.int64(KEY_SEED), n=np.int64(N_LWE), bits=np.int64(BITS), blind_rotates=np.int64(gates),
                        result=result, **inputs)
    print(f"{dst}: {gates} blind rotations, {time.time() - t0:.1f} s on {threads} threads, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
