#!/usr/bin/env python3
"""The carry-save circuits of the three-input gates against the circuits they replace (profiles/gate3_circuits.txt):
128-bit peba1_hamming_match / peba1_hamming_match_csa alone and 64 per flush, the 128-slot peba1_function_f_fast /
peba1_function_f_fast3; each pair interleaved, three repetitions, every line with the shader clock its launches ran at.
Prints a table; not used by tests, smoke or bench."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from peba1_amd import api, circuits, lib
L = lib.load()
pp = api.ParameterSet(128)
ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
L.tfhe_hip_set_encrypt_seed(5)
api.set_deferred(True)
L.tfhe_hip_set_kernel_timing(1)
rng = np.random.default_rng(1)
def dev(arr):
    return arr.set_words(arr.words())
def num(v, bits):
    return dev(circuits.encrypt_number(pp, v, bits, ks))
pairs = []
for i in range(64):
    a = int.from_bytes(rng.bytes(16), "little"); b = int.from_bytes(rng.bytes(16), "little")
    pairs.append((num(a, 128), num(b, 128), bin(a ^ b).count("1")))
bound = num(64, 8)
def run(fn, count):
    rbs = [api.CiphertextArray(pp, 8) for _ in range(count)]
    api.flush(); api.reset_stats()
    t = time.perf_counter()
    for i in range(count):
        fn(rbs[i], pairs[i][0], pairs[i][1], 128, bound, ks)
    levels = api.flush()
    ms = (time.perf_counter() - t) * 1e3
    s = api.stats()
    for i in range(count):
        assert rbs[i].decrypt(ks)[0] == (1 if pairs[i][2] > 64 else 0)
    ghz = 0.1 * s["clk_shader_cycles"] / max(1, s["clk_ref_ticks"])
    return ms, levels, s["blind_rotates"], ghz
print("circuit count rep wall_ms levels blind_rotates shader_GHz", flush=True)
for warm in range(1):
    run(circuits.hamming_match, 1); run(circuits.hamming_match_csa, 1)
for rep in range(3):
    for count in (1, 64):
        for name, fn in (("hamming_match", circuits.hamming_match), ("hamming_match_csa", circuits.hamming_match_csa)):
            ms, lv, br, ghz = run(fn, count)
            print(f"{name} {count} {rep} {ms:.2f} {lv} {br} {ghz:.3f}", flush=True)
template = [(37 * i + 11) % 255 for i in range(128)]
probe = [(91 * i + 5) % 256 for i in range(128)]
S = circuits.EncryptedVector(pp, probe, 8, ks).to_device(); T = circuits.EncryptedVector(pp, template, 8, ks).to_device()
b24 = num(256, 24)
def runf(fn):
    rb = api.CiphertextArray(pp, 24)
    api.flush(); api.reset_stats()
    t = time.perf_counter()
    fn(rb, S, T, b24, 8, ks)
    levels = api.flush()
    ms = (time.perf_counter() - t) * 1e3
    s = api.stats()
    assert rb.decrypt(ks)[0] == 1
    return ms, levels, s["blind_rotates"], 0.1 * s["clk_shader_cycles"] / max(1, s["clk_ref_ticks"])
runf(circuits.function_f_fast); runf(circuits.function_f_fast3)
for rep in range(3):
    for name, fn in (("function_f_fast", circuits.function_f_fast), ("function_f_fast3", circuits.function_f_fast3)):
        ms, lv, br, ghz = runf(fn)
        print(f"{name} 128slots {rep} {ms:.2f} {lv} {br} {ghz:.3f}", flush=True)
ks.close()
print("DONE")
