#!/usr/bin/env python3
"""What packing costs at P128 (profiles/packing.txt): for count = 1, 128, 1,024 the time of tfhe_hip_pack_samples_device
between two HIP events on the library's stream, beside tfhe_hip_export_samples_device_async of the same samples and one
blind-rotate launch of the same width (kernel timing, from the stats), the bytes that leave the device either way, and
the shader clock the blind-rotate launches ran at.  Prints; asserts nothing but that the packed bits decrypt.

    python tools/pack_cost.py [--reps 30]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    from peba1_amd import api, lib
    L = lib.load()
    pp = api.ParameterSet(128)
    ks = api.SecretKeySet(pp, 0x5EBA2, device=True)
    pk = api.PackingKey(ks, seed=11)
    L.tfhe_hip_set_encrypt_seed(3)
    L.tfhe_hip_set_kernel_timing(1)
    api.set_deferred(True)
    stream = torch.cuda.ExternalStream(L.tfhe_hip_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(3):
            fn()
        assert L.tfhe_hip_stream_sync() == 0
        ms = []
        for _ in range(args.reps):
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    print("P128: n = %d, N = %d, packing key (t, basebit) = (%d, %d); %d repetitions, median (min) in ms"
          % (pp.n, pp.N, pk.t, pk.basebit, args.reps))
    print("%6s  %18s  %18s  %22s  %12s  %12s" % ("count", "pack (events)", "export (events)", "blind-rotate launch", "bytes LWE", "bytes packed"))
    N = pp.N
    rng = np.random.default_rng(1)
    xa, xb = rng.integers(0, 2, N), rng.integers(0, 2, N)
    a, b = api.CiphertextArray(pp, N).encrypt(xa, ks), api.CiphertextArray(pp, N).encrypt(xb, ks)
    for count in (1, 128, 1024):
        r = api.CiphertextArray(pp, count)
        api.flush()
        api.reset_stats()
        assert L.tfhe_hip_gate_batch(api.GATE_CODES["AND"], r.ptr, a.ptr, b.ptr, count, ks.cloud) == 0
        api.flush()
        st = api.stats()
        assert st["br_launches"] == 1, st["br_launches"]
        ghz = st["clk_shader_cycles"] / st["clk_ref_ticks"] * 0.1 if st["clk_ref_ticks"] else float("nan")
        packed = torch.zeros(2 * N, dtype=torch.int32, device="cuda:0")
        flat = torch.zeros(count * pp.words, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        tp = timed(lambda: api.pack_device(pk, r, count, ks, packed.data_ptr()))
        te = timed(lambda: L.tfhe_hip_export_samples_device_async(r.ptr, count, pp.ptr, C.c_void_p(flat.data_ptr())))
        assert L.tfhe_hip_stream_sync() == 0
        assert list(api.packed_decrypt(packed.cpu().numpy(), count, ks)) == list((xa & xb)[:count])
        print("%6d  %8.4f (%7.4f)  %8.4f (%7.4f)  %9.4f at %.3f GHz  %12d  %12d"
              % (count, tp[0], tp[1], te[0], te[1], st["ms_blind_rotate"], ghz, count * pp.words * 4, 2 * N * 4))
        r.close()
    pk.close()
    ks.close()


if __name__ == "__main__":
    main()
