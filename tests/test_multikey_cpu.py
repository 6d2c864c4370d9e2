"""Multi-client batch entries without a GPU: peba1_function_f_batch / peba1_hamming_match_batch (circuits.cpp) compiled
against the plaintext-bit provider of the tfhe API (tests/mock), with libtfhe-hip's extensions stubbed here; the header
declares them; protocol.py parses --clients."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "peba1_circuits.h"

// stubs of the libtfhe-hip extensions the batch drivers call, recording what they were asked
static int g_batch = 0, g_deferred = 0, g_flushes = 0, g_batch_during_flush = -1;
extern "C" int tfhe_hip_set_batch_keys(int on) { int was = g_batch; g_batch = on; return was; }
extern "C" int tfhe_hip_get_deferred(void) { return g_deferred; }
extern "C" void tfhe_hip_set_deferred(int on) { g_deferred = on; }
extern "C" int tfhe_hip_flush(void) { ++g_flushes; g_batch_during_flush = g_batch; return 7; }

int main() {
    const int K = 5, nslots = 3, bits = 8, hb = 16;
    auto *params = new_default_gate_bootstrapping_parameters(128);
    std::vector<TFheGateBootstrappingSecretKeySet *> keys;
    std::vector<const TFheGateBootstrappingCloudKeySet *> ck;
    for (int c = 0; c < K; ++c) { keys.push_back(new_random_gate_bootstrapping_secret_keyset(params)); ck.push_back(&keys[c]->cloud); }
    auto enc = [&](uint64_t v, int n, int c) {
        LweSample *p = new_gate_bootstrapping_ciphertext_array(n, params);
        for (int i = 0; i < n; ++i) bootsSymEncrypt(&p[i], (v >> i) & 1, keys[c]);
        return p;
    };
    std::vector<std::vector<LweSample *>> A(K), B(K);
    std::vector<LweSample *const *> pa(K), pb(K);
    std::vector<LweSample *> rb(K), bound(K), rh(K), ha(K), hbv(K), hbound(K);
    std::printf("{\"clients\": [");
    for (int c = 0; c < K; ++c) {
        for (int s = 0; s < nslots; ++s) { A[c].push_back(enc((37 * s + 11 * c + 3) % 256, bits, c)); B[c].push_back(enc((91 * s + 5 * c) % 256, bits, c)); }
        pa[c] = A[c].data(); pb[c] = B[c].data();
        rb[c] = new_gate_bootstrapping_ciphertext_array(3 * bits, params);
        bound[c] = enc(6000 * c, 3 * bits, c);
        const int w = peba1_hamming_count_bits(hb);
        ha[c] = enc(0xB3C5u * (c + 1) & 0xFFFF, hb, c); hbv[c] = enc(0x2E91u + 77 * c, hb, c);
        hbound[c] = enc(3 + 2 * c, w, c);
        rh[c] = new_gate_bootstrapping_ciphertext_array(w, params);
    }
    g_batch = 0; g_deferred = 0;
    const int lf = peba1_function_f_batch(rb.data(), pa.data(), pb.data(), K, nslots, bound.data(), bits, ck.data(), 0);
    const int batch_f = g_batch_during_flush;
    std::vector<LweSample *> rf(K);
    for (int c = 0; c < K; ++c) rf[c] = new_gate_bootstrapping_ciphertext_array(3 * bits, params);
    peba1_function_f_batch(rf.data(), pa.data(), pb.data(), K, nslots, bound.data(), bits, ck.data(), 1);
    const int lh = peba1_hamming_match_batch(rh.data(), ha.data(), hbv.data(), K, hb, hbound.data(), ck.data());
    for (int c = 0; c < K; ++c)
        std::printf("%s{\"f\": %d, \"f_fast\": %d, \"hamming\": %d}", c ? ", " : "", bootsSymDecrypt(&rb[c][0], keys[c]),
                    bootsSymDecrypt(&rf[c][0], keys[c]), bootsSymDecrypt(&rh[c][0], keys[c]));
    std::printf("], \"levels\": [%d, %d], \"flushes\": %d, \"batch_during_flush\": %d, \"batch_after\": %d, \"deferred_after\": %d}\n",
                lf, lh, g_flushes, batch_f, g_batch, g_deferred);
    return 0;
}
"""


def test_batch_drivers_over_the_plaintext_mock(tmp_path):
    t = str(tmp_path)
    inc = os.path.join(ROOT, "include")
    with open(os.path.join(t, "batch_driver.cpp"), "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=gnu++11", "-fPIC", "-shared", "-I" + inc,
                           os.path.join(ROOT, "tests/mock/plain_tfhe.cpp"), "-o", t + "/libplain_tfhe.so"])
    subprocess.check_call(["g++", "-O1", "-std=gnu++17", "-I" + inc, t + "/batch_driver.cpp",
                           os.path.join(ROOT, "peba1_amd/csrc/circuits.cpp"), os.path.join(ROOT, "peba1_amd/csrc/circuits_fast.cpp"),
                           "-o", t + "/batch_driver", "-L" + t, "-lplain_tfhe", "-Wl,-rpath," + t])
    out = json.loads(subprocess.check_output([t + "/batch_driver"]).decode())
    K, nslots = 5, 3
    assert len(out["clients"]) == K
    for c, got in enumerate(out["clients"]):
        a = [(37 * s + 11 * c + 3) % 256 for s in range(nslots)]
        b = [(91 * s + 5 * c) % 256 for s in range(nslots)]
        dist = sum((x - y) ** 2 for x, y in zip(a, b)) % (1 << 24)
        assert got["f"] == got["f_fast"] == (1 if dist > 6000 * c else 0), c
        ham = bin(((0xB3C5 * (c + 1)) & 0xFFFF) ^ (0x2E91 + 77 * c)).count("1")
        assert got["hamming"] == (1 if ham > 3 + 2 * c else 0), c
    # one flush per batch, with batching on during it; the caller's settings (both 0) restored
    assert out["flushes"] == 3 and out["levels"] == [7, 7]
    assert out["batch_during_flush"] == 1 and out["batch_after"] == 0 and out["deferred_after"] == 0


def test_header_declares_batch_entries():
    with open(os.path.join(ROOT, "include", "peba1_circuits.h")) as f:
        circ = f.read()
    for name in ("peba1_function_f_batch", "peba1_hamming_match_batch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", circ), name
    with open(os.path.join(ROOT, "include", "tfhe_hip.h")) as f:
        hip = f.read()
    assert re.search(r"\bint\s+tfhe_hip_last_flush_keys\s*\(\s*void\s*\)", hip)
    assert re.search(r"\bint\s+tfhe_hip_set_batch_keys\s*\(", hip)
    assert '"batch_keys"' in hip and "TFHE_HIP_BATCH_KEYS" in hip


def test_protocol_parses_clients():
    from peba1_amd import protocol
    a = protocol.parse_args(["--clients", "4", "--nslots", "2", "--fast"])
    assert (a.clients, a.nslots, a.fast) == (4, 2, True)
    assert protocol.parse_args([]).clients == 0
    x = protocol.client_inputs(1, 3, 0x10)
    assert x["key_seed"] == 0x12 and len(x["template"]) == len(x["sample"]) == 3
