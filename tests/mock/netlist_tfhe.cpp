// netlist_tfhe.cpp -- TEST INFRASTRUCTURE: a provider of the tfhe gate API AND of tfhe_hip_gate3 that does no
// arithmetic at all: it records the netlist a circuit issues, one row {op, negate_mask, dst, a, b, c} of wire numbers
// per call, so that the circuit can be replayed gate by gate through the CPU oracle (tests/gate3_common.py) and its
// gates and depth counted without a GPU.  Every write makes a new wire (SSA); LweSample::slot holds a sample's
// current wire, -2 for a fresh sample (a trivial encryption of 0).  bootsCOPY moves the wire number and records nothing.
//   op: 0..9 two-input gate (enum TfheHipGate), 16 MUX, 17 NOT, 32 + enum TfheHipGate3 three-input gate,
//       100 INPUT (a = the encrypted bit), 101 CONSTANT (a = the value)
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "tfhe/tfhe.h"

namespace {
std::vector<int32_t> g_rows;
int32_t g_next = 0;
TFheGateBootstrappingParameterSet g_params;
LweParams g_lwe = {1, 0.0, 0.0};

void row(int32_t op, int32_t mask, LweSample *d, int32_t a, int32_t b, int32_t c) {
    const int32_t dst = g_next++;
    const int32_t r[6] = {op, mask, dst, a, b, c};
    g_rows.insert(g_rows.end(), r, r + 6);
    d->slot = dst;
}
}  // namespace

extern "C" {

void netlist_reset(void) { g_rows.clear(); g_next = 0; }
int32_t netlist_rows(void) { return (int32_t)(g_rows.size() / 6); }
void netlist_copy(int32_t *out) { for (size_t i = 0; i < g_rows.size(); ++i) out[i] = g_rows[i]; }
int32_t netlist_wire(const LweSample *s) { return s->slot; }

TFheGateBootstrappingParameterSet *new_default_gate_bootstrapping_parameters(int32_t) {
    g_params.ks_t = 8; g_params.ks_basebit = 2; g_params.in_out_params = &g_lwe; g_params.tgsw_params = nullptr;
    return &g_params;
}
void delete_gate_bootstrapping_parameters(TFheGateBootstrappingParameterSet *) {}
TFheGateBootstrappingSecretKeySet *new_random_gate_bootstrapping_secret_keyset(const TFheGateBootstrappingParameterSet *p) {
    auto *k = static_cast<TFheGateBootstrappingSecretKeySet *>(std::calloc(1, sizeof(TFheGateBootstrappingSecretKeySet)));
    k->params = p; k->cloud.params = p;
    return k;
}
void delete_gate_bootstrapping_secret_keyset(TFheGateBootstrappingSecretKeySet *k) { std::free(k); }
LweSample *new_gate_bootstrapping_ciphertext_array(int32_t n, const TFheGateBootstrappingParameterSet *) {
    auto *p = static_cast<LweSample *>(std::calloc((size_t)(n > 0 ? n : 1), sizeof(LweSample)));
    for (int i = 0; i < n; ++i) p[i].slot = -2;
    return p;
}
void delete_gate_bootstrapping_ciphertext_array(int32_t, LweSample *p) { std::free(p); }

void bootsSymEncrypt(LweSample *r, int32_t m, const TFheGateBootstrappingSecretKeySet *) { row(100, 0, r, m & 1, -1, -1); }
int32_t bootsSymDecrypt(const LweSample *, const TFheGateBootstrappingSecretKeySet *) { return -1; }   // no values here
void bootsCONSTANT(LweSample *r, int32_t v, const TFheGateBootstrappingCloudKeySet *) { row(101, 0, r, v ? 1 : 0, -1, -1); }
void bootsCOPY(LweSample *r, const LweSample *a, const TFheGateBootstrappingCloudKeySet *) { r->slot = a->slot; }
void bootsNOT(LweSample *r, const LweSample *a, const TFheGateBootstrappingCloudKeySet *) { row(17, 0, r, a->slot, -1, -1); }
void bootsMUX(LweSample *r, const LweSample *a, const LweSample *b, const LweSample *c, const TFheGateBootstrappingCloudKeySet *) {
    row(16, 0, r, a->slot, b->slot, c->slot);
}
#define NETLIST_GATE2(NAME, CODE)                                                                                        \
    void NAME(LweSample *r, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *) {          \
        row(CODE, 0, r, a->slot, b->slot, -1);                                                                           \
    }
NETLIST_GATE2(bootsNAND, 0)
NETLIST_GATE2(bootsOR, 1)
NETLIST_GATE2(bootsAND, 2)
NETLIST_GATE2(bootsNOR, 3)
NETLIST_GATE2(bootsXOR, 4)
NETLIST_GATE2(bootsXNOR, 5)
NETLIST_GATE2(bootsANDNY, 6)
NETLIST_GATE2(bootsANDYN, 7)
NETLIST_GATE2(bootsORNY, 8)
NETLIST_GATE2(bootsORYN, 9)
#undef NETLIST_GATE2

void tfhe_hip_gate3(int gate, int negate_mask, LweSample *r, const LweSample *a, const LweSample *b, const LweSample *c,
                    const TFheGateBootstrappingCloudKeySet *) {
    row(32 + gate, negate_mask, r, a->slot, b->slot, c->slot);
}

}  // extern "C"
