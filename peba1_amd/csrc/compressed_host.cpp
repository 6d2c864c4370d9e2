// compressed_host.cpp -- host side of the seed-compressed cloud keys: the key object, its generators, the two expansions
// and the C ABI (include/tfhe_hip.h "seed-compressed cloud keys").  The arithmetic of key generation and of the host
// expansion is in host_keys.cpp, the device expansion in expand.hip behind Engine::upload_compressed_key; the file form is
// in io.cpp.
#include <cstring>
#include <string>

#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {

// null (the error is set) for a parameter set the kernels cannot run: the message of a refused keyset
TfheHipCompressedCloudKey *new_compressed_object(const char *who, const Params &p) {
    if (const char *why = unsupported_reason(p)) { set_error(std::string(who) + ": " + why); return nullptr; }
    auto *key = new TfheHipCompressedCloudKey();
    key->magic = COMPRESSED_KEY_MAGIC;
    key->p = p;
    return key;
}

TfheHipCompressedCloudKey *make_compressed_key(const char *who, const TFheGateBootstrappingSecretKeySet *secret,
                                               const uint64_t *noise_seed, const uint32_t *mask_seed10) {
    if (!secret || !secret->lwe_key) { set_error(std::string(who) + ": null secret keyset"); return nullptr; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    TfheHipCompressedCloudKey *key = new_compressed_object(who, sk.p);
    if (!key) return nullptr;
    if (noise_seed) {
        std::memcpy(key->seed, mask_seed10, sizeof key->seed);
        Rng noise(*noise_seed);
        generate_compressed_key(sk, noise, *key);
    } else {
        // two fresh ChaCha20 streams, as for a keyset: the noise stream's key stays here, the mask stream's key is the seed
        os_seed(key->seed);
        Rng noise = Rng::secure();
        generate_compressed_key(sk, noise, *key);
    }
    return key;
}

}  // namespace

extern "C" {

TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key(const TFheGateBootstrappingSecretKeySet *secret) {
    return make_compressed_key("tfhe_hip_new_compressed_cloud_key", secret, nullptr, nullptr);
}
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key_seeded(const TFheGateBootstrappingSecretKeySet *secret,
                                                                    uint64_t noise_seed, const uint32_t *mask_seed10) {
    const char *who = "tfhe_hip_new_compressed_cloud_key_seeded";
    if (!mask_seed10) { set_error(std::string(who) + ": null mask seed"); return nullptr; }
    return make_compressed_key(who, secret, &noise_seed, mask_seed10);
}
TfheHipCompressedCloudKey *tfhe_hip_new_compressed_cloud_key_from_words(const TFheGateBootstrappingParameterSet *params,
                                                                        const uint32_t *mask_seed10, const Torus32 *bk_body,
                                                                        const Torus32 *ksk_body) {
    const char *who = "tfhe_hip_new_compressed_cloud_key_from_words";
    if (!params || !params->in_out_params || !mask_seed10 || !bk_body || !ksk_body) { set_error(std::string(who) + ": null argument"); return nullptr; }
    TfheHipCompressedCloudKey *key = new_compressed_object(who, params_of(params));
    if (!key) return nullptr;
    std::memcpy(key->seed, mask_seed10, sizeof key->seed);
    key->bk_body.assign(bk_body, bk_body + key->p.bk_body_words());
    key->ksk_body.assign(ksk_body, ksk_body + key->p.ksk_body_words());
    return key;
}
void tfhe_hip_delete_compressed_cloud_key(TfheHipCompressedCloudKey *key) {
    if (!key) return;
    if (key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_delete_compressed_cloud_key: not a compressed cloud key (or already deleted)"); return; }
    key->magic = 0;
    delete key;
}

const uint32_t *tfhe_hip_compressed_key_seed(const TfheHipCompressedCloudKey *key) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_compressed_key_seed: null or deleted compressed cloud key"); return nullptr; }
    return key->seed;
}
const Torus32 *tfhe_hip_compressed_key_bk_body(const TfheHipCompressedCloudKey *key, int64_t *count) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_compressed_key_bk_body: null or deleted compressed cloud key"); if (count) *count = 0; return nullptr; }
    if (count) *count = (int64_t)key->bk_body.size();
    return key->bk_body.data();
}
const Torus32 *tfhe_hip_compressed_key_ksk_body(const TfheHipCompressedCloudKey *key, int64_t *count) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_compressed_key_ksk_body: null or deleted compressed cloud key"); if (count) *count = 0; return nullptr; }
    if (count) *count = (int64_t)key->ksk_body.size();
    return key->ksk_body.data();
}
int64_t tfhe_hip_compressed_key_bytes(const TfheHipCompressedCloudKey *key) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_compressed_key_bytes: null or deleted compressed cloud key"); return -1; }
    return (int64_t)(sizeof key->seed + (key->bk_body.size() + key->ksk_body.size()) * sizeof(Torus32));
}

TFheGateBootstrappingCloudKeySet *tfhe_hip_expand_cloud_key_host(const TfheHipCompressedCloudKey *key) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_expand_cloud_key_host: null or deleted compressed cloud key"); return nullptr; }
    auto *ck = new TfheHipCloudKey();
    ck->p = key->p;
    expand_masks_host(key->p, key->seed, key->bk_body.data(), key->ksk_body.data(), ck->bk, ck->ksk);
    return io_adopt_cloud(ck);
}
TFheGateBootstrappingCloudKeySet *tfhe_hip_expand_cloud_key(const TfheHipCompressedCloudKey *key) {
    if (!key || key->magic != COMPRESSED_KEY_MAGIC) { set_error("tfhe_hip_expand_cloud_key: null or deleted compressed cloud key"); return nullptr; }
    auto *ck = new TfheHipCloudKey();
    ck->p = key->p;
    ck->mask_seed.assign(key->seed, key->seed + 10);
    ck->bk_body = key->bk_body;
    ck->ksk_body = key->ksk_body;
    return io_adopt_cloud(ck);
}

int tfhe_hip_kernel_expand_masks(const uint32_t *mask_seed10, int64_t first_word, int32_t count, uint32_t *out) {
    return guarded_rc([&] {
        if (!mask_seed10 || !out) api_fail("tfhe_hip_kernel_expand_masks: null argument");
        if (first_word < 0 || (first_word >> 60) || count < 1 || count > EXPAND_MASKS_MAX)
            api_fail("tfhe_hip_kernel_expand_masks: first_word must be in 0 .. 2^60 - 1 and count in 1 .. 2^24");
        auto g = recorder_lock();
        Engine::get().run_expand_masks(mask_seed10, first_word, count, out);
        return 0;
    });
}
int64_t tfhe_hip_test_key_image(const TFheGateBootstrappingCloudKeySet *cloud, int which, Torus32 *out, int64_t capacity) {
    int64_t words = -1;
    guarded([&] {
        if (!cloud || !cloud->bk || (which != 0 && which != 1) || capacity < 0) api_fail("tfhe_hip_test_key_image: bad arguments");
        auto g = recorder_lock();
        pool_of_key(cloud);
        words = (int64_t)Engine::get().read_key_image(cloud->bk->dev, which, out, (size_t)capacity);
    });
    return words;
}
double tfhe_hip_last_expand_ms(void) {
    auto g = recorder_lock();
    return Engine::get().last_expand_ms;
}

}  // extern "C"
