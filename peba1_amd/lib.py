"""ctypes loader for libtfhe-hip.so (the C-ABI drop-in boundary, include/*.h).

The library is the product: it fails loudly if the shared object is missing and
the library itself aborts if no HIP device is present when a gate is evaluated.
There is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PEBA1_TFHE_HIP_LIB: another build of the same library (tools/diag/build_variants.sh: A/B runs of kernel variants on one
# box); it must exist like the default one -- there is no fallback either way
LIB_PATH = os.environ.get("PEBA1_TFHE_HIP_LIB") or os.path.join(_HERE, "libtfhe-hip.so")
CIRCUITS_PATH = os.path.join(_HERE, "libpeba1-circuits.so")


class LweSample(C.Structure):
    _fields_ = [("a", C.POINTER(C.c_int32)), ("b", C.c_int32), ("slot", C.c_int32),
                ("current_variance", C.c_double)]


class LweParams(C.Structure):
    _fields_ = [("n", C.c_int32), ("alpha_min", C.c_double), ("alpha_max", C.c_double)]


class TLweParams(C.Structure):
    _fields_ = [("N", C.c_int32), ("k", C.c_int32), ("alpha_min", C.c_double), ("alpha_max", C.c_double)]


class TGswParams(C.Structure):
    _fields_ = [("l", C.c_int32), ("Bgbit", C.c_int32), ("Bg", C.c_int32), ("halfBg", C.c_int32),
                ("maskMod", C.c_uint32), ("tlwe_params", C.POINTER(TLweParams)), ("kpl", C.c_int32),
                ("offset", C.c_uint32)]


class ParameterSet(C.Structure):
    _fields_ = [("ks_t", C.c_int32), ("ks_basebit", C.c_int32), ("in_out_params", C.POINTER(LweParams)),
                ("tgsw_params", C.POINTER(TGswParams))]


class CloudKeySet(C.Structure):
    _fields_ = [("params", C.POINTER(ParameterSet)), ("bk", C.c_void_p), ("bkFFT", C.c_void_p)]


class SecretKeySet(C.Structure):
    _fields_ = [("params", C.POINTER(ParameterSet)), ("lwe_key", C.c_void_p), ("tgsw_key", C.c_void_p),
                ("cloud", CloudKeySet)]


class Stats(C.Structure):
    """TfheHipStats up to multi_outputs.  The header only ever appends fields, so this stays a prefix of the struct;
    StatsAll and StatsWhole below append what came since, StatsWhole being the whole of it."""
    _fields_ = [("blind_rotates", C.c_uint64), ("keyswitches", C.c_uint64), ("linear_ops", C.c_uint64),
                ("levels", C.c_uint64), ("flushes", C.c_uint64), ("br_launches", C.c_uint64),
                ("ms_blind_rotate", C.c_double), ("ms_keyswitch", C.c_double), ("ms_flush_wall", C.c_double),
                ("ms_blind_rotate_busy", C.c_double), ("reused_gates", C.c_uint64),
                ("br8_launches", C.c_uint64), ("br8_rotations", C.c_uint64), ("ms_blind_rotate8", C.c_double),
                ("clk_shader_cycles", C.c_uint64), ("clk_ref_ticks", C.c_uint64), ("dead_gates", C.c_uint64),
                ("folded_gates", C.c_uint64),
                ("br_wide4_launches", C.c_uint64), ("br_split_launches", C.c_uint64),
                ("br_wave8_launches", C.c_uint64), ("br_wave2_launches", C.c_uint64),
                ("br_tables0_launches", C.c_uint64), ("br_tables1_launches", C.c_uint64),
                ("br_tables2_launches", C.c_uint64), ("lut_rotations", C.c_uint64),
                ("multi_rotations", C.c_uint64), ("multi_outputs", C.c_uint64)]


class StatsAll(Stats):
    """TfheHipStats up to ks_index_launches: ctypes lays a subclass's fields out behind its base's, as the header appended
    them (every field is 8 bytes wide: no padding in between).  STATS_FIELDS names these; StatsWhole below is the whole
    struct, what tfhe_hip_get_stats fills."""
    _fields_ = [("lincomb_ops", C.c_uint64), ("lincomb_launches", C.c_uint64),
                ("ks_pergate_launches", C.c_uint64), ("ks_strip_launches", C.c_uint64), ("ks_index_launches", C.c_uint64)]


class StatsWhole(StatsAll):
    """The whole of TfheHipStats: the counters of the ring-encrypted inputs stand at its end.  api.stats() reads this and
    returns STATS_FIELDS, api.unpack_stats() the two below."""
    _fields_ = [("unpacked_samples", C.c_uint64), ("unpack_launches", C.c_uint64)]


class ExpandStats(C.Structure):
    """TfheHipExpandStats: the counters of the seed-compressed cloud keys, read through an entry of their own
    (tfhe_hip_get_expand_stats) -- TfheHipStats, which callers allocate, keeps its size."""
    _fields_ = [("expanded_keys", C.c_uint64), ("expand_launches", C.c_uint64)]


class KsMatrixStats(C.Structure):
    """TfheHipKsMatrixStats: launches of the matrix key switch (tfhe_hip_get_ks_matrix_stats)."""
    _fields_ = [("ks_matrix_launches", C.c_uint64)]


class SeededStats(C.Structure):
    """TfheHipSeededStats: device-expanded packing keys and seeded unpacks (tfhe_hip_get_seeded_stats)."""
    _fields_ = [("expanded_packing_keys", C.c_uint64), ("packing_expand_launches", C.c_uint64),
                ("seeded_unpacked_samples", C.c_uint64), ("seeded_unpack_launches", C.c_uint64)]


class SeededLweStats(C.Structure):
    """TfheHipSeededLweStats: seeded imports of LWE sample arrays (tfhe_hip_get_seeded_lwe_stats)."""
    _fields_ = [("seeded_imported_samples", C.c_uint64), ("seeded_import_launches", C.c_uint64)]


STATS_FIELDS = [f for f, _ in Stats._fields_] + [f for f, _ in StatsAll._fields_]
UNPACK_STATS_FIELDS = [f for f, _ in StatsWhole._fields_]
EXPAND_STATS_FIELDS = [f for f, _ in ExpandStats._fields_]
SEEDED_STATS_FIELDS = [f for f, _ in SeededStats._fields_]
SEEDED_LWE_STATS_FIELDS = [f for f, _ in SeededLweStats._fields_]


PS = C.POINTER(ParameterSet)
CK = C.POINTER(CloudKeySet)
SK = C.POINTER(SecretKeySet)
LS = C.POINTER(LweSample)
I32P = C.POINTER(C.c_int32)
U32P = C.POINTER(C.c_uint32)

# every symbol include/tfhe/tfhe_gate_bootstrapping_functions.h and include/tfhe_hip.h declare
_GATE2 = ["bootsAND", "bootsOR", "bootsXOR", "bootsXNOR", "bootsNAND", "bootsNOR", "bootsANDNY", "bootsANDYN",
          "bootsORNY", "bootsORYN"]
SIGNATURES = {
    "new_gate_bootstrapping_ciphertext_array": (LS, [C.c_int32, PS]),
    "delete_gate_bootstrapping_ciphertext_array": (None, [C.c_int32, LS]),
    "new_gate_bootstrapping_ciphertext": (LS, [PS]),
    "delete_gate_bootstrapping_ciphertext": (None, [LS]),
    "bootsCONSTANT": (None, [LS, C.c_int32, CK]),
    "bootsNOT": (None, [LS, LS, CK]),
    "bootsCOPY": (None, [LS, LS, CK]),
    "bootsMUX": (None, [LS, LS, LS, LS, CK]),
    "new_default_gate_bootstrapping_parameters": (PS, [C.c_int32]),
    "new_random_gate_bootstrapping_secret_keyset": (SK, [PS]),
    "delete_gate_bootstrapping_parameters": (None, [PS]),
    "delete_gate_bootstrapping_secret_keyset": (None, [SK]),
    "delete_gate_bootstrapping_cloud_keyset": (None, [CK]),
    "bootsSymEncrypt": (None, [LS, C.c_int32, SK]),
    "bootsSymDecrypt": (C.c_int32, [LS, SK]),
    "modSwitchFromTorus32": (C.c_int32, [C.c_int32, C.c_int32]),
    "modSwitchToTorus32": (C.c_int32, [C.c_int32, C.c_int32]),
    "export_tfheGateBootstrappingParameterSet_toFile": (None, [C.c_void_p, PS]),
    "new_tfheGateBootstrappingParameterSet_fromFile": (PS, [C.c_void_p]),
    "export_tfheGateBootstrappingCloudKeySet_toFile": (None, [C.c_void_p, CK]),
    "new_tfheGateBootstrappingCloudKeySet_fromFile": (CK, [C.c_void_p]),
    "export_tfheGateBootstrappingSecretKeySet_toFile": (None, [C.c_void_p, SK]),
    "new_tfheGateBootstrappingSecretKeySet_fromFile": (SK, [C.c_void_p]),
    "export_gate_bootstrapping_ciphertext_toFile": (None, [C.c_void_p, LS, PS]),
    "import_gate_bootstrapping_ciphertext_fromFile": (None, [C.c_void_p, LS, PS]),
    "tfhe_hip_test_wg_times": (C.c_int, [CK, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "tfhe_hip_last_error": (C.c_char_p, []),
    "tfhe_hip_clear_error": (None, []),
    "tfhe_hip_set_device": (C.c_int, [C.c_int]),
    "tfhe_hip_get_device": (C.c_int, []),
    "tfhe_hip_device_pci_bus_id": (C.c_int, [C.c_char_p, C.c_int]),
    "tfhe_hip_new_parameters": (PS, [C.c_int32] * 7 + [C.c_double] * 3),
    "tfhe_hip_new_p2048_parameters": (PS, []),
    "tfhe_hip_new_secret_keyset_seeded": (SK, [PS, C.c_uint64]),
    "tfhe_hip_new_secret_keyset_seeded_host": (SK, [PS, C.c_uint64]),
    "tfhe_hip_set_encrypt_seed": (None, [C.c_uint64]),
    "tfhe_hip_randomness_is_seeded": (C.c_int, []),
    "tfhe_hip_test_chacha20_block": (None, [C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tfhe_hip_key_lwe": (I32P, [SK, C.POINTER(C.c_int64)]),
    "tfhe_hip_key_tlwe": (I32P, [SK, C.POINTER(C.c_int64)]),
    "tfhe_hip_key_bk": (I32P, [CK, C.POINTER(C.c_int64)]),
    "tfhe_hip_key_ksk": (I32P, [CK, C.POINTER(C.c_int64)]),
    "tfhe_hip_sample_words": (C.c_int32, [PS]),
    "tfhe_hip_export_samples": (C.c_int, [LS, C.c_int32, PS, I32P]),
    "tfhe_hip_import_samples": (C.c_int, [LS, C.c_int32, PS, I32P]),
    "tfhe_hip_export_samples_device": (C.c_int, [LS, C.c_int32, PS, C.c_void_p]),
    "tfhe_hip_import_samples_device": (C.c_int, [LS, C.c_int32, PS, C.c_void_p]),
    "tfhe_hip_export_samples_device_async": (C.c_int, [LS, C.c_int32, PS, C.c_void_p]),
    "tfhe_hip_import_samples_device_async": (C.c_int, [LS, C.c_int32, PS, C.c_void_p]),
    "tfhe_hip_stream": (C.c_void_p, []),
    "tfhe_hip_sync_samples": (C.c_int, [LS, C.c_int32]),
    "tfhe_hip_set_deferred": (None, [C.c_int]),
    "tfhe_hip_get_deferred": (C.c_int, []),
    "tfhe_hip_flush": (C.c_int, []),
    "tfhe_hip_flush_async": (C.c_int, []),
    "tfhe_hip_wait": (C.c_int, []),
    "tfhe_hip_stream_sync": (C.c_int, []),
    "tfhe_hip_wait_event": (C.c_int, [C.c_void_p, C.c_char_p]),
    "tfhe_hip_set_diag_label": (None, [C.c_char_p]),
    "tfhe_hip_gate_batch": (C.c_int, [C.c_int, LS, LS, LS, C.c_int32, CK]),
    "tfhe_hip_gate3": (None, [C.c_int, C.c_int, LS, LS, LS, LS, CK]),
    "tfhe_hip_gate3_batch": (C.c_int, [C.c_int, C.c_int, LS, LS, LS, LS, C.c_int32, CK]),
    "tfhe_hip_new_lut": (C.c_void_p, [PS, I32P]),
    "tfhe_hip_new_lut_constant": (C.c_void_p, [PS, C.c_int32]),
    "tfhe_hip_new_lut_from_table": (C.c_void_p, [PS, I32P, C.c_int32]),
    "tfhe_hip_delete_lut": (None, [C.c_void_p]),
    "tfhe_hip_lut_words": (I32P, [C.c_void_p, I32P]),
    "tfhe_hip_lut_bootstrap": (None, [C.c_void_p, LS, C.c_int32, C.POINTER(LS), I32P, C.c_int32, CK]),
    "tfhe_hip_lut_bootstrap_batch": (C.c_int, [C.c_void_p, LS, C.c_int32, C.POINTER(LS), I32P, C.c_int32, C.c_int32, CK]),
    "tfhe_hip_new_lut_multi": (C.c_void_p, [C.c_void_p, C.c_int32, I32P, I32P, I32P, I32P]),
    "tfhe_hip_new_lut_multi_from_tables": (C.c_void_p, [PS, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_delete_lut_multi": (None, [C.c_void_p]),
    "tfhe_hip_lut_multi_nout": (C.c_int32, [C.c_void_p]),
    "tfhe_hip_lut_multi_output": (C.c_int32, [C.c_void_p, C.c_int32, I32P, I32P, I32P]),
    "tfhe_hip_lut_multi_words": (I32P, [C.c_void_p, I32P]),
    "tfhe_hip_lut_bootstrap_multi": (None, [C.c_void_p, C.POINTER(LS), C.c_int32, C.POINTER(LS), I32P, C.c_int32, CK]),
    "tfhe_hip_lut_bootstrap_multi_batch": (C.c_int, [C.c_void_p, C.POINTER(LS), C.c_int32, C.POINTER(LS), I32P, C.c_int32,
                                                     C.c_int32, CK]),
    "tfhe_hip_linear": (None, [LS, C.c_int32, C.POINTER(LS), I32P, C.c_int32, CK]),
    "tfhe_hip_linear_batch": (C.c_int, [LS, C.c_int32, C.POINTER(LS), I32P, C.c_int32, C.c_int32, CK]),
    "tfhe_hip_sym_encrypt_torus": (None, [LS, C.c_int32, SK]),
    "tfhe_hip_sym_phase": (C.c_int32, [LS, SK]),
    "tfhe_hip_set_tuning": (C.c_int, [C.c_char_p, C.c_int64]),
    "tfhe_hip_test_form_admissible": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int]),
    "tfhe_hip_test_set_alloc_cap": (None, [C.c_int64]),
    "tfhe_hip_test_alloc_held": (C.c_int64, []),
    "tfhe_hip_test_stage_place": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "tfhe_hip_get_stats": (None, [C.POINTER(StatsWhole)]),
    "tfhe_hip_reset_stats": (None, []),
    "tfhe_hip_set_kernel_timing": (None, [C.c_int]),
    "tfhe_hip_last_flush_keys": (C.c_int, []),
    "tfhe_hip_set_batch_keys": (C.c_int, [C.c_int]),
    "tfhe_hip_test_schedule": (C.c_int, [I32P, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_test_level_plan": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [I32P] * 9),
    "tfhe_hip_test_level_plan3": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [I32P] * 9),
    "tfhe_hip_test_level_plan_lut": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [I32P] * 10),
    "tfhe_hip_test_level_plan_multi": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, I32P,
                                                 C.c_int32] + [I32P] * 10),
    "tfhe_hip_test_level_plan_lin": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, I32P,
                                               C.c_int32, I32P, C.c_int32] + [I32P] * 16),
    "tfhe_hip_test_level_plan_full": (C.c_int, [I32P, I32P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, I32P,
                                                C.c_int32, I32P, C.c_int32] + [I32P] * 18),
    "tfhe_hip_test_level_slack": (C.c_int, [I32P, C.c_int32, C.c_int32, C.c_int32, I32P, C.POINTER(C.c_double), C.c_int32, C.c_int32, I32P,
                                            I32P, C.POINTER(C.c_double)]),
    "tfhe_hip_test_level_cost": (C.c_int, [C.c_int32] * 9 + [C.POINTER(C.c_double)]),
    "tfhe_hip_test_set_level_cost": (C.c_int, [I32P, C.POINTER(C.c_double), C.c_int32]),
    "tfhe_hip_last_level_slack": (C.c_int, [C.POINTER(C.c_double)]),     # out4
    "tfhe_hip_test_br_plan": (C.c_int, [C.c_int32] * 3 + [I32P, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_test_ks_plan": (C.c_int, [C.c_int32] * 5 + [I32P, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "tfhe_hip_test_ks_plan_form": (C.c_int, [C.c_int32] * 5 + [I32P, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "tfhe_hip_kernel_negacyclic":(C.c_int, [CK, I32P, I32P, I32P, C.c_int32]),
    "tfhe_hip_kernel_bootstrap_woks": (C.c_int, [CK, I32P, C.c_int32, I32P, I32P]),
    "tfhe_hip_kernel_lut_bootstrap_woks": (C.c_int, [CK, I32P, C.c_int32, I32P, I32P, C.c_int32, I32P, I32P]),
    "tfhe_hip_kernel_lut_bootstrap_multi_woks": (C.c_int, [CK, I32P, C.c_int32, I32P, I32P, C.c_int32, I32P, I32P, C.c_int32,
                                                           I32P, I32P]),
    "tfhe_hip_kernel_keyswitch": (C.c_int, [CK, I32P, C.c_int32, I32P]),
    "tfhe_hip_kernel_keyswitch_matrix": (C.c_int, [CK, I32P, C.c_int32, I32P]),
    "tfhe_hip_test_ks_plan_form2": (C.c_int, [C.c_int32] * 5 + [I32P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "tfhe_hip_test_ks_byte_planes": (C.c_int, [U32P, C.c_int32, C.POINTER(C.c_int8)]),
    "tfhe_hip_new_packing_key": (C.c_void_p, [SK, C.c_int32, C.c_int32]),
    "tfhe_hip_new_packing_key_seeded": (C.c_void_p, [SK, C.c_int32, C.c_int32, C.c_uint64]),
    "tfhe_hip_new_packing_key_from_words": (C.c_void_p, [PS, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_delete_packing_key": (None, [C.c_void_p]),
    "tfhe_hip_packing_key_words": (I32P, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfhe_hip_packing_key_decomposition": (C.c_int, [C.c_void_p, I32P, I32P]),
    "tfhe_hip_pack_samples": (C.c_int, [C.c_void_p, LS, C.c_int32, CK, I32P]),
    "tfhe_hip_pack_samples_device": (C.c_int, [C.c_void_p, LS, C.c_int32, CK, C.c_void_p]),
    "tfhe_hip_packed_phase": (C.c_int, [SK, I32P, I32P]),
    "tfhe_hip_packed_decrypt_bits": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_test_pack_bounds": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tfhe_hip_kernel_pack": (C.c_int, [C.c_void_p, CK, I32P, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_ring_encrypt": (C.c_int, [SK, I32P, I32P]),
    "tfhe_hip_ring_encrypt_seeded": (C.c_int, [SK, I32P, I32P, C.c_uint64]),
    "tfhe_hip_ring_encrypt_bits": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_ring_encrypt_bits_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, C.c_uint64]),
    "tfhe_hip_unpack_samples": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_unpack_samples_scattered": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, C.POINTER(LS)]),
    "tfhe_hip_unpack_samples_device": (C.c_int, [CK, C.c_void_p, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_extract": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_new_compressed_cloud_key": (C.c_void_p, [SK]),
    "tfhe_hip_new_compressed_cloud_key_seeded": (C.c_void_p, [SK, C.c_uint64, U32P]),
    "tfhe_hip_new_compressed_cloud_key_from_words": (C.c_void_p, [PS, U32P, I32P, I32P]),
    "tfhe_hip_delete_compressed_cloud_key": (None, [C.c_void_p]),
    "tfhe_hip_compressed_key_seed": (U32P, [C.c_void_p]),
    "tfhe_hip_compressed_key_bk_body": (I32P, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfhe_hip_compressed_key_ksk_body": (I32P, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfhe_hip_compressed_key_bytes": (C.c_int64, [C.c_void_p]),
    "tfhe_hip_expand_cloud_key_host": (CK, [C.c_void_p]),
    "tfhe_hip_expand_cloud_key": (CK, [C.c_void_p]),
    "tfhe_hip_export_compressed_cloud_key_toFile": (None, [C.c_void_p, C.c_void_p]),
    "tfhe_hip_new_compressed_cloud_key_fromFile": (C.c_void_p, [C.c_void_p]),
    "tfhe_hip_kernel_expand_masks": (C.c_int, [U32P, C.c_int64, C.c_int32, U32P]),
    "tfhe_hip_test_key_image": (C.c_int64, [CK, C.c_int, I32P, C.c_int64]),
    "tfhe_hip_last_expand_ms": (C.c_double, []),
    "tfhe_hip_get_expand_stats": (None, [C.POINTER(ExpandStats)]),
    "tfhe_hip_get_ks_matrix_stats": (None, [C.POINTER(KsMatrixStats)]),
    "tfhe_hip_get_seeded_stats": (None, [C.POINTER(SeededStats)]),
    "tfhe_hip_new_compressed_packing_key": (C.c_void_p, [SK, C.c_int32, C.c_int32]),
    "tfhe_hip_new_compressed_packing_key_seeded": (C.c_void_p, [SK, C.c_int32, C.c_int32, C.c_uint64, U32P]),
    "tfhe_hip_new_compressed_packing_key_from_words": (C.c_void_p, [PS, C.c_int32, C.c_int32, U32P, I32P]),
    "tfhe_hip_delete_compressed_packing_key": (None, [C.c_void_p]),
    "tfhe_hip_compressed_packing_key_seed": (U32P, [C.c_void_p]),
    "tfhe_hip_compressed_packing_key_body": (I32P, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tfhe_hip_compressed_packing_key_decomposition": (C.c_int, [C.c_void_p, I32P, I32P]),
    "tfhe_hip_compressed_packing_key_bytes": (C.c_int64, [C.c_void_p]),
    "tfhe_hip_expand_packing_key_host": (C.c_void_p, [C.c_void_p]),
    "tfhe_hip_expand_packing_key": (C.c_void_p, [C.c_void_p]),
    "tfhe_hip_export_compressed_packing_key_toFile": (None, [C.c_void_p, C.c_void_p]),
    "tfhe_hip_new_compressed_packing_key_fromFile": (C.c_void_p, [C.c_void_p]),
    "tfhe_hip_ring_encrypt_compressed": (C.c_int, [SK, I32P, I32P]),
    "tfhe_hip_ring_encrypt_compressed_seeded": (C.c_int, [SK, I32P, I32P, U32P, C.c_uint64]),
    "tfhe_hip_ring_encrypt_bits_compressed": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_ring_encrypt_bits_compressed_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, U32P, C.c_uint64]),
    "tfhe_hip_ring_expand_host": (C.c_int, [I32P, C.c_int32, I32P]),
    "tfhe_hip_unpack_samples_seeded": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_unpack_samples_seeded_scattered": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, C.POINTER(LS)]),
    "tfhe_hip_unpack_samples_seeded_device": (C.c_int, [CK, C.c_void_p, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_extract_seeded": (C.c_int, [CK, I32P, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_test_pack_image": (C.c_int64, [C.c_void_p, CK, I32P, C.c_int64]),
    "tfhe_hip_test_extract_rows": (C.c_int64, [I32P, C.c_int64]),
    "tfhe_hip_sym_encrypt_bits_compressed": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_sym_encrypt_bits_compressed_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, U32P, C.c_uint64]),
    "tfhe_hip_sym_encrypt_torus_compressed": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_sym_encrypt_torus_compressed_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, U32P, C.c_uint64]),
    "tfhe_hip_lwe_expand_host": (C.c_int, [I32P, C.c_int32, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_import_samples_seeded": (C.c_int, [PS, I32P, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_import_samples_seeded_scattered": (C.c_int, [PS, I32P, C.c_int32, I32P, C.c_int32, C.POINTER(LS)]),
    "tfhe_hip_import_samples_seeded_device": (C.c_int, [PS, C.c_void_p, C.c_int32, I32P, C.c_int32, LS]),
    "tfhe_hip_kernel_lwe_expand": (C.c_int, [PS, I32P, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_test_expand_slots": (C.c_int64, [I32P, C.c_int64]),
    "tfhe_hip_get_seeded_lwe_stats": (None, [C.POINTER(SeededLweStats)]),
    "tfhe_hip_tgsw_words": (C.c_int64, [PS]),
    "tfhe_hip_tgsw_encrypt_bits": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_tgsw_encrypt_bits_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, C.c_uint64]),
    "tfhe_hip_new_selector": (C.c_void_p, [PS, I32P, C.c_int32]),
    "tfhe_hip_delete_selector": (None, [C.c_void_p]),
    "tfhe_hip_selector_bits": (C.c_int32, [C.c_void_p]),
    "tfhe_hip_ring_select": (C.c_int, [C.c_void_p, I32P, C.c_int32, I32P]),
    "tfhe_hip_ring_select_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfhe_hip_last_select_ms": (C.c_double, []),
    "tfhe_hip_kernel_ring_cmux": (C.c_int, [C.c_void_p, C.c_int32, I32P, I32P, C.c_int32, I32P]),
    "tfhe_hip_test_select_bounds": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "tfhe_hip_ring_lookup": (C.c_int, [C.c_void_p, I32P, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_ring_lookup_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "tfhe_hip_kernel_ring_cmux_rotate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_tgsw_encrypt_polys": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_tgsw_encrypt_polys_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, C.c_uint64]),
    "tfhe_hip_ring_center_words": (C.c_int, [PS, I32P, C.c_int64]),
    "tfhe_hip_ring_inner": (C.c_int, [C.c_void_p, C.c_int32, CK, I32P, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_ring_inner_device": (C.c_int, [C.c_void_p, C.c_int32, CK, C.c_void_p, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_product": (C.c_int, [C.c_void_p, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_kernel_ring_inner_rows": (C.c_int, [C.c_void_p, C.c_int32, I32P, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_new_public_gallery": (C.c_void_p, [PS, I32P, C.c_int32]),
    "tfhe_hip_delete_public_gallery": (None, [C.c_void_p]),
    "tfhe_hip_public_gallery_polys": (C.c_int32, [C.c_void_p]),
    "tfhe_hip_ring_mul_public": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_ring_mul_public_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "tfhe_hip_ring_inner_public": (C.c_int, [C.c_void_p, CK, I32P, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_ring_inner_public_device": (C.c_int, [C.c_void_p, CK, C.c_void_p, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_public_product": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, I32P, C.c_int32, I32P]),
    "tfhe_hip_kernel_ring_public_rows": (C.c_int, [C.c_void_p, I32P, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_test_public_bounds": (C.c_int, [C.c_int32, C.c_int32]),
    "tfhe_hip_ring_mul_public_sum": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I32P, I32P]),
    "tfhe_hip_ring_mul_public_sum_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "tfhe_hip_ring_inner_public_sum": (C.c_int, [C.c_void_p, CK, I32P, C.c_int32, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_ring_inner_public_sum_device": (C.c_int, [C.c_void_p, CK, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_public_sum_product": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I32P, I32P]),
    "tfhe_hip_kernel_ring_public_sum_rows": (C.c_int, [C.c_void_p, I32P, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_test_public_sum_bounds": (C.c_int, [C.c_int32, C.c_int32, C.c_int64]),
    "tfhe_hip_ring_inner_sum_max_terms": (C.c_int32, [PS]),
    "tfhe_hip_ring_mul_tgsw_sum": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I32P, I32P]),
    "tfhe_hip_ring_mul_tgsw_sum_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "tfhe_hip_ring_inner_sum": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, CK, I32P, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_ring_inner_sum_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, CK, C.c_void_p, C.c_int32, C.c_int32, LS]),
    "tfhe_hip_kernel_ring_inner_sum_product": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I32P, I32P]),
    "tfhe_hip_kernel_ring_inner_sum_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, I32P, C.c_int32, C.c_int32, C.c_int32, I32P]),
    "tfhe_hip_test_inner_sum_bounds": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tfhe_hip_test_inner_sum_block_rows": (C.c_int32, [C.c_int32]),
    "tfhe_hip_ring_blind_rotate": (C.c_int, [CK, I32P, C.c_int32, I32P, LS, C.c_int32, I32P]),
    "tfhe_hip_ring_blind_rotate_device": (C.c_int, [CK, C.c_void_p, C.c_int32, I32P, LS, C.c_int32, C.c_void_p]),
    "tfhe_hip_ring_lut_bootstrap": (C.c_int, [CK, I32P, C.c_int32, I32P, LS, C.c_int32, LS]),
    "tfhe_hip_ring_lut_bootstrap_device": (C.c_int, [CK, C.c_void_p, C.c_int32, I32P, LS, C.c_int32, LS]),
    "tfhe_hip_last_ring_rotate_ms": (C.c_double, []),
    "tfhe_hip_kernel_ring_rotate": (C.c_int, [CK, I32P, C.c_int32, I32P, I32P, C.c_int32, I32P, I32P]),
    "tfhe_hip_test_ntt_bounds": (C.c_int, [C.c_int32, C.c_double, C.POINTER(C.c_double), I32P, C.POINTER(C.c_double)]),
    "tfhe_hip_tgsw_compressed_words": (C.c_int64, [PS, C.c_int32]),
    "tfhe_hip_tgsw_encrypt_bits_compressed": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_tgsw_encrypt_bits_compressed_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, C.c_uint64]),
    "tfhe_hip_tgsw_encrypt_polys_compressed": (C.c_int, [SK, I32P, C.c_int32, I32P]),
    "tfhe_hip_tgsw_encrypt_polys_compressed_seeded": (C.c_int, [SK, I32P, C.c_int32, I32P, C.c_uint64]),
    "tfhe_hip_tgsw_expand_host": (C.c_int, [PS, I32P, C.c_int32, I32P]),
    "tfhe_hip_new_selector_compressed": (C.c_void_p, [PS, I32P, C.c_int32, C.c_int32]),
    "tfhe_hip_selector_upload_bytes": (C.c_int64, [C.c_void_p]),
}
for _g in _GATE2:
    SIGNATURES[_g] = (None, [LS, LS, LS, CK])
_lib = None


def load():
    """Load libtfhe-hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(peba1_amd has no CPU fallback)")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)   # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib

