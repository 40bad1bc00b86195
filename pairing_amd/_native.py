"""ctypes binding of the HIP library pairing_amd/lib/libpairing_amd.so.

This is the only way the Python package reaches compute: every function
below ends in a HIP kernel on the current device.  There is no CPU fallback;
if the library is missing or fails to load, import raises.

Array convention (numpy uint64, C-contiguous, the ABI layout of
include/pairing_amd.h):
  Fq (n,6)  Fq2 (n,12)  Fq6 (n,36)  Fq12 (n,72)
  G1Affine (n,13)  G2Affine (n,25)  G1 (n,18)  G2 (n,36)  G2Prepared (n,2449)
  Fr / FrRepr (n,4)
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# PA_LIB_PATH: an A/B build of the same sources (tools/curve_variants.sh); default the in-tree library
LIB_PATH = os.environ.get("PA_LIB_PATH") or os.path.join(HERE, "lib", "libpairing_amd.so")

W_FQ, W_FQ2, W_FQ6, W_FQ12 = 6, 12, 36, 72
W_G1A, W_G1, W_G2A, W_G2 = 13, 18, 25, 36
W_G2P = 68 * 3 * 12 + 1
W_FR = 4

PA_OK = 0


class PairingError(RuntimeError):
    """A negative status code from the C ABI (see include/pairing_amd.h)."""


def _share_torch_hip_runtime():
    """Make this library and torch use ONE HIP runtime in the process.

    The torch wheel ships its own libamdhip64.so (soname libamdhip64.so.7,
    loaded by torch's libc10_hip through RPATH $ORIGIN), while
    libpairing_amd.so needs libamdhip64.so.7 from /opt/rocm.  Imported after
    torch, this library binds to torch's runtime by soname; imported before
    it, two runtimes would end up in the process and torch's would find no
    device.  So torch's runtime file is loaded first (without importing
    torch): a later `import torch` then reuses it (same file), and the
    stream handles and device pointers of the device.py layer belong to the
    runtime that launches our kernels.  PA_SYSTEM_HIP=1 keeps /opt/rocm's."""
    if "torch" in sys.modules or os.environ.get("PA_SYSTEM_HIP") == "1":
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def _load():
    _share_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "pairing_amd: HIP library %s is missing -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)" % LIB_PATH)
    return ctypes.CDLL(LIB_PATH)


_lib = _load()
_P = ctypes.c_void_p
_N = ctypes.c_size_t

# Every exported entry point with its argument types (all return int).
_SIGS = {
    "pa_device_count": [ctypes.POINTER(ctypes.c_int)],
    "pa_set_device": [ctypes.c_int],
    "pa_synchronize": [],
    "pa_set_pairing_kernel": [ctypes.c_int],
    "pa_set_decode_kernel": [ctypes.c_int],
    "pa_fq_mul_batch": [_P, _P, _P, _N],
    "pa_fq_square_batch": [_P, _P, _N],
    "pa_fq_add_batch": [_P, _P, _P, _N],
    "pa_fq_sub_batch": [_P, _P, _P, _N],
    "pa_fq_inverse_batch": [_P, _P, _P, _N],
    "pa_fq_from_repr_batch": [_P, _P, _P, _N],
    "pa_fq_into_repr_batch": [_P, _P, _N],
    "pa_fq2_mul_batch": [_P, _P, _P, _N],
    "pa_fq2_square_batch": [_P, _P, _N],
    "pa_fq6_mul_batch": [_P, _P, _P, _N],
    "pa_fq12_mul_batch": [_P, _P, _P, _N],
    "pa_fq12_square_batch": [_P, _P, _N],
    "pa_fq12_inverse_batch": [_P, _P, _P, _N],
    "pa_fq12_frobenius_map_batch": [_P, _P, _N, _N],
    "pa_fq12_cyclotomic_square_batch": [_P, _P, _N],
    "pa_fq12_mul_by_014_batch": [_P, _P, _P, _P, _P, _N],
    "pa_g2_prepare_batch": [_P, _P, _N],
    "pa_miller_loop_batch": [_P, _P, _P, _N],
    "pa_miller_loop_shared_prepared": [_P, _N, _P, _P],
    "pa_multi_miller_loop": [_P, _P, _N, _P],
    "pa_final_exponentiation_batch": [_P, _P, _P, _N],
    "pa_pairing_batch": [_P, _P, _P, _N],
    "pa_g1_batch_normalization": [_P, _N],
    "pa_g1_wnaf_fixed_base": [_P, _P, _N, _P],
    "pa_g1_wnaf_fixed_base_window": [_P, _P, _N, ctypes.c_int, _P],
    "pa_g1_batch_normalization_device": [_P, _N, _P],
    "pa_g1_fixed_base_table_device": [_P, _P, _P, _P],
    "pa_g1_fixed_base_mul_device": [_P, _P, _P, _N, _P],
    "pa_g1_wnaf_fixed_base_device": [_P, _P, _P, _N, _P, _P, _P],
    "pa_g1_wnaf_fixed_base_window_device": [_P, _P, _P, _N, ctypes.c_int, _P, _P, _P],
    "pa_g1_fixed_base_glv_table_device": [_P, _P, _P, _P],
    "pa_g1_fixed_base_glv_mul_device": [_P, _P, _P, _P, _P, _N, _P],
    "pa_fq_mul_batch_device": [_P, _P, _P, _N, _P],
    "pa_fq_mul_batch_soa_device": [_P, _P, _P, _N, _P],
    "pa_miller_loop_fused_batch_device": [_P, _P, _P, _N, _P],
    "pa_pairing_miller_loop_batch_device": [_P, _P, _P, _N, _P],
    "pa_g2_prepare_batch_device": [_P, _P, _N, _P],
    "pa_miller_loop_batch_device": [_P, _P, _P, _N, _P],
    "pa_miller_loop_shared_prepared_device": [_P, _N, _P, _P, _P],
    "pa_final_exponentiation_batch_device": [_P, _P, _P, _N, _P],
    "pa_pairing_batch_device": [_P, _P, _P, _P, _N, _P],
    "pa_g1_decode_batch": [_P, _N, ctypes.c_int, ctypes.c_int, _P, _P],
    "pa_g2_decode_batch": [_P, _N, ctypes.c_int, ctypes.c_int, _P, _P],
    "pa_g1_encode_batch": [_P, _N, ctypes.c_int, _P],
    "pa_g2_encode_batch": [_P, _N, ctypes.c_int, _P],
    "pa_fq_sqrt_batch": [_P, _P, _P, _N],
    "pa_fq2_sqrt_batch": [_P, _P, _P, _N],
    "pa_multi_miller_loop_affine": [_P, _P, _N, _P],
    "pa_multi_pairing": [_P, _P, _N, _P, _P],
    "pa_pairing_batch_multi_gpu": [_P, _P, _P, _N, ctypes.c_int],
    "pa_g1_decode_batch_device": [_P, _N, ctypes.c_int, ctypes.c_int, _P, _P, _P],
    "pa_g2_decode_batch_device": [_P, _N, ctypes.c_int, ctypes.c_int, _P, _P, _P],
    "pa_fr_mul_batch": [_P, _P, _P, _N],
    "pa_fr_square_batch": [_P, _P, _N],
    "pa_fr_add_batch": [_P, _P, _P, _N],
    "pa_fr_sub_batch": [_P, _P, _P, _N],
    "pa_fr_double_batch": [_P, _P, _N],
    "pa_fr_negate_batch": [_P, _P, _N],
    "pa_fr_inverse_batch": [_P, _P, _P, _N],
    "pa_fr_from_repr_batch": [_P, _P, _P, _N],
    "pa_fr_into_repr_batch": [_P, _P, _N],
    "pa_fr_pow_batch": [_P, _P, _N, _P, _N],
    "pa_fr_legendre_batch": [_P, _P, _N],
    "pa_fr_sqrt_batch": [_P, _P, _P, _N],
    "pa_fr_mul_batch_device": [_P, _P, _P, _N, _P],
    "pa_g1_affine_mul_batch": [_P, _P, _P, _N],
    "pa_g2_affine_mul_batch": [_P, _P, _P, _N],
    "pa_g1_mul_assign_batch": [_P, _P, _P, _N],
    "pa_g2_mul_assign_batch": [_P, _P, _P, _N],
    "pa_g1_multiexp": [_P, _P, _N, _P],
    "pa_g2_multiexp": [_P, _P, _N, _P],
    "pa_g1_multiexp_device": [_P, _P, _N, _P, _P, _N, _P],
    "pa_g2_multiexp_device": [_P, _P, _N, _P, _P, _N, _P],
    "pa_g1_msm_bases_prepare": [_P, _N, ctypes.POINTER(_P)],
    "pa_g1_msm_bases_prepare_device": [_P, _N, _P, ctypes.POINTER(_P)],
    "pa_g1_msm_bases_len": [_P],                      # returns size_t (below)
    "pa_g1_msm_bases_in_subgroup": [_P],
    "pa_g1_msm_bases_free": [_P],
    "pa_g1_multiexp_prepared_workspace_bytes": [_P, _N],   # returns size_t (below)
    "pa_g1_multiexp_prepared_device": [_P, _P, _N, _P, _P, _N, _P],
    "pa_g1_multiexp_prepared": [_P, _P, _N, _P],
    "pa_g1_multiexp_prepared_batch_workspace_bytes": [_P, _N, _N],   # returns size_t (below)
    "pa_g1_multiexp_prepared_batch_device": [_P, _P, _N, _N, ctypes.c_uint, _P, _P, _N, _P],
    "pa_g1_multiexp_prepared_batch": [_P, _P, _N, _N, ctypes.c_uint, _P],
    "pa_g2_msm_bases_prepare": [_P, _N, ctypes.POINTER(_P)],
    "pa_g2_msm_bases_prepare_device": [_P, _N, _P, ctypes.POINTER(_P)],
    "pa_g2_msm_bases_len": [_P],                      # returns size_t (below)
    "pa_g2_msm_bases_in_subgroup": [_P],
    "pa_g2_msm_bases_free": [_P],
    "pa_g2_multiexp_prepared_workspace_bytes": [_P, _N],   # returns size_t (below)
    "pa_g2_multiexp_prepared_device": [_P, _P, _N, _P, _P, _N, _P],
    "pa_g2_multiexp_prepared": [_P, _P, _N, _P],
    "pa_g2_multiexp_prepared_batch_workspace_bytes": [_P, _N, _N],   # returns size_t (below)
    "pa_g2_multiexp_prepared_batch_device": [_P, _P, _N, _N, ctypes.c_uint, _P, _P, _N, _P],
    "pa_g2_multiexp_prepared_batch": [_P, _P, _N, _N, ctypes.c_uint, _P],
    "pa_fr_ntt_domain_create": [ctypes.c_uint, ctypes.POINTER(_P)],
    "pa_fr_ntt_domain_free": [_P],                    # returns nothing (below)
    "pa_fr_ntt_domain_log_n": [_P],                   # returns unsigned (below)
    "pa_fr_ntt_domain_bytes": [_P],                   # returns size_t (below)
    "pa_fr_ntt_domain_passes": [_P],                  # returns unsigned (below)
    "pa_fr_ntt_domain_tile_log": [_P],                # returns unsigned (below)
    "pa_fr_ntt_polys_per_workgroup": [_P],            # returns size_t (below)
    "pa_fr_ntt_max_log_n": [],                        # returns unsigned (below)
    "pa_fr_ntt_workspace_bytes": [_P, _N],            # returns size_t (below)
    "pa_fr_ntt": [_P, ctypes.c_int, _P, _P, _N],
    "pa_fr_ntt_device": [_P, ctypes.c_int, _P, _P, _N, _P, _N, _P],
    "pa_fr_ntt_quotient_workspace_bytes": [_P, _N],   # returns size_t (below)
    "pa_fr_ntt_quotient": [_P, _P, _P, _P, _P, _N],
    "pa_fr_ntt_quotient_device": [_P, _P, _P, _P, _P, _N, _P, _N, _P],
}
for _g in (1, 2):
    for _op in ("double", "negate", "into_affine", "into_projective"):
        _SIGS["pa_g%d_%s_batch" % (_g, _op)] = [_P, _P, _N]
    for _op in ("add", "add_mixed", "sub", "eq"):
        _SIGS["pa_g%d_%s_batch" % (_g, _op)] = [_P, _P, _P, _N]
    for _op in ("double", "into_affine"):
        _SIGS["pa_g%d_%s_batch_device" % (_g, _op)] = [_P, _P, _N, _P]
    for _op in ("add", "add_mixed", "eq"):
        _SIGS["pa_g%d_%s_batch_device" % (_g, _op)] = [_P, _P, _P, _N, _P]
    _SIGS["pa_g%d_recommended_wnaf_for_scalar" % _g] = [_P]
    _SIGS["pa_g%d_wnaf_fixed_base_exact" % _g] = [_P, _P, _N, ctypes.c_int, _P]
    _SIGS["pa_g%d_wnaf_fixed_scalar_exact" % _g] = [_P, _N, _P, ctypes.c_int, _P]
    _SIGS["pa_g%d_wnaf_fixed_base_exact_device" % _g] = [_P, _P, _P, _N, ctypes.c_int, _P, _N, _P]
    _SIGS["pa_g%d_wnaf_fixed_scalar_exact_device" % _g] = [_P, _N, _P, _P, ctypes.c_int, _P, _N, _P]
    _SIGS["pa_g%d_recommended_wnaf_for_num_scalars" % _g] = [_N]
_SIGS.update({
    "pa_fq2_inverse_batch": [_P, _P, _P, _N],
    "pa_multi_pairing_device": [_P, _P, _N, _P, _P, _P, _P],
    "pa_multi_pairing_batch": [_P, _P, _P, _N, _P, _P, _P],
    "pa_multi_pairing_batch_device": [_P, _P, _P, _N, _P, _P, _P, _P, _P],
    "pa_multi_pairing_batch_workspace_bytes": [_N, _N],   # returns size_t (below)
    "pa_fq2_frobenius_map_batch": [_P, _P, _N, _N],
    "pa_fq6_square_batch": [_P, _P, _N],
    "pa_fq6_inverse_batch": [_P, _P, _P, _N],
    "pa_fq6_frobenius_map_batch": [_P, _P, _N, _N],
    "pa_fq_pow_batch": [_P, _P, _N, _P, _N],
    "pa_fq12_pow_batch": [_P, _P, _N, _P, _N],
    "pa_g2_batch_normalization": [_P, _N],
    "pa_g2_batch_normalization_device": [_P, _N, _P],
    "pa_g2_wnaf_fixed_base": [_P, _P, _N, _P],
    "pa_g2_wnaf_fixed_base_window": [_P, _P, _N, ctypes.c_int, _P],
    "pa_g2_wnaf_fixed_base_device": [_P, _P, _P, _N, _P, _P, _P],
    "pa_g2_wnaf_fixed_base_window_device": [_P, _P, _P, _N, ctypes.c_int, _P, _P, _P],
    "pa_r1cs_create": [_P, _P, _P, _N, _N, ctypes.POINTER(_P)],
    "pa_r1cs_eval_device": [_P, _P, _N, ctypes.c_uint, _P, _P, _P, _P, _N, _P],
    "pa_r1cs_eval": [_P, _P, _N, ctypes.c_uint, _P, _P, _P],
    "pa_r1cs_rows": [_P],                             # these four return size_t (below)
    "pa_r1cs_cols": [_P],
    "pa_r1cs_bytes": [_P],
    "pa_r1cs_eval_workspace_bytes": [_P, _N],
    "pa_groth16_pk_create": [_P, ctypes.c_uint, ctypes.POINTER(_P)],
    "pa_groth16_pk_in_subgroup": [_P],
    "pa_groth16_prove_workspace_bytes": [_P, _P, _N],   # returns size_t (below)
    "pa_groth16_prove_device": [_P, _P, _P, _P, _P, _P, _N, _P, _P, _N, _P],
    "pa_groth16_prove": [_P, _P, _P, _P, _P, _P, _N, _P],
    "pa_groth16_vk_create": [_P, ctypes.POINTER(_P)],
    "pa_groth16_vk_n_public": [_P],                     # these four return size_t (below)
    "pa_groth16_vk_bytes": [_P],
    "pa_groth16_vk_input_sum_workspace_bytes": [_P, _N],
    "pa_groth16_verify_workspace_bytes": [_P, _N],
    "pa_groth16_vk_input_sum_device": [_P, _P, _N, ctypes.c_uint, _N, _P, _P, _N, _P],
    "pa_groth16_vk_input_sum": [_P, _P, _N, ctypes.c_uint, _N, _P],
    "pa_groth16_verify_device": [_P, _P, _P, _N, ctypes.c_uint, _N, _P, _P, _P, _N, _P],
    "pa_groth16_verify": [_P, _P, _P, _N, ctypes.c_uint, _N, _P, _P],
    "pa_groth16_verify_encoded_device": [_P, _P, _P, _N, ctypes.c_uint, _N, _P, _P, _P, _P, _N, _P],
    "pa_groth16_verify_encoded": [_P, _P, _P, _N, ctypes.c_uint, _N, _P, _P, _P],
    "pa_g1_multiexp_u128_workspace_bytes": [_N],                   # these two return size_t (below)
    "pa_groth16_verify_aggregate_workspace_bytes": [_P, _N],
    "pa_g1_multiexp_u128_device": [_P, _P, _N, _P, _P, _N, _P],
    "pa_g1_multiexp_u128": [_P, _P, _N, _P],
    "pa_groth16_verify_aggregate_device": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P, _P, _P, _N, _P],
    "pa_groth16_verify_aggregate": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P, _P],
    "pa_groth16_verify_aggregate_encoded_device": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P, _P, _P, _P, _N, _P],
    "pa_groth16_verify_aggregate_encoded": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P, _P, _P],
    "pa_groth16_verify_aggregate_points_device": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P, _P, _N, _P],
    "pa_groth16_verify_aggregate_points": [_P, _P, _P, _N, ctypes.c_uint, _P, _N, _P],
    "pa_groth16_circuit_create": [_P, _P, _P, _N, _N, _N, ctypes.POINTER(_P)],
    "pa_groth16_circuit_rows": [_P],                    # these seven return size_t (below)
    "pa_groth16_circuit_cols": [_P],
    "pa_groth16_circuit_n_public": [_P],
    "pa_groth16_circuit_bytes": [_P],
    "pa_groth16_generate_g1_len": [_P, ctypes.c_uint],
    "pa_groth16_generate_g2_len": [_P],
    "pa_groth16_generate_workspace_bytes": [_P, ctypes.c_uint],
    "pa_groth16_generate_device": [_P, _P, _P, _P, _P, _P, _P, _P, _N, _P],
    "pa_groth16_generate": [_P, _P, _P, _P, _P, _P, _P],
    "pa_groth16_generate_scalars_device": [_P, _P, _P, _P, _P, _N, _P],
    "pa_groth16_generate_scalars": [_P, _P, _P, _P],
})
for _name, _args in _SIGS.items():
    _fn = getattr(_lib, _name)
    _fn.argtypes = _args
    _fn.restype = ctypes.c_int
_lib.pa_version.restype = ctypes.c_char_p
_lib.pa_g1_fixed_base_table_words.restype = ctypes.c_size_t
_lib.pa_g1_fixed_base_workspace_words.restype = ctypes.c_size_t
_lib.pa_g2_fixed_base_table_words.restype = ctypes.c_size_t
_lib.pa_g2_fixed_base_workspace_words.restype = ctypes.c_size_t
_lib.pa_last_error.restype = ctypes.c_char_p
_lib.pa_multiexp_workspace_bytes.argtypes = [ctypes.c_int, _N]
_lib.pa_multiexp_workspace_bytes.restype = ctypes.c_size_t
_lib.pa_wnaf_exact_workspace_bytes.argtypes = [ctypes.c_int, _N, ctypes.c_int, ctypes.c_int]
_lib.pa_wnaf_exact_workspace_bytes.restype = ctypes.c_size_t
for _g in (1, 2):
    for _name in ("msm_bases_len", "multiexp_prepared_workspace_bytes", "multiexp_prepared_batch_workspace_bytes"):
        getattr(_lib, "pa_g%d_%s" % (_g, _name)).restype = ctypes.c_size_t
_lib.pa_multi_pairing_batch_workspace_bytes.restype = ctypes.c_size_t
_lib.pa_fr_ntt_domain_free.restype = None
for _name in ("pa_fr_ntt_domain_log_n", "pa_fr_ntt_domain_passes", "pa_fr_ntt_domain_tile_log", "pa_fr_ntt_max_log_n"):
    getattr(_lib, _name).restype = ctypes.c_uint
for _name in ("pa_fr_ntt_domain_bytes", "pa_fr_ntt_polys_per_workgroup", "pa_fr_ntt_workspace_bytes",
              "pa_fr_ntt_quotient_workspace_bytes"):
    getattr(_lib, _name).restype = ctypes.c_size_t
for _name in ("pa_r1cs_rows", "pa_r1cs_cols", "pa_r1cs_bytes", "pa_r1cs_eval_workspace_bytes", "pa_r1cs_chunk_len",
              "pa_groth16_prove_workspace_bytes", "pa_groth16_vk_n_public", "pa_groth16_vk_bytes",
              "pa_groth16_vk_input_sum_workspace_bytes", "pa_groth16_verify_workspace_bytes",
              "pa_g1_multiexp_u128_workspace_bytes", "pa_groth16_verify_aggregate_workspace_bytes",
              "pa_groth16_circuit_rows", "pa_groth16_circuit_cols", "pa_groth16_circuit_n_public",
              "pa_groth16_circuit_bytes", "pa_groth16_generate_g1_len", "pa_groth16_generate_g2_len",
              "pa_groth16_generate_workspace_bytes"):
    getattr(_lib, _name).restype = ctypes.c_size_t
_lib.pa_r1cs_chunk_len.argtypes = []
for _name in ("pa_r1cs_free", "pa_groth16_pk_free", "pa_groth16_vk_free", "pa_groth16_circuit_free"):
    getattr(_lib, _name).argtypes = [_P]
    getattr(_lib, _name).restype = None


def version():
    return _lib.pa_version().decode()


def _check(rc, what):
    if rc != PA_OK:
        raise PairingError("%s failed (%d): %s" % (what, rc, _lib.pa_last_error().decode()))


def call(name, *args):
    _check(getattr(_lib, name)(*args), name)


def device_count():
    c = ctypes.c_int(0)
    rc = _lib.pa_device_count(ctypes.byref(c))
    return c.value if rc == PA_OK else 0


def set_pairing_kernel(variant):
    """Pairing kernels: 0 default by batch size (<= 2304 pairs on the
    cooperative kernels: a four-wave quad VM per pairing; <= 32768 a lane pair
    per pairing; <= 34048 one lane per pairing; larger lane pairs), 1 lane pairs, 2
    cooperative for every size, 3 one lane per pairing for every size, 4
    cooperative for every size on the round-2 one-wave VM.  Identical results."""
    call("pa_set_pairing_kernel", int(variant))


def set_decode_kernel(variant):
    """Point-decoding kernels: 0 default by batch size (<= PA_DECODE_QUAD_MAX
    records: one record per group of lane quads, the latency form), 1 one lane
    per record, 2 quad groups for every size.  Identical results."""
    call("pa_set_decode_kernel", int(variant))


def set_device(dev):
    call("pa_set_device", dev)


def ptr(a):
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("arrays must be C-contiguous")
    return a.ctypes.data_as(ctypes.c_void_p)


def as_rows(a, width, name="array"):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError("%s must have shape (n, %d), got %s" % (name, width, a.shape))
    return a


def csr_offsets(offsets, n):
    """The CSR offsets of multi_pairing_batch as a host uint64 array: m + 1
    entries from 0 to n (the number of pairs), non-decreasing.  Takes a numpy
    array or a CPU tensor of an integer type; anything else is a ValueError."""
    if getattr(offsets, "is_cuda", False):
        raise ValueError("offsets must be host memory (a numpy array or a CPU tensor)")
    o = np.asarray(offsets)
    if o.ndim != 1 or o.shape[0] < 1 or o.dtype.kind not in "iu":
        raise ValueError("offsets must be a 1-d integer array of m + 1 entries, got %s %s" % (o.dtype, o.shape))
    if o.dtype.kind == "i" and (o < 0).any():
        raise ValueError("offsets must not be negative")
    o = np.ascontiguousarray(o, dtype=np.uint64)
    if int(o[0]) != 0:
        raise ValueError("offsets must start at 0, got %d" % int(o[0]))
    if (o[1:] < o[:-1]).any():
        raise ValueError("offsets must be non-decreasing")
    if int(o[-1]) != int(n):
        raise ValueError("the last offset is %d, the call has %d pairs" % (int(o[-1]), int(n)))
    return o


class _MsmBases:
    """A pa_g{1,2}_msm_bases handle: multiexp bases of one group prepared once on
    one device (include/pairing_amd.h).  `len` and `in_subgroup` are read at
    creation; close() frees the device memory, is idempotent and also runs when
    the object is collected.  Any use after close() raises ValueError before a
    native call.  owns=False wraps a handle someone else frees.  The two groups
    are sibling subclasses: neither passes for the other."""

    GROUP = 0   # 1 or 2: the pa_g{GROUP}_* entries this handle belongs to

    def __init__(self, handle, length, in_subgroup, owns=True):
        self._handle = handle
        self._owns = owns
        self.len = int(length)
        self.in_subgroup = bool(in_subgroup)

    @classmethod
    def _adopt(cls, handle):
        """take ownership of a handle a prepare call just returned"""
        h = ctypes.c_void_p(handle.value)
        return cls(h, getattr(_lib, "pa_g%d_msm_bases_len" % cls.GROUP)(h),
                   getattr(_lib, "pa_g%d_msm_bases_in_subgroup" % cls.GROUP)(h))

    def __len__(self):
        return self.len

    @property
    def closed(self):
        return self._handle is None

    def handle(self):
        if self._handle is None:
            raise ValueError("prepared multiexp bases used after close()")
        return self._handle

    def check_terms(self, m):
        """the handle, after checking that a multiexp over m terms fits"""
        h = self.handle()
        if m > self.len:
            raise ValueError("%d scalars for %d prepared bases" % (m, self.len))
        return h

    def close(self):
        h, self._handle = self._handle, None
        if h is not None and self._owns:
            call("pa_g%d_msm_bases_free" % self.GROUP, h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone
            pass


class G1MsmBases(_MsmBases):
    """prepared G1 bases (pa_g1_msm_bases)"""
    GROUP = 1


class G2MsmBases(_MsmBases):
    """prepared G2 bases (pa_g2_msm_bases)"""
    GROUP = 2


def msm_bases(prepared, cls, maker):
    """`prepared` if it is a live handle of class cls (G1MsmBases or G2MsmBases),
    else a ValueError: another group's handle, a closed one, anything else"""
    if not isinstance(prepared, cls):
        raise ValueError("prepared must come from %s" % maker)
    prepared.handle()   # a closed object is rejected first
    return prepared


MSM_SCALARS_REPR, MSM_SCALARS_MONTGOMERY = 0, 1   # PA_MSM_SCALARS_* of the header


def msm_scalars(montgomery):
    """the PA_MSM_SCALARS_* flag of a batched multiexp: False for FrRepr rows,
    True for Montgomery Fr rows; anything else is a ValueError"""
    if montgomery is True or montgomery is False:
        return MSM_SCALARS_MONTGOMERY if montgomery else MSM_SCALARS_REPR
    raise ValueError("montgomery must be True or False, got %r" % (montgomery,))


def batch_shape(scalars, count, name="scalars"):
    """(rows, k, m) of a batched multiexp's scalars: a (k, m, 4) array, or
    (k * m, 4) rows with count = k vectors end to end"""
    a = np.ascontiguousarray(scalars, dtype=np.uint64)
    if a.ndim == 3 and count is None:
        if a.shape[2] != 4:
            raise ValueError("%s must have shape (k, m, 4), got %s" % (name, a.shape))
        return a.reshape(-1, 4), a.shape[0], a.shape[1]
    if a.ndim != 2 or a.shape[1] != 4 or count is None:
        raise ValueError("%s must have shape (k, m, 4), or (k * m, 4) with count=k, got %s" % (name, a.shape))
    k = int(count)
    if k < 0 or (k == 0 and a.shape[0]) or (k and a.shape[0] % k):
        raise ValueError("%d rows of %s are not %d vectors of equal length" % (a.shape[0], name, k))
    return a, k, a.shape[0] // k if k else 0


NTT_MODES = {"forward": 0, "inverse": 1, "coset_forward": 2, "coset_inverse": 3}   # PA_NTT_* of the header
NTT_MAX_LOG_N = int(_lib.pa_fr_ntt_max_log_n())


def ntt_mode(mode):
    """the PA_NTT_* code of a mode name; anything else is a ValueError"""
    try:
        return NTT_MODES[mode]
    except (KeyError, TypeError):
        raise ValueError("mode must be one of %s, got %r" % (", ".join(NTT_MODES), mode)) from None


class FrNttDomain:
    """A pa_fr_ntt_domain handle: the power tables of one radix-2 evaluation
    domain of 2^log_n points on one device (include/pairing_amd.h).  `log_n`,
    `len` = 2^log_n, `passes`, `tile_log`, `polys_per_workgroup`, `bytes` (device
    memory held) are read at creation;
    close() frees the device memory, is idempotent and also runs when the
    object is collected.  Any use after close() raises ValueError before a
    native call.  owns=False wraps a handle someone else frees."""

    def __init__(self, handle, log_n, owns=True, passes=0, tile_log=0, polys_per_workgroup=0, nbytes=0):
        self._handle = handle
        self._owns = owns
        self.log_n = int(log_n)
        self.len = 1 << self.log_n
        self.passes = int(passes)
        self.tile_log = int(tile_log)
        self.polys_per_workgroup = int(polys_per_workgroup)
        self.bytes = int(nbytes)

    @classmethod
    def _adopt(cls, handle):
        """take ownership of a handle pa_fr_ntt_domain_create just returned"""
        h = ctypes.c_void_p(handle.value)
        return cls(h, _lib.pa_fr_ntt_domain_log_n(h),
                   passes=_lib.pa_fr_ntt_domain_passes(h), tile_log=_lib.pa_fr_ntt_domain_tile_log(h),
                   polys_per_workgroup=_lib.pa_fr_ntt_polys_per_workgroup(h), nbytes=_lib.pa_fr_ntt_domain_bytes(h))

    def __len__(self):
        return self.len

    @property
    def closed(self):
        return self._handle is None

    def handle(self):
        if self._handle is None:
            raise ValueError("NTT domain used after close()")
        return self._handle

    def check_rows(self, rows):
        """(handle, batch) after checking that `rows` is a positive multiple of 2^log_n, or zero rows"""
        h = self.handle()
        if rows % self.len:
            raise ValueError("%d rows are not a multiple of the domain's %d points" % (rows, self.len))
        return h, rows // self.len

    def workspace_bytes(self, batch):
        """pa_fr_ntt_workspace_bytes(domain, batch): 0 for a one-pass domain"""
        return int(_lib.pa_fr_ntt_workspace_bytes(self.handle(), int(batch)))

    def quotient_workspace_bytes(self, batch):
        """pa_fr_ntt_quotient_workspace_bytes(domain, batch): 3 or 6 arrays of batch polynomials, 0 for log_n = 0"""
        return int(_lib.pa_fr_ntt_quotient_workspace_bytes(self.handle(), int(batch)))

    def close(self):
        h, self._handle = self._handle, None
        if h is not None and self._owns:
            _lib.pa_fr_ntt_domain_free(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone
            pass


W_PROOF = W_G1A + W_G2A + W_G1A   # pa_groth16_proof: A (13), B (25), C (13) affine records
R1CS_CHUNK_LEN = int(_lib.pa_r1cs_chunk_len())


class _Handle:
    """A device object of the C ABI behind an opaque pointer: close() frees it, is
    idempotent and also runs when the object is collected; any use after close()
    raises ValueError before a native call.  owns=False wraps a handle someone
    else frees."""

    WHAT = "object"
    FREE = None   # name of the pa_*_free entry

    def __init__(self, handle, owns=True):
        self._handle = handle
        self._owns = owns

    @property
    def closed(self):
        return self._handle is None

    def handle(self):
        if self._handle is None:
            raise ValueError("%s used after close()" % self.WHAT)
        return self._handle

    def close(self):
        h, self._handle = self._handle, None
        if h is not None and self._owns:
            getattr(_lib, self.FREE)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone
            pass


class R1cs(_Handle):
    """A pa_r1cs handle: the matrices A, B, C of a constraint system on one device
    (include/pairing_amd.h).  `rows`, `cols` and `bytes` (device memory held) are
    read at creation."""

    WHAT = "R1CS object"
    FREE = "pa_r1cs_free"

    def __init__(self, handle, rows, cols, nbytes=0, owns=True):
        super().__init__(handle, owns)
        self.rows, self.cols, self.bytes = int(rows), int(cols), int(nbytes)

    @classmethod
    def _adopt(cls, handle):
        """take ownership of a handle pa_r1cs_create just returned"""
        h = ctypes.c_void_p(handle.value)
        return cls(h, _lib.pa_r1cs_rows(h), _lib.pa_r1cs_cols(h), _lib.pa_r1cs_bytes(h))

    def check_eval(self, witness_rows, count, log_n):
        """(handle, k, log_n) of an evaluation: `witness_rows` rows are k = count vectors of `cols` rows (count
        None: as many as the rows hold), and 2^log_n covers the system's rows"""
        h = self.handle()
        log_n = int(log_n)
        if log_n < 0 or log_n > NTT_MAX_LOG_N:
            raise ValueError("log_n must be 0..%d, got %d" % (NTT_MAX_LOG_N, log_n))
        if (1 << log_n) < self.rows:
            raise ValueError("2^%d points do not hold the system's %d rows" % (log_n, self.rows))
        if count is None:
            if self.cols == 0:
                raise ValueError("a system of no columns needs count=k")
            count = witness_rows // self.cols
        k = int(count)
        if k < 0 or witness_rows != k * self.cols:
            raise ValueError("%d witness rows are not %d vectors of %d" % (witness_rows, k, self.cols))
        return h, k, log_n

    def eval_workspace_bytes(self, k):
        """pa_r1cs_eval_workspace_bytes(r, k): the partial sums of the rows of several chunks"""
        return int(_lib.pa_r1cs_eval_workspace_bytes(self.handle(), int(k)))


class Groth16Pk(_Handle):
    """A pa_groth16_pk handle: a proving key's five query sets prepared for the
    multiexps, and alpha, beta, delta, on one device.  `log_n`, `n_vars`,
    `n_public`, `h_len` are what it was created with; `in_subgroup` says whether
    all five sets passed their membership test."""

    WHAT = "Groth16 key"
    FREE = "pa_groth16_pk_free"

    def __init__(self, handle, log_n, n_vars, n_public, h_len, in_subgroup=True, owns=True):
        super().__init__(handle, owns)
        self.log_n, self.n_vars, self.n_public, self.h_len = int(log_n), int(n_vars), int(n_public), int(h_len)
        self.in_subgroup = bool(in_subgroup)

    def check_prove(self, r1cs, domain, witness_rows, r_rows, s_rows):
        """(handles, k) of a prove call after the checks that need no device"""
        h = self.handle()
        if not isinstance(r1cs, R1cs):
            raise ValueError("r1cs must come from r1cs()")
        if not isinstance(domain, FrNttDomain):
            raise ValueError("domain must come from fr_ntt_domain")
        hr, hd = r1cs.handle(), domain.handle()
        if domain.log_n != self.log_n:
            raise ValueError("the domain has log_n = %d, the key %d" % (domain.log_n, self.log_n))
        if r1cs.cols != self.n_vars:
            raise ValueError("the system has %d columns, the key %d variables" % (r1cs.cols, self.n_vars))
        if r1cs.rows > (1 << self.log_n):
            raise ValueError("the system's %d rows exceed the domain's %d points" % (r1cs.rows, 1 << self.log_n))
        k = r_rows
        if s_rows != k or witness_rows != k * self.n_vars:
            raise ValueError("%d witness rows, %d r rows and %d s rows are not k proofs of %d variables"
                             % (witness_rows, r_rows, s_rows, self.n_vars))
        return (h, hr, hd), k

    def prove_workspace_bytes(self, r1cs, k):
        """pa_groth16_prove_workspace_bytes; a batch over the limit is a ValueError: split it"""
        if not isinstance(r1cs, R1cs):
            raise ValueError("r1cs must come from r1cs()")
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative, got %d" % k)
        n = int(_lib.pa_groth16_prove_workspace_bytes(self.handle(), r1cs.handle(), k))
        if n == 0:
            raise ValueError("a batch of %d proofs is over a multiexp's item limit, or the system does not fit the "
                             "key: split it" % k)
        return n


class Groth16Key(ctypes.Structure):
    """pa_groth16_key of the header"""
    _fields_ = [("alpha_g1", ctypes.c_uint64 * W_G1A), ("beta_g1", ctypes.c_uint64 * W_G1A),
                ("delta_g1", ctypes.c_uint64 * W_G1A), ("beta_g2", ctypes.c_uint64 * W_G2A),
                ("delta_g2", ctypes.c_uint64 * W_G2A), ("n_vars", ctypes.c_size_t), ("n_public", ctypes.c_size_t),
                ("a_query", _P), ("b_g1_query", _P), ("b_g2_query", _P), ("l_query", _P), ("h_query", _P),
                ("h_len", ctypes.c_size_t)]


GROTH16_VK_MAX_INPUTS = 512        # PA_GROTH16_VK_MAX_INPUTS of the header
GROTH16_ENCODED_PROOF_BYTES = 192  # PA_GROTH16_ENCODED_PROOF_BYTES: A (48), B (96), C (48) compressed


class Groth16VKey(ctypes.Structure):
    """pa_groth16_vkey of the header"""
    _fields_ = [("alpha_g1", ctypes.c_uint64 * W_G1A), ("beta_g2", ctypes.c_uint64 * W_G2A),
                ("gamma_g2", ctypes.c_uint64 * W_G2A), ("delta_g2", ctypes.c_uint64 * W_G2A),
                ("ic", _P), ("n_public", ctypes.c_size_t)]


class Groth16Vk(_Handle):
    """A pa_groth16_vk handle: a verifying key prepared on one device -- e(alpha, beta),
    -gamma and -delta (affine and prepared), ic[0] and a fixed-base comb table for each of
    ic[1..l]; for the aggregate check the comb tables of ic[0] and alpha and -beta.  `n_public` counts the constant one, `n_inputs` = n_public - 1 is the l of a
    verify call, `bytes` the device memory held."""

    WHAT = "Groth16 verifying key"
    FREE = "pa_groth16_vk_free"

    def __init__(self, handle, n_public, nbytes=0, owns=True):
        super().__init__(handle, owns)
        self.n_public, self.bytes = int(n_public), int(nbytes)
        self.n_inputs = self.n_public - 1

    @classmethod
    def _adopt(cls, handle):
        """take ownership of a handle pa_groth16_vk_create just returned"""
        h = ctypes.c_void_p(handle.value)
        return cls(h, _lib.pa_groth16_vk_n_public(h), _lib.pa_groth16_vk_bytes(h))

    def check_inputs(self, rows, k, stride):
        """(handle, stride) of a call over k proofs after the checks that need no device: `rows` input rows
        at `stride` rows per proof (None: n_inputs) must hold the last proof's n_inputs rows"""
        h = self.handle()
        l = self.n_inputs
        stride = l if stride is None else int(stride)
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative, got %d" % k)
        if stride < l:
            raise ValueError("input stride %d is below the key's %d inputs" % (stride, l))
        need = (k - 1) * stride + l if k and l else 0
        if rows < need:
            raise ValueError("%d input rows do not hold %d proofs of %d inputs at stride %d (%d rows)"
                             % (rows, k, l, stride, need))
        return h, stride

    def _bytes(self, name, k):
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative, got %d" % k)
        n = int(getattr(_lib, name)(self.handle(), k))
        if n == 0 and k and (name != "pa_groth16_vk_input_sum_workspace_bytes" or self.n_inputs):
            raise ValueError("a batch of %d proofs is over PA_GROTH16_VERIFY_MAX_BATCH: split it" % k)
        return n

    def verify_aggregate_workspace_bytes(self, k):
        """pa_groth16_verify_aggregate_workspace_bytes, for the three aggregate entries (never 0)"""
        return self._bytes("pa_groth16_verify_aggregate_workspace_bytes", k)

    def verify_workspace_bytes(self, k):
        """pa_groth16_verify_workspace_bytes; a batch over the limit is a ValueError: split it"""
        return self._bytes("pa_groth16_verify_workspace_bytes", k)

    def input_sum_workspace_bytes(self, k):
        """pa_groth16_vk_input_sum_workspace_bytes (0 for a key without inputs)"""
        return self._bytes("pa_groth16_vk_input_sum_workspace_bytes", k)


class FrCsr(ctypes.Structure):
    """pa_fr_csr of the header"""
    _fields_ = [("row_ptr", _P), ("col", _P), ("val", _P)]


FR_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def trapdoor_rows(trapdoor):
    """pa_groth16_trapdoor as a (5, 4) uint64 array (tau, alpha, beta, gamma, delta; Montgomery rows), checked as
    the library checks it: every value below r, gamma and delta not zero"""
    t = as_rows(trapdoor, W_FR, "trapdoor")
    if t.shape[0] != 5:
        raise ValueError("trapdoor must be 5 rows (tau, alpha, beta, gamma, delta), got %d" % t.shape[0])
    for row, name in zip(t, ("tau", "alpha", "beta", "gamma", "delta")):
        v = sum(int(x) << (64 * i) for i, x in enumerate(row))
        if v >= FR_MODULUS:
            raise ValueError("trapdoor %s is not below r" % name)
        if v == 0 and name in ("gamma", "delta"):
            raise ValueError("trapdoor %s must not be zero" % name)
    return t


class Groth16Circuit(_Handle):
    """A pa_groth16_circuit handle: the transposed matrices of a constraint system on one
    device, what parameter generation sums over.  `rows` (constraints), `cols` (variables),
    `n_public` (counting the constant one) and `bytes` (device memory held) are read at
    creation."""

    WHAT = "Groth16 circuit"
    FREE = "pa_groth16_circuit_free"

    def __init__(self, handle, rows, cols, n_public, nbytes=0, owns=True):
        super().__init__(handle, owns)
        self.rows, self.cols, self.n_public, self.bytes = int(rows), int(cols), int(n_public), int(nbytes)

    @classmethod
    def _adopt(cls, handle):
        """take ownership of a handle pa_groth16_circuit_create just returned"""
        h = ctypes.c_void_p(handle.value)
        return cls(h, _lib.pa_groth16_circuit_rows(h), _lib.pa_groth16_circuit_cols(h),
                   _lib.pa_groth16_circuit_n_public(h), _lib.pa_groth16_circuit_bytes(h))

    def check_generate(self, domain):
        """(handles, log_n) of a generation call after the checks that need no device"""
        h = self.handle()
        if not isinstance(domain, FrNttDomain):
            raise ValueError("domain must come from fr_ntt_domain")
        hd = domain.handle()
        if domain.len < self.rows:
            raise ValueError("the circuit's %d rows exceed the domain's %d points" % (self.rows, domain.len))
        return (h, hd), domain.log_n

    def g1_len(self, log_n):
        """records of g1_out: 3 n_vars + 2^log_n + 2"""
        return 3 * self.cols + (1 << int(log_n)) + 2

    def g2_len(self):
        """records of g2_out: n_vars + 3"""
        return self.cols + 3

    def generate_workspace_bytes(self, log_n):
        """pa_groth16_generate_workspace_bytes; a domain smaller than the circuit's rows is a ValueError"""
        log_n = int(log_n)
        if log_n < 0 or log_n > NTT_MAX_LOG_N:
            raise ValueError("log_n must be 0..%d, got %d" % (NTT_MAX_LOG_N, log_n))
        if (1 << log_n) < self.rows:
            raise ValueError("2^%d points do not hold the circuit's %d rows" % (log_n, self.rows))
        return int(_lib.pa_groth16_generate_workspace_bytes(self.handle(), log_n))


class Groth16Params:
    """What groth16_generate returns: views into the two output arrays (pa_groth16_generate_offsets
    of the header).  a_query, b_g1_query (n_vars, 13), b_g2_query (n_vars, 25), ic (n_public, 13),
    l_query (n_vars - n_public, 13), h_query (2^log_n - 1, 13), alpha_g1, beta_g1, delta_g1 (1, 13),
    beta_g2, gamma_g2, delta_g2 (1, 25); `g1` and `g2` are the whole arrays."""

    def __init__(self, g1, g2, n_vars, n_public, log_n):
        self.g1, self.g2 = g1, g2
        self.n_vars, self.n_public, self.log_n = int(n_vars), int(n_public), int(log_n)
        nv, h0 = self.n_vars, 3 * self.n_vars
        c0 = h0 + (1 << self.log_n) - 1
        self.a_query, self.b_g1_query = g1[:nv], g1[nv:2 * nv]
        self.ic, self.l_query = g1[2 * nv:2 * nv + self.n_public], g1[2 * nv + self.n_public:h0]
        self.h_query = g1[h0:c0]
        self.alpha_g1, self.beta_g1, self.delta_g1 = g1[c0:c0 + 1], g1[c0 + 1:c0 + 2], g1[c0 + 2:c0 + 3]
        self.b_g2_query = g2[:nv]
        self.beta_g2, self.gamma_g2, self.delta_g2 = g2[nv:nv + 1], g2[nv + 1:nv + 2], g2[nv + 2:nv + 3]

    def pk_args(self):
        """the arguments of groth16_pk, n_public and log_n included"""
        return (self.alpha_g1, self.beta_g1, self.delta_g1, self.beta_g2, self.delta_g2, self.a_query,
                self.b_g1_query, self.b_g2_query, self.l_query, self.h_query, self.n_public, self.log_n)

    def vk_args(self):
        """the arguments of groth16_vk"""
        return (self.alpha_g1, self.beta_g2, self.gamma_g2, self.delta_g2, self.ic)
