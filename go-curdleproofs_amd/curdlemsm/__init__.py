"""ctypes binding of libcurdlemsm.so (include/curdle_msm.h).

Thin plumbing only: every function below forwards to one C-ABI entry point of
the HIP library; there is no Python or CPU implementation of the MSM here.  If
the shared library is missing, importing this package raises -- the product
path must fail loudly rather than fall back.

Layouts are gnark-crypto's (see the header): points are uint64[n, 12]
(G1Affine, Montgomery), scalars uint64[n, 4] (fr.Element, Montgomery), results
uint64[18] (G1Jac, canonical representative).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CURDLE_MSM_LIB", os.path.join(os.path.dirname(_HERE), "libcurdlemsm.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build it with `make -C go-curdleproofs_amd` "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`)")

# PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process do not
# both see the GPU.  When torch is present (it provides device memory, streams and
# torch.distributed to callers of this binding) load it first so that
# libcurdlemsm.so binds to the runtime already in the process.
try:  # pragma: no cover - depends on the environment
    import torch  # noqa: F401
except Exception:  # torch absent: the system ROCm runtime is used
    torch = None

_lib = C.CDLL(LIB_PATH)

OK, EINVAL, ENODEV, EHIP, ENOMEM, EBUSY = 0, -1, -2, -3, -4, -5
MSM_SLOTS = 8

# Every symbol include/curdle_msm.h declares (tests check they are all exported).
SYMBOLS = [
    "curdle_init", "curdle_shutdown", "curdle_last_error", "curdle_plan_override", "curdle_device_available",
    "curdle_init_devices", "curdle_device_count", "curdle_set_device", "curdle_get_device", "curdle_get_device_selection", "curdle_stat_spread_calls",
    "curdle_msm_g1_replicated",
    "curdle_msm_g1_ex", "curdle_msm_g1_device_ex", "curdle_msm_g1_device_windows_ex", "curdle_msm_g1_device_submit_ex",
    "curdle_msm_forget_bases",
    "curdle_msm_g1", "curdle_msm_g1_device", "curdle_msm_g1_device_windows",
    "curdle_msm_g1_device_submit", "curdle_msm_wait",
    "curdle_msm_window_bits", "curdle_msm_num_windows", "curdle_msm_window_widths", "curdle_msm_num_windows_ex",
    "curdle_msm_window_widths_ex", "curdle_g1_sum",
    "curdle_msm_g1_batch", "curdle_msm_g1_batch_device", "curdle_msm_g1_multi",
    "curdle_rand_new", "curdle_rand_free", "curdle_rand_get_fr", "curdle_rand_get_g1_affine",
    "curdle_rand_permutation",
    "curdle_acc_new", "curdle_acc_free", "curdle_acc_accumulate_check", "curdle_acc_accumulate_check_deferred",
    "curdle_acc_verify",
    "curdle_acc_get_A_c", "curdle_acc_num_bases", "curdle_acc_export",
    "curdle_profile_enable", "curdle_profile_last", "curdle_selftest_op", "curdle_selftest_shape", "curdle_msm_free_slots",
    "curdle_synth_points_walk_device",
    "curdle_crs_generate", "curdle_crs_free", "curdle_crs_size", "curdle_shuffle_permute_commit",
    "curdle_prove", "curdle_verify", "curdle_proof_from_bytes", "curdle_proof_free", "curdle_verify_proof",
    "curdle_verify_batch", "curdle_verify_set_eager",
    "curdle_whisk_is_valid_shuffle_proof", "curdle_whisk_is_valid_shuffle_proof_batch",
    "curdle_whisk_generate_shuffle_proof",
    "curdle_whisk_is_valid_tracker_proof", "curdle_whisk_is_valid_tracker_proof_batch", "curdle_whisk_generate_tracker_proof", "curdle_proof_reencode", "curdle_merlin_test_vector", "curdle_g1_decompress_batch", "curdle_g1_decompress_begin", "curdle_g1_decompress_finish", "curdle_g1_decompress_start", "curdle_g1_decompress_points",
    "curdle_g1_scalar_mul_batch",
    "curdle_g1_compress", "curdle_g1_decompress", "curdle_set_last_error", "curdle_fr_inner_product",
    "curdle_dbases_create", "curdle_dbases_free", "curdle_dbases_size", "curdle_dbases_valid",
    "curdle_msm_g1_dbases", "curdle_msm_g1_dbases_host", "curdle_msm_g1_dbases_windows", "curdle_msm_g1_dbases_submit",
    "curdle_dacc_begin", "curdle_dacc_run", "curdle_dacc_submit", "curdle_dacc_poll", "curdle_dacc_wait", "curdle_dacc_abort", "curdle_stat_dacc_builds",
    "curdle_dacc_run_members", "curdle_stat_dacc_members",
    "curdle_verify_set_device_acc", "curdle_verify_export_accumulator",
    "curdle_g1_check_batch", "curdle_g1_check_batch_device", "curdle_verify_checked", "curdle_verify_proof_checked",
    "curdle_stat_check_paths",
    "curdle_g1_check_jac_batch", "curdle_g1_check_jac_batch_device", "curdle_verify_batch_checked", "curdle_stat_batch_checked",
    "curdle_transcript_batch", "curdle_transcript_batch_host", "curdle_stat_transcript", "curdle_transcript_last_kernel_ms",
    "curdle_whisk_is_valid_tracker_proof_batch_ex", "curdle_whisk_is_valid_tracker_proof_batch_device", "curdle_stat_tracker",
    "curdle_g1_compress_batch", "curdle_g1_compress_batch_device",
    "curdle_whisk_generate_tracker_proof_batch_blinders", "curdle_whisk_generate_tracker_proof_batch", "curdle_stat_tracker_prove",
    "curdle_whisk_is_own_tracker", "curdle_whisk_find_own_trackers", "curdle_whisk_find_own_trackers_device", "curdle_stat_tracker_own",
    "curdle_whisk_find_own_trackers_ex", "curdle_whisk_find_own_trackers_device_ex", "curdle_stat_tracker_own_ct",
    "curdle_g1_normalize_batch", "curdle_g1_normalize_batch_device", "curdle_g1_scalar_mul_batch_device", "curdle_stat_normalize",
    "curdle_fbase_create", "curdle_fbase_free", "curdle_g1_fixed_base_mul_batch", "curdle_g1_fixed_base_mul_batch_device",
    "curdle_stat_fbase", "curdle_whisk_compute_tracker", "curdle_whisk_k_commitment", "curdle_whisk_compute_trackers_batch",
    "curdle_g1_fixed_base_mul_batch_ex", "curdle_g1_fixed_base_mul_batch_device_ex", "curdle_whisk_compute_trackers_batch_ex",
    "curdle_stat_fbase_ct",
    "curdle_g1_scalar_mul_batch_ex", "curdle_g1_scalar_mul_batch_device_ex", "curdle_stat_g1_mul_ct",
    "curdle_whisk_generate_tracker_proof_batch_blinders_ex", "curdle_whisk_generate_tracker_proof_batch_ex",
    "curdle_whisk_is_valid_tracker_proof_batch_combined", "curdle_whisk_is_valid_tracker_proof_batch_combined_device",
    "curdle_stat_tracker_combined", "curdle_whisk_tracker_combined_scalars", "curdle_tracker_combined_last_kernel_ms",
    "curdle_stat_transcript_paths", "curdle_keccak_permute_batch",
    "curdle_msm_reduce_plan", "curdle_msm_stream_plan",
    "curdle_msm_g1_ct", "curdle_msm_g1_ct_device", "curdle_stat_msm_ct", "curdle_shuffle_permute_commit_ex",
    "curdle_g1_permute_ct_device",
    "curdle_msm_g1_ct_batch", "curdle_msm_g1_ct_batch_device", "curdle_msm_g1_ct_multi", "curdle_stat_msm_ct_batch",
    "curdle_prove_ex", "curdle_stat_alg_msm",
    "curdle_fr_permute_ct", "curdle_fr_permute_ct_device", "curdle_stat_fr_permute_ct",
    "curdle_prove_ct", "curdle_whisk_generate_shuffle_proof_ct", "curdle_stat_host_point_mul",
    "curdle_fr_permute_ct_batch", "curdle_fr_permute_ct_batch_device", "curdle_g1_permute_ct_batch_device",
    "curdle_prove_batch", "curdle_whisk_generate_shuffle_proof_batch", "curdle_stat_prove_batch",
    "curdle_ct_bases_create", "curdle_ct_bases_create_device", "curdle_ct_bases_free", "curdle_ct_bases_size",
    "curdle_ct_bases_chunk_bits", "curdle_ct_bases_export",
    "curdle_msm_g1_ct_bases", "curdle_msm_g1_ct_bases_device", "curdle_msm_g1_ct_bases_batch",
    "curdle_msm_g1_ct_bases_batch_device", "curdle_stat_msm_ct_bases",
    "curdle_msm_g1_ct_bases_sets_batch", "curdle_msm_g1_ct_bases_sets_batch_device",
    "curdle_prover_ct_create", "curdle_prover_ct_free", "curdle_prover_ct_prove", "curdle_prover_ct_whisk_shuffle_proof",
    "curdle_stat_alg_msm_resident",
    "curdle_crs_from_points", "curdle_crs_from_bytes", "curdle_crs_export_points", "curdle_crs_to_bytes",
    "curdle_fp_invert_batch", "curdle_fp_invert_batch_device", "curdle_stat_fp_invert",
]

_u64p = C.POINTER(C.c_uint64)
_vp = C.c_void_p


class _Profile(C.Structure):
    _fields_ = [("n_kernels", C.c_int), ("name", C.c_char_p * 16), ("ms", C.c_float * 16),
                ("window_bits", C.c_int), ("num_windows", C.c_int), ("entries", C.c_ulonglong),
                ("fragments", C.c_ulonglong), ("large_buckets", C.c_ulonglong)]


def _sig(name, restype, *argtypes):
    f = getattr(_lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_init = _sig("curdle_init", C.c_int, C.c_int)
_shutdown = _sig("curdle_shutdown", C.c_int)
_init_devices = _sig("curdle_init_devices", C.c_int, C.POINTER(C.c_int), C.c_int)
_device_count = _sig("curdle_device_count", C.c_int)
_set_device = _sig("curdle_set_device", C.c_int, C.c_int)
_get_device = _sig("curdle_get_device", C.c_int)
_get_device_selection = _sig("curdle_get_device_selection", C.c_int)
_stat_spread_calls = _sig("curdle_stat_spread_calls", C.c_ulonglong)
_msm_g1_ex = _sig("curdle_msm_g1_ex", C.c_int, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_msm_g1_device_windows_ex = _sig("curdle_msm_g1_device_windows_ex", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                 C.c_uint, _vp, _vp)
_msm_submit_ex = _sig("curdle_msm_g1_device_submit_ex", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint,
                      C.POINTER(C.c_int))
_msm_forget_bases = _sig("curdle_msm_forget_bases", C.c_int, _vp)
_msm_g1_replicated = _sig("curdle_msm_g1_replicated", C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t,
                          C.c_int, _vp)
_last_error = _sig("curdle_last_error", C.c_int, C.c_char_p, C.c_size_t)
_plan_override = _sig("curdle_plan_override", C.c_int, C.c_char_p, C.c_longlong)
_device_available = _sig("curdle_device_available", C.c_int)
_msm_g1 = _sig("curdle_msm_g1", C.c_int, _vp, _vp, C.c_size_t, _vp)
_msm_g1_device = _sig("curdle_msm_g1_device", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp)
_msm_g1_device_windows = _sig("curdle_msm_g1_device_windows", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int,
                              C.c_int, _vp, _vp)
_msm_submit = _sig("curdle_msm_g1_device_submit", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int,
                   C.POINTER(C.c_int))
_msm_wait = _sig("curdle_msm_wait", C.c_int, C.c_int, _vp)
_window_bits = _sig("curdle_msm_window_bits", C.c_int, C.c_size_t)
_num_windows = _sig("curdle_msm_num_windows", C.c_int, C.c_size_t, C.c_int)
_window_widths = _sig("curdle_msm_window_widths", C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_int))
_num_windows_ex = _sig("curdle_msm_num_windows_ex", C.c_int, C.c_size_t, C.c_int, C.c_uint)
_window_widths_ex = _sig("curdle_msm_window_widths_ex", C.c_int, C.c_size_t, C.c_int, C.c_uint, C.POINTER(C.c_int))
_msm_batch_device = _sig("curdle_msm_g1_batch_device", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp)
_g1_sum = _sig("curdle_g1_sum", C.c_int, _vp, C.c_size_t, _vp)
_msm_batch = _sig("curdle_msm_g1_batch", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp)
_msm_multi = _sig("curdle_msm_g1_multi", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp)
_rand_new = _sig("curdle_rand_new", _vp, C.c_uint64)
_rand_free = _sig("curdle_rand_free", None, _vp)
_rand_get_fr = _sig("curdle_rand_get_fr", C.c_int, _vp, _vp)
_rand_get_g1 = _sig("curdle_rand_get_g1_affine", C.c_int, _vp, _vp)
_rand_perm = _sig("curdle_rand_permutation", C.c_int, _vp, C.c_size_t, _vp)
_acc_new = _sig("curdle_acc_new", _vp)
_acc_free = _sig("curdle_acc_free", None, _vp)
_acc_check = _sig("curdle_acc_accumulate_check", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp)
_acc_check_deferred = _sig("curdle_acc_accumulate_check_deferred", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t,
                           _vp, C.c_size_t, _vp)
_acc_verify = _sig("curdle_acc_verify", C.c_int, _vp, C.POINTER(C.c_int))
_acc_get_A_c = _sig("curdle_acc_get_A_c", C.c_int, _vp, _vp)
_acc_num_bases = _sig("curdle_acc_num_bases", C.c_size_t, _vp)
_acc_export = _sig("curdle_acc_export", C.c_int, _vp, _vp, _vp)
_profile_enable = _sig("curdle_profile_enable", C.c_int, C.c_int)
_profile_last = _sig("curdle_profile_last", C.c_int, C.POINTER(_Profile))
_synth_walk = _sig("curdle_synth_points_walk_device", C.c_int, _vp, _vp, C.c_size_t, _vp)
_dbases_create = _sig("curdle_dbases_create", C.c_int, _vp, C.c_size_t, C.POINTER(C.c_void_p))
_dbases_free = _sig("curdle_dbases_free", None, _vp)
_msm_dbases_windows = _sig("curdle_msm_g1_dbases_windows", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp)
_msm_dbases_host = _sig("curdle_msm_g1_dbases_host", C.c_int, _vp, _vp, C.c_size_t, _vp)
_msm_dbases_submit = _sig("curdle_msm_g1_dbases_submit", C.c_int, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int))
_dacc_begin = _sig("curdle_dacc_begin", C.c_int, _vp, _vp, C.c_size_t, C.POINTER(C.c_void_p))
_dacc_run = _sig("curdle_dacc_run", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp)
_dacc_submit = _sig("curdle_dacc_submit", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp)
_dacc_poll = _sig("curdle_dacc_poll", C.c_int, _vp, C.POINTER(C.c_int))
_dacc_wait = _sig("curdle_dacc_wait", C.c_int, _vp, _vp)
_dacc_abort = _sig("curdle_dacc_abort", None, _vp)
_stat_dacc_builds = _sig("curdle_stat_dacc_builds", C.c_int, C.POINTER(C.c_ulonglong))
_dacc_run_members = _sig("curdle_dacc_run_members", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp,
                         C.c_size_t, _vp, _vp)
_msm_free_slots = _sig("curdle_msm_free_slots", C.c_int)
_stat_dacc_members = _sig("curdle_stat_dacc_members", C.c_int, C.POINTER(C.c_ulonglong))
_selftest_op = _sig("curdle_selftest_op", C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_int)
_selftest_shape = _sig("curdle_selftest_shape", C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))


_crs_generate = _sig("curdle_crs_generate", _vp, C.c_size_t, _vp)
_crs_free = _sig("curdle_crs_free", None, _vp)
_crs_size = _sig("curdle_crs_size", C.c_size_t, _vp)
_spc = _sig("curdle_shuffle_permute_commit", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_prove = _sig("curdle_prove", C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t,
              C.POINTER(C.c_size_t))
_verify = _sig("curdle_verify", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
               C.POINTER(C.c_int))
_proof_from_bytes = _sig("curdle_proof_from_bytes", C.c_int, _vp, C.c_size_t, C.POINTER(_vp))
_proof_free = _sig("curdle_proof_free", None, _vp)
_verify_proof = _sig("curdle_verify_proof", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_int))
_verify_batch = _sig("curdle_verify_batch", C.c_int, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                     C.c_int, _vp)
_whisk_valid_shuffle = _sig("curdle_whisk_is_valid_shuffle_proof", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp,
                            C.POINTER(C.c_int))
_whisk_valid_shuffle_batch = _sig("curdle_whisk_is_valid_shuffle_proof_batch", C.c_int, _vp, C.c_size_t, _vp, _vp, C.c_size_t,
                                  _vp, _vp, C.c_int, _vp)
_whisk_gen_shuffle = _sig("curdle_whisk_generate_shuffle_proof", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp)
_whisk_valid_tracker = _sig("curdle_whisk_is_valid_tracker_proof", C.c_int, _vp, _vp, _vp, C.POINTER(C.c_int))
_whisk_valid_tracker_batch = _sig("curdle_whisk_is_valid_tracker_proof_batch", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp)
_whisk_valid_tracker_batch_ex = _sig("curdle_whisk_is_valid_tracker_proof_batch_ex", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_whisk_valid_tracker_batch_device = _sig("curdle_whisk_is_valid_tracker_proof_batch_device", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp)
_stat_tracker = _sig("curdle_stat_tracker", C.c_int, C.POINTER(C.c_ulonglong))
_whisk_valid_tracker_batch_combined = _sig("curdle_whisk_is_valid_tracker_proof_batch_combined", C.c_int, _vp, _vp, _vp, C.c_size_t,
                                           _vp, _vp)
_whisk_valid_tracker_batch_combined_device = _sig("curdle_whisk_is_valid_tracker_proof_batch_combined_device", C.c_int, _vp, _vp,
                                                  _vp, C.c_size_t, _vp, _vp, _vp)
_stat_tracker_combined = _sig("curdle_stat_tracker_combined", C.c_int, C.POINTER(C.c_ulonglong))
_tracker_combined_last_kernel_ms = _sig("curdle_tracker_combined_last_kernel_ms", C.c_int, C.POINTER(C.c_double))
_whisk_tracker_combined_scalars = _sig("curdle_whisk_tracker_combined_scalars", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp)
_whisk_gen_tracker = _sig("curdle_whisk_generate_tracker_proof", C.c_int, _vp, _vp, _vp, _vp)
_whisk_gen_tracker_batch_blinders = _sig("curdle_whisk_generate_tracker_proof_batch_blinders", C.c_int, _vp, _vp, _vp, C.c_size_t,
                                         _vp, _vp)
_whisk_gen_tracker_batch = _sig("curdle_whisk_generate_tracker_proof_batch", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp)
_stat_tracker_prove = _sig("curdle_stat_tracker_prove", C.c_int, C.POINTER(C.c_ulonglong))
_whisk_gen_tracker_batch_blinders_ex = _sig("curdle_whisk_generate_tracker_proof_batch_blinders_ex", C.c_int, _vp, _vp, _vp,
                                            C.c_size_t, C.c_uint, _vp, _vp)
_whisk_gen_tracker_batch_ex = _sig("curdle_whisk_generate_tracker_proof_batch_ex", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint,
                                   _vp, _vp)
_whisk_is_own_tracker = _sig("curdle_whisk_is_own_tracker", C.c_int, _vp, _vp, C.POINTER(C.c_int))
_whisk_find_own = _sig("curdle_whisk_find_own_trackers", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp)
_whisk_find_own_device = _sig("curdle_whisk_find_own_trackers_device", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp)
_stat_tracker_own = _sig("curdle_stat_tracker_own", C.c_int, C.POINTER(C.c_ulonglong))
_whisk_find_own_ex = _sig("curdle_whisk_find_own_trackers_ex", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_uint)
_whisk_find_own_device_ex = _sig("curdle_whisk_find_own_trackers_device_ex", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp,
                                 C.c_uint)
_stat_tracker_own_ct = _sig("curdle_stat_tracker_own_ct", C.c_int, C.POINTER(C.c_ulonglong))
_fbase_create = _sig("curdle_fbase_create", C.c_int, _vp, C.POINTER(_vp))
_fbase_free = _sig("curdle_fbase_free", None, _vp)
_fbase_mul = _sig("curdle_g1_fixed_base_mul_batch", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int, _vp)
_fbase_mul_device = _sig("curdle_g1_fixed_base_mul_batch_device", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int, _vp, _vp)
_stat_fbase = _sig("curdle_stat_fbase", C.c_int, C.POINTER(C.c_ulonglong))
_whisk_compute_tracker = _sig("curdle_whisk_compute_tracker", C.c_int, _vp, _vp, _vp)
_whisk_k_commitment = _sig("curdle_whisk_k_commitment", C.c_int, _vp, _vp)
_whisk_compute_trackers_batch = _sig("curdle_whisk_compute_trackers_batch", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp)
_fbase_mul_ex = _sig("curdle_g1_fixed_base_mul_batch_ex", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_uint, _vp)
_fbase_mul_device_ex = _sig("curdle_g1_fixed_base_mul_batch_device_ex", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_uint,
                            _vp, _vp)
_whisk_compute_trackers_batch_ex = _sig("curdle_whisk_compute_trackers_batch_ex", C.c_int, _vp, _vp, C.c_size_t, C.c_uint, _vp, _vp)
_stat_fbase_ct = _sig("curdle_stat_fbase_ct", C.c_int, C.POINTER(C.c_ulonglong))
_verify_set_eager = _sig("curdle_verify_set_eager", C.c_int, C.c_int)
_reencode = _sig("curdle_proof_reencode", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t))
_merlin_tv = _sig("curdle_merlin_test_vector", C.c_int, C.c_char_p, C.c_char_p, _vp, C.c_size_t, C.c_char_p, _vp,
                  C.c_size_t)
_g1_compress = _sig("curdle_g1_compress", C.c_int, _vp, _vp)
_g1_decompress = _sig("curdle_g1_decompress", C.c_int, _vp, C.c_int, _vp)
_g1_compress_batch = _sig("curdle_g1_compress_batch", C.c_int, _vp, C.c_size_t, _vp)
_g1_compress_batch_device = _sig("curdle_g1_compress_batch_device", C.c_int, _vp, C.c_size_t, _vp, _vp)
_g1_normalize_batch = _sig("curdle_g1_normalize_batch", C.c_int, _vp, C.c_int, C.c_size_t, _vp)
_g1_normalize_batch_device = _sig("curdle_g1_normalize_batch_device", C.c_int, _vp, C.c_int, C.c_size_t, _vp, _vp)
_scalar_mul_batch_device = _sig("curdle_g1_scalar_mul_batch_device", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp)
_stat_normalize = _sig("curdle_stat_normalize", C.c_int, C.POINTER(C.c_ulonglong))
_scalar_mul_batch_ex = _sig("curdle_g1_scalar_mul_batch_ex", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_uint, _vp)
_scalar_mul_batch_device_ex = _sig("curdle_g1_scalar_mul_batch_device_ex", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t,
                                   C.c_uint, _vp, _vp)
_stat_g1_mul_ct = _sig("curdle_stat_g1_mul_ct", C.c_int, C.POINTER(C.c_ulonglong))
_msm_g1_ct = _sig("curdle_msm_g1_ct", C.c_int, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_msm_g1_ct_device = _sig("curdle_msm_g1_ct_device", C.c_int, _vp, _vp, C.c_size_t, C.c_uint, _vp, _vp)
_stat_msm_ct = _sig("curdle_stat_msm_ct", C.c_int, C.POINTER(C.c_ulonglong))
_g1_permute_ct_device = _sig("curdle_g1_permute_ct_device", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp)
_spc_ex = _sig("curdle_shuffle_permute_commit_ex", C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, C.c_uint, _vp, _vp, _vp, _vp)
G1_FORM_JAC, G1_FORM_XYZZ = 0, 1


class CurdleError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"curdle error {code}: {msg}")
        self.code = code
        self.msg = msg


def last_error() -> str:
    buf = C.create_string_buffer(256)
    _last_error(buf, 256)
    return buf.value.decode()


def _check(rc: int) -> None:
    if rc != OK:
        raise CurdleError(rc, last_error())


def _as_u64(a, cols=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if cols is not None and a.size and a.shape[-1] != cols:
        raise ValueError(f"expected last dimension {cols}, got {a.shape}")
    return a


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_vp)


def plan_override(name: str, value=None) -> None:
    """Test / measurement hook: set one of the library's knobs (host/knobs.h; the name with or without
    CURDLE_), or put it back to "not set" with value None.  The environment is read only once."""
    _check(_plan_override(name.encode(), -1 if value is None else int(value)))


class knobs:
    """with knobs(WINDOW_BITS=12, SEG_LEN=16): ... -- the knobs are unset again on the way out."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            plan_override(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            plan_override(k, None)
        return False


def init(device: int = 0) -> None:
    _check(_init(device))


def shutdown() -> None:
    _check(_shutdown())


def init_devices(devices) -> None:
    """One process, several GPUs: one context per entry of `devices` (HIP device ids; an id may
    repeat).  See curdle_init_devices in include/curdle_msm.h."""
    arr = (C.c_int * len(devices))(*[int(d) for d in devices])
    _check(_init_devices(arr, len(devices)))


def device_count() -> int:
    return int(_device_count())


def set_device(ordinal: int) -> None:
    """The calling thread's current context (0 <= ordinal < device_count())."""
    _check(_set_device(int(ordinal)))


def get_device() -> int:
    return int(_get_device())


def get_device_selection() -> int:
    """The ordinal this thread selected with set_device, or -1 if it has made no selection."""
    return int(_get_device_selection())


def stat_spread_calls() -> int:
    return int(_stat_spread_calls())


# flags of the *_ex entry points (include/curdle_msm.h)
MSM_ANY_CURVE_POINT, MSM_BASES_UNCHANGED = 1, 2


SPLIT_AUTO, SPLIT_WINDOWS, SPLIT_POINTS = 0, 1, 2


def msm_g1_replicated(d_points, d_scalars, n: int, split: int = SPLIT_AUTO) -> np.ndarray:
    """One MSM over inputs resident on EVERY configured context (d_points[i] / d_scalars[i]: raw
    device pointers on context i's GPU), split by Pippenger windows or point ranges, one host
    thread per device, partials summed on the host."""
    k = device_count()
    assert len(d_points) == k and len(d_scalars) == k, "one pointer per configured device"
    pp = (C.c_void_p * k)(*[int(p) for p in d_points])
    ps = (C.c_void_p * k)(*[int(p) for p in d_scalars])
    out = np.zeros(18, dtype=np.uint64)
    _check(_msm_g1_replicated(pp, ps, n, int(split), _ptr(out)))
    return out


def device_available() -> bool:
    return bool(_device_available())


def msm_g1(points, scalars, flags: int = 0) -> np.ndarray:
    """(*G1Jac).MultiExp on host arrays: points uint64[n,12], scalars uint64[n,4] -> uint64[18].
    flags: MSM_ANY_CURVE_POINT = no endomorphism, gnark's result for bases outside the subgroup too."""
    points = _as_u64(points, 12)
    scalars = _as_u64(scalars, 4)
    n = points.shape[0] if points.size else 0
    ns = scalars.shape[0] if scalars.size else 0
    if n != ns:
        # gnark MultiExp: "len(points) != len(scalars)"
        raise CurdleError(EINVAL, "len(points) != len(scalars)")
    out = np.zeros(18, dtype=np.uint64)
    if flags:
        _check(_msm_g1_ex(_ptr(points), _ptr(scalars), n, int(flags), _ptr(out)))
    else:
        _check(_msm_g1(_ptr(points), _ptr(scalars), n, _ptr(out)))
    return out


def msm_g1_device(d_points: int, d_scalars: int, n: int, stream: int = 0, window_bits: int = 0,
                  win_begin: int = 0, win_end: int = -1, flags: int = 0) -> np.ndarray:
    """MSM on device-resident inputs (raw device pointers, e.g. torch_tensor.data_ptr()).
    flags: MSM_ANY_CURVE_POINT, MSM_BASES_UNCHANGED (the library keeps its converted copy of d_points)."""
    out = np.zeros(18, dtype=np.uint64)
    if flags:
        _check(_msm_g1_device_windows_ex(d_points, d_scalars, n, window_bits, win_begin, win_end, int(flags), _ptr(out),
                                         stream or None))
    else:
        _check(_msm_g1_device_windows(d_points, d_scalars, n, window_bits, win_begin, win_end, _ptr(out),
                                      stream or None))
    return out


def msm_g1_ct(points, scalars, scalar_bits: int = 255) -> np.ndarray:
    """msm_g1 for SECRET scalars (curdle_msm_g1_ct): the same 18 words by kernels whose instruction and address streams
    do not depend on the scalars.  scalar_bits (1...255) is the caller's public bound: a scalar at or above
    2^scalar_bits fails the call with EINVAL.  At most 65,536 pairs; bases in the prime-order subgroup."""
    points = _as_u64(points, 12)
    scalars = _as_u64(scalars, 4)
    n = points.shape[0] if points.size else 0
    ns = scalars.shape[0] if scalars.size else 0
    if n != ns:
        raise CurdleError(EINVAL, "len(points) != len(scalars)")
    out = np.zeros(18, dtype=np.uint64)
    _check(_msm_g1_ct(_ptr(points), _ptr(scalars), n, int(scalar_bits), _ptr(out)))
    return out


def msm_g1_ct_device(d_points: int, d_scalars: int, n: int, scalar_bits: int = 255, stream: int = 0) -> np.ndarray:
    """msm_g1_ct on device-resident inputs (curdle_msm_g1_ct_device; raw device pointers, multiples of 16)."""
    out = np.zeros(18, dtype=np.uint64)
    _check(_msm_g1_ct_device(d_points or None, d_scalars or None, n, int(scalar_bits), _ptr(out), stream or None))
    return out


def g1_permute_ct_device(d_in: int, d_perm: int, n: int, d_out: int, stream: int = 0) -> None:
    """d_out[i] = d_in[d_perm[i]] over 96-byte records by the oblivious gather of the flagged shuffle step
    (curdle_g1_permute_ct_device): no address is made of the permutation."""
    _check(_g1_permute_ct_device(d_in or None, d_perm or None, n, d_out or None, stream or None))


def stat_msm_ct() -> dict:
    """Pairs walked by the constant-time MSM, its walk launches and its finished sums since the library was loaded."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_msm_ct(out))
    return {"pairs": int(out[0]), "walks": int(out[1]), "sums": int(out[2])}


_msm_g1_ct_batch = _sig("curdle_msm_g1_ct_batch", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_msm_g1_ct_batch_device = _sig("curdle_msm_g1_ct_batch_device", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp, _vp)
_msm_g1_ct_multi = _sig("curdle_msm_g1_ct_multi", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_uint, _vp)
_stat_msm_ct_batch = _sig("curdle_stat_msm_ct_batch", C.c_int, C.POINTER(C.c_ulonglong))
_stat_alg_msm = _sig("curdle_stat_alg_msm", C.c_int, C.POINTER(C.c_ulonglong))


def msm_g1_ct_batch(points, scalars, offsets, scalar_bits: int = 255) -> np.ndarray:
    """msm_g1_batch for SECRET scalars (curdle_msm_g1_ct_batch): k MSMs in one constant-time walk -> uint64[k, 18], row j
    bit for bit msm_g1_ct on MSM j.  At most 65,536 pairs in all and 4,096 MSMs; one scalar_bits for the call."""
    points = _as_u64(points, 12)
    scalars = _as_u64(scalars, 4)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)  # size_t
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_g1_ct_batch(_ptr(points), _ptr(scalars), _ptr(offs), k, int(scalar_bits), _ptr(out)))
    return out


def msm_g1_ct_batch_device(d_points: int, d_scalars: int, offsets, scalar_bits: int = 255, stream: int = 0) -> np.ndarray:
    """msm_g1_ct_batch on device-resident, concatenated inputs (curdle_msm_g1_ct_batch_device; raw device pointers,
    multiples of 16; offsets stays a host array)."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_g1_ct_batch_device(d_points or None, d_scalars or None, _ptr(offs), k, int(scalar_bits), _ptr(out),
                                   stream or None))
    return out


def msm_g1_ct_multi(points_sets, scalars, scalar_bits: int = 255) -> np.ndarray:
    """msm_g1_multi for SECRET scalars (curdle_msm_g1_ct_multi): one scalar vector against k base sets of n points each
    -> uint64[k, 18]; k n <= 65,536."""
    sets = [_as_u64(p, 12) for p in points_sets]
    scalars = _as_u64(scalars, 4)
    n = scalars.shape[0] if scalars.size else 0
    for s in sets:
        if (s.shape[0] if s.size else 0) != n:
            raise CurdleError(EINVAL, "len(points) != len(scalars)")
    arr = (_vp * len(sets))(*[s.ctypes.data for s in sets])
    out = np.zeros((len(sets), 18), dtype=np.uint64)
    _check(_msm_g1_ct_multi(C.cast(arr, _vp), len(sets), _ptr(scalars), n, int(scalar_bits), _ptr(out)))
    return out


def stat_msm_ct_batch() -> dict:
    """Batched constant-time MSM calls, the MSMs in them and the level launches of k_g1_sum_ct_seg since the library
    was loaded."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_msm_ct_batch(out))
    return {"calls": int(out[0]), "msms": int(out[1]), "levels": int(out[2])}


def stat_alg_msm() -> dict:
    """The protocol code's MSM funnel (alg::MultiExp / MultiExpBatch / MultiExpShared): calls and pairs that went to the
    bucket MSM, and calls and pairs that went to the constant-time MSM."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_alg_msm(out))
    return {"bucket_calls": int(out[0]), "bucket_pairs": int(out[1]), "ct_calls": int(out[2]), "ct_pairs": int(out[3])}


_ct_bases_create = _sig("curdle_ct_bases_create", C.c_int, _vp, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p))
_ct_bases_create_device = _sig("curdle_ct_bases_create_device", C.c_int, _vp, C.c_size_t, C.c_uint, C.POINTER(C.c_void_p), _vp)
_ct_bases_free = _sig("curdle_ct_bases_free", None, _vp)
_ct_bases_size = _sig("curdle_ct_bases_size", C.c_size_t, _vp)
_ct_bases_chunk_bits = _sig("curdle_ct_bases_chunk_bits", C.c_uint, _vp)
_ct_bases_export = _sig("curdle_ct_bases_export", C.c_int, _vp, C.c_uint, _vp)
_msm_g1_ct_bases = _sig("curdle_msm_g1_ct_bases", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_msm_g1_ct_bases_device = _sig("curdle_msm_g1_ct_bases_device", C.c_int, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp, _vp)
_msm_g1_ct_bases_batch = _sig("curdle_msm_g1_ct_bases_batch", C.c_int, _vp, _vp, _vp, _vp, C.c_size_t, C.c_uint, _vp)
_msm_g1_ct_bases_batch_device = _sig("curdle_msm_g1_ct_bases_batch_device", C.c_int, _vp, _vp, _vp, _vp, C.c_size_t, C.c_uint,
                                     _vp, _vp)
_stat_msm_ct_bases = _sig("curdle_stat_msm_ct_bases", C.c_int, C.POINTER(C.c_ulonglong))


class CtBases:
    """A resident PUBLIC base set for the constant-time MSM (curdle_ct_bases): the table of the points 2^(c j) P_i, so
    that a lane walks c bits of a secret scalar instead of scalar_bits.  `points` is uint64[n, 12], or with device=True
    a raw device pointer and n; chunk_bits is 8, 16, 32, 64 or 0 for the library's choice.  rows (a host array of
    public indices into the set, or None for 0, 1, ..., n - 1) and offsets always stay host arrays."""

    def __init__(self, points, chunk_bits: int = 0, n: int = None, device: bool = False, stream: int = 0):
        self._h = C.c_void_p()
        if device:
            _check(_ct_bases_create_device(points or None, int(n), int(chunk_bits), C.byref(self._h), stream or None))
        else:
            pts = _as_u64(points, 12)
            _check(_ct_bases_create(_ptr(pts), pts.shape[0] if pts.size else 0, int(chunk_bits), C.byref(self._h)))
        self.n = int(_ct_bases_size(self._h))
        self.chunk_bits = int(_ct_bases_chunk_bits(self._h))
        self.chunks = (255 + self.chunk_bits - 1) // self.chunk_bits

    def free(self):
        if self._h:
            _ct_bases_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def export(self, chunk: int) -> np.ndarray:
        """Row `chunk` of the table: 2^(chunk_bits chunk) P_i as uint64[n, 12]."""
        out = np.zeros((self.n, 12), dtype=np.uint64)
        _check(_ct_bases_export(self._h, int(chunk), _ptr(out)))
        return out

    @staticmethod
    def _rows(rows):
        return None if rows is None else np.ascontiguousarray(rows, dtype=np.uint32)

    def msm(self, scalars, rows=None, scalar_bits: int = 255) -> np.ndarray:
        """sum_p scalars[p] * P_rows[p] -> uint64[18], bit for bit msm_g1_ct on the same pairs."""
        sc, r = _as_u64(scalars, 4), self._rows(rows)
        n = sc.shape[0] if sc.size else 0
        if r is not None and len(r) != n:
            raise CurdleError(EINVAL, "len(rows) != len(scalars)")
        out = np.zeros(18, dtype=np.uint64)
        _check(_msm_g1_ct_bases(self._h, None if r is None else _ptr(r), _ptr(sc), n, int(scalar_bits), _ptr(out)))
        return out

    def msm_device(self, d_scalars: int, n: int, rows=None, scalar_bits: int = 255, stream: int = 0) -> np.ndarray:
        """msm on device-resident scalars (a raw device pointer, a multiple of 16)."""
        r = self._rows(rows)
        if r is not None and len(r) != n:
            raise CurdleError(EINVAL, "len(rows) != n")
        out = np.zeros(18, dtype=np.uint64)
        _check(_msm_g1_ct_bases_device(self._h, None if r is None else _ptr(r), d_scalars or None, n, int(scalar_bits), _ptr(out),
                                       stream or None))
        return out

    def msm_batch(self, scalars, offsets, rows=None, scalar_bits: int = 255) -> np.ndarray:
        """k MSMs in one walk: MSM j covers the pairs [offsets[j], offsets[j + 1]) -> uint64[k, 18]."""
        sc, r = _as_u64(scalars, 4), self._rows(rows)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)  # size_t
        k = len(offs) - 1
        out = np.zeros((k, 18), dtype=np.uint64)
        _check(_msm_g1_ct_bases_batch(self._h, None if r is None else _ptr(r), _ptr(sc), _ptr(offs), k, int(scalar_bits),
                                      _ptr(out)))
        return out

    def msm_batch_device(self, d_scalars: int, offsets, rows=None, scalar_bits: int = 255, stream: int = 0) -> np.ndarray:
        r = self._rows(rows)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        k = len(offs) - 1
        out = np.zeros((k, 18), dtype=np.uint64)
        _check(_msm_g1_ct_bases_batch_device(self._h, None if r is None else _ptr(r), d_scalars or None, _ptr(offs), k,
                                             int(scalar_bits), _ptr(out), stream or None))
        return out


CT_BASES_MAX_SETS = 4                                  # CURDLE_CT_BASES_MAX_SETS
_msm_g1_ct_bases_sets_batch = _sig("curdle_msm_g1_ct_bases_sets_batch", C.c_int, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t,
                                   C.c_uint, _vp)
_msm_g1_ct_bases_sets_batch_device = _sig("curdle_msm_g1_ct_bases_sets_batch_device", C.c_int, _vp, C.c_size_t, _vp, _vp, _vp,
                                          C.c_size_t, C.c_uint, _vp, _vp)


def _set_handles(sets):
    return (C.c_void_p * max(1, len(sets)))(*[s._h for s in sets])


def msm_g1_ct_bases_sets_batch(sets, rows, scalars, offsets, scalar_bits: int = 255) -> np.ndarray:
    """CtBases.msm_batch over up to four CtBases of one chunk_bits in one call (curdle_msm_g1_ct_bases_sets_batch): rows
    index the concatenation of the sets -> uint64[k, 18], bit for bit the batch over one handle of the concatenated
    points."""
    sc, r = _as_u64(scalars, 4), CtBases._rows(rows)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_g1_ct_bases_sets_batch(_set_handles(sets), len(sets), None if r is None else _ptr(r), _ptr(sc), _ptr(offs), k,
                                       int(scalar_bits), _ptr(out)))
    return out


def msm_g1_ct_bases_sets_batch_device(sets, rows, d_scalars: int, offsets, scalar_bits: int = 255, stream: int = 0) -> np.ndarray:
    """msm_g1_ct_bases_sets_batch on device-resident scalars (a raw device pointer, a multiple of 16)."""
    r = CtBases._rows(rows)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_g1_ct_bases_sets_batch_device(_set_handles(sets), len(sets), None if r is None else _ptr(r), d_scalars or None,
                                              _ptr(offs), k, int(scalar_bits), _ptr(out), stream or None))
    return out


def stat_msm_ct_bases() -> dict:
    """Constant-time base tables built on a device, MSM calls over them, (pair, chunk) lanes walked and MSMs finished
    since the library was loaded."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_msm_ct_bases(out))
    return {"tables": int(out[0]), "calls": int(out[1]), "lanes": int(out[2]), "msms": int(out[3])}


def msm_g1_device_submit(d_points: int, d_scalars: int, n: int, window_bits: int = 0, win_begin: int = 0,
                         win_end: int = -1, flags: int = 0) -> int:
    """Enqueue one MSM (or window range) and return a ticket; see msm_wait()."""
    t = C.c_int(-1)
    if flags:
        _check(_msm_submit_ex(d_points, d_scalars, n, window_bits, win_begin, win_end, int(flags), C.byref(t)))
    else:
        _check(_msm_submit(d_points, d_scalars, n, window_bits, win_begin, win_end, C.byref(t)))
    return t.value


def msm_forget_bases(d_points: int) -> None:
    """Drops the converted copy a MSM_BASES_UNCHANGED call left for d_points."""
    _check(_msm_forget_bases(d_points))


class DBases:
    """A resident, pre-converted base set (curdle_dbases): the plain MSM over it uploads and converts
    nothing per call."""

    def __init__(self, points):
        pts = _as_u64(points, 12)
        self.n = len(pts)
        self._h = C.c_void_p()
        _check(_dbases_create(_ptr(pts), self.n, C.byref(self._h)))

    def free(self):
        if self._h:
            _dbases_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def msm(self, d_scalars: int, n: int = None, window_bits: int = 0, win_begin: int = 0, win_end: int = -1) -> np.ndarray:
        """scalars in device memory; a window range gives the scaled partial."""
        out = np.zeros(18, dtype=np.uint64)
        _check(_msm_dbases_windows(self._h, d_scalars, self.n if n is None else n, window_bits, win_begin, win_end, _ptr(out)))
        return out

    def msm_host(self, scalars) -> np.ndarray:
        sc = _as_u64(scalars, 4)
        out = np.zeros(18, dtype=np.uint64)
        _check(_msm_dbases_host(self._h, _ptr(sc), len(sc), _ptr(out)))
        return out

    def submit(self, d_scalars: int, n: int = None, window_bits: int = 0, win_begin: int = 0, win_end: int = -1) -> int:
        t = C.c_int(-1)
        _check(_msm_dbases_submit(self._h, d_scalars, self.n if n is None else n, window_bits, win_begin, win_end, C.byref(t)))
        return t.value


def _dacc_args(bases, inst, checks_u32, pool, xp, xs):
    inst, pool, xp, xs = _as_u64(inst, 12), _as_u64(pool, 4), _as_u64(xp, 12), _as_u64(xs, 4)
    checks = np.ascontiguousarray(checks_u32, dtype=np.uint32).reshape(-1, 35)
    if len(xp) != len(xs):
        raise ValueError("as many loose scalars as loose points")
    acc = C.c_void_p()
    _check(_dacc_begin(bases._h, _ptr(inst) if len(inst) else None, len(inst), C.byref(acc)))
    n_res = bases.n + len(inst)
    args = (_ptr(checks) if len(checks) else None, len(checks), _ptr(pool) if len(pool) else None, len(pool),
            _ptr(xp) if len(xp) else None, _ptr(xs) if len(xs) else None, len(xp))
    return acc, args, (checks, pool, xp, xs, inst), n_res


def dacc_run(bases: "DBases", inst, checks_u32, pool, xp, xs, export: bool = True):
    """curdle_dacc_begin + curdle_dacc_run over resident `bases` and the instance points `inst`: checks_u32 is
    (n_checks, 35) uint32 (curdle_dacc_check records), pool / xs Montgomery fr.Elements, xp the loose points.
    Returns (out_jac, slot scalars (n_res, 4)) -- the scalars are None without export."""
    acc, args, _keep, n_res = _dacc_args(bases, inst, checks_u32, pool, xp, xs)
    out = np.zeros(18, dtype=np.uint64)
    scalars = np.full((n_res, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if export else None
    _check(_dacc_run(acc, *args, _ptr(out), _ptr(scalars) if export and n_res else None))  # a failed run ends the accumulation
    return out, scalars


def dacc_run_members(bases: "DBases", inst, checks_u32, check_member, n_members: int, pool, xp, xs, extra_member,
                     export: bool = True, check_members: bool = True):
    """curdle_dacc_begin + curdle_dacc_run_members: the arguments of dacc_run plus the member (below n_members) of every
    check and of every loose pair.  Returns (sums (n_members, 18), slot scalars (n_members, n_res, 4) or None).  Array
    lengths that do not match and member indices outside [0, n_members) raise ValueError before anything is begun
    (check_members=False leaves the indices to the library, which refuses them with EINVAL)."""
    n_members = int(n_members)
    if n_members < 0:
        raise ValueError("n_members is negative")
    members = []
    for name, m, n in (("check_member", check_member, len(np.asarray(checks_u32).reshape(-1, 35))),
                       ("extra_member", extra_member, len(_as_u64(xp, 12)))):
        m = np.asarray(m if m is not None else [], dtype=np.int64).reshape(-1)
        if len(m) != n:
            raise ValueError(f"{name} has {len(m)} entries for {n}")
        if len(m) and (m.min() < 0 or m.max() >= (n_members if check_members else 1 << 32)):
            raise ValueError(f"{name} names a member outside [0, {n_members})")
        members.append(np.ascontiguousarray(m, dtype=np.uint32))
    cm_, xm_ = members
    acc, args, _keep, n_res = _dacc_args(bases, inst, checks_u32, pool, xp, xs)
    out = np.zeros((n_members, 18), dtype=np.uint64)
    scalars = np.full((n_members, n_res, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if export else None
    checks_p, n_checks, pool_p, pool_len, xp_p, xs_p, n_extra = args
    _check(_dacc_run_members(acc, checks_p, _ptr(cm_) if n_checks else None, n_checks, n_members, pool_p, pool_len, xp_p, xs_p,
                             _ptr(xm_) if n_extra else None, n_extra, _ptr(out) if n_members else None,
                             _ptr(scalars) if export and n_res and n_members else None))  # ends the accumulation either way
    return out, scalars


def msm_free_slots() -> int:
    """Workspace slots of the calling thread's context that no call holds right now (curdle_msm_free_slots)."""
    return int(_msm_free_slots())


def stat_dacc_members() -> dict:
    """curdle_stat_dacc_members: member-form accumulations run, members summed by them, members of failed batch groups
    that were still verified one by one."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_dacc_members(out))
    return dict(zip(("runs", "members", "one_by_one"), (int(v) for v in out)))


class DaccJob:
    """A submitted accumulation (curdle_dacc_submit): poll() / wait(), or abort()."""

    def __init__(self, acc, keep, scalars):
        self._acc, self._keep, self.scalars = acc, keep, scalars

    def __del__(self):          # dropped without wait / abort: the workspace slot goes back
        try:
            dacc_abort(self)
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass


def dacc_submit(bases: "DBases", inst, checks_u32, pool, xp, xs, export: bool = True) -> DaccJob:
    acc, args, keep, n_res = _dacc_args(bases, inst, checks_u32, pool, xp, xs)
    scalars = np.full((n_res, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if export else None
    _check(_dacc_submit(acc, *args, _ptr(scalars) if export and n_res else None))  # a failed submission ends the accumulation
    return DaccJob(acc, keep, scalars)


def dacc_poll(job: DaccJob) -> bool:
    done = C.c_int(0)
    _check(_dacc_poll(job._acc, C.byref(done)))
    return bool(done.value)


def dacc_wait(job: DaccJob):
    """(out_jac, slot scalars or None); ends the accumulation."""
    out = np.zeros(18, dtype=np.uint64)
    acc, job._acc = job._acc, None
    _check(_dacc_wait(acc, _ptr(out)))
    return out, job.scalars


def stat_dacc_builds() -> dict:
    """Launches of each build of the slot-scalar evaluation so far (curdle_stat_dacc_builds)."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_dacc_builds(out))
    return dict(zip(("front_lds", "front_global", "split_lds", "split_global"), (int(v) for v in out)))


def dacc_abort(job: DaccJob) -> None:
    if job._acc:
        acc, job._acc = job._acc, None
        _dacc_abort(acc)


def msm_wait(ticket: int) -> np.ndarray:
    out = np.zeros(18, dtype=np.uint64)
    _check(_msm_wait(ticket, _ptr(out)))
    return out


def window_bits(n: int) -> int:
    return _window_bits(n)


def num_windows(n: int, c: int = 0, flags: int = 0) -> int:
    """W of the plan a call with these flags runs: ceil(127 / c), or ceil(255 / c) with MSM_ANY_CURVE_POINT."""
    rc = _num_windows_ex(n, c, int(flags))
    if rc < 0:
        _check(rc)
    return rc


def window_widths(n: int, c: int = 0, flags: int = 0):
    """Widths (bits) of the Pippenger windows for (n, c, flags), lowest first; the top one is unsigned."""
    buf = (C.c_int * 64)()
    W = _window_widths_ex(n, c, int(flags), buf)
    if W < 0:
        _check(W)
    return [int(buf[i]) for i in range(W)]


def msm_g1_batch_device(d_points: int, d_scalars: int, offsets, stream: int = 0) -> np.ndarray:
    """k independent MSMs over device-resident, concatenated inputs -> uint64[k, 18]."""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_batch_device(d_points, d_scalars, _ptr(offs), k, _ptr(out), stream or None))
    return out


def g1_sum(jac_points) -> np.ndarray:
    jac_points = _as_u64(jac_points, 18)
    k = jac_points.shape[0] if jac_points.size else 0
    out = np.zeros(18, dtype=np.uint64)
    _check(_g1_sum(_ptr(jac_points), k, _ptr(out)))
    return out


def msm_g1_batch(points, scalars, offsets) -> np.ndarray:
    points = _as_u64(points, 12)
    scalars = _as_u64(scalars, 4)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)  # size_t
    k = len(offs) - 1
    out = np.zeros((k, 18), dtype=np.uint64)
    _check(_msm_batch(_ptr(points), _ptr(scalars), _ptr(offs), k, _ptr(out)))
    return out


def msm_g1_multi(points_sets, scalars) -> np.ndarray:
    sets = [_as_u64(p, 12) for p in points_sets]
    scalars = _as_u64(scalars, 4)
    n = scalars.shape[0] if scalars.size else 0
    for s in sets:
        if (s.shape[0] if s.size else 0) != n:
            raise CurdleError(EINVAL, "len(points) != len(scalars)")
    arr = (_vp * len(sets))(*[s.ctypes.data for s in sets])
    out = np.zeros((len(sets), 18), dtype=np.uint64)
    _check(_msm_multi(C.cast(arr, _vp), len(sets), _ptr(scalars), n, _ptr(out)))
    return out


class Rand:
    """common.Rand (common/rand.go) through the library's host mirror."""

    def __init__(self, seed: int):
        self._h = _rand_new(seed)
        if not self._h:
            raise MemoryError("curdle_rand_new")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _rand_free is not None:      # module globals may be gone at interpreter exit
            _rand_free(h)

    def get_fr(self) -> np.ndarray:
        out = np.zeros(4, dtype=np.uint64)
        _check(_rand_get_fr(self._h, _ptr(out)))
        return out

    def get_frs(self, n: int) -> np.ndarray:
        return np.array([self.get_fr() for _ in range(n)], dtype=np.uint64).reshape(n, 4)

    def get_g1_affine(self) -> np.ndarray:
        out = np.zeros(12, dtype=np.uint64)
        _check(_rand_get_g1(self._h, _ptr(out)))
        return out

    def get_g1_affines(self, n: int) -> np.ndarray:
        return np.array([self.get_g1_affine() for _ in range(n)], dtype=np.uint64).reshape(n, 12)

    def generate_permutation(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint32)
        _check(_rand_perm(self._h, n, _ptr(out)))
        return out


class MsmAccumulator:
    """msmaccumulator.MsmAccumulator (msmaccumulator/msmaccumulator.go:11-64)."""

    def __init__(self):
        self._h = _acc_new()
        if not self._h:
            raise MemoryError("curdle_acc_new")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _acc_free is not None:
            _acc_free(h)

    def accumulate_check(self, C_jac, x, v, rand: Rand) -> None:
        C_jac = _as_u64(C_jac)
        x = _as_u64(x, 4)
        v = _as_u64(v, 12)
        nx = x.shape[0] if x.size else 0
        nv = v.shape[0] if v.size else 0
        _check(_acc_check(self._h, _ptr(C_jac), _ptr(x), nx, _ptr(v), nv, rand._h))

    def accumulate_check_deferred(self, c_scalars, c_points, x, v, rand: Rand) -> None:
        """AccumulateCheck with C = sum_j c_scalars[j] * c_points[j] folded into the map."""
        cs = _as_u64(c_scalars, 4)
        cp = _as_u64(c_points, 12)
        x = _as_u64(x, 4)
        v = _as_u64(v, 12)
        n = lambda a: a.shape[0] if a.size else 0
        _check(_acc_check_deferred(self._h, _ptr(cs), _ptr(cp), n(cs), _ptr(x), n(x), _ptr(v), n(v), rand._h))

    def verify(self) -> bool:
        ok = C.c_int(0)
        _check(_acc_verify(self._h, C.byref(ok)))
        return bool(ok.value)

    @property
    def A_c(self) -> np.ndarray:
        out = np.zeros(18, dtype=np.uint64)
        _check(_acc_get_A_c(self._h, _ptr(out)))
        return out

    def num_bases(self) -> int:
        return _acc_num_bases(self._h)

    def export(self):
        n = self.num_bases()
        pts = np.zeros((n, 12), dtype=np.uint64)
        sc = np.zeros((n, 4), dtype=np.uint64)
        if n:
            _check(_acc_export(self._h, _ptr(pts), _ptr(sc)))
        return pts, sc


def profile_enable(on=True) -> None:
    """True / 1: HIP events around every kernel; 2: around the dominant kernel only; False / 0: off."""
    _check(_profile_enable(int(on)))


def profile_last() -> dict:
    p = _Profile()
    _check(_profile_last(C.byref(p)))
    return {
        "kernels": {p.name[i].decode(): float(p.ms[i]) for i in range(p.n_kernels)},
        "window_bits": p.window_bits,
        "num_windows": p.num_windows,
        "entries": int(p.entries),
        "fragments": int(p.fragments),
        "large_buckets": int(p.large_buckets),
    }


def selftest_shape(op: int):
    """(words read, words written) per item of selftest operation `op`: the library's own table."""
    iw, ow = C.c_uint32(0), C.c_uint32(0)
    _check(_selftest_shape(op, C.byref(iw), C.byref(ow)))
    return iw.value, ow.value


def selftest_op(op: int, inp: np.ndarray, on_device: bool) -> np.ndarray:
    """inp: uint32[n, in_width] -> uint32[n, out_width] (see curdle_selftest_op)."""
    iw, ow = selftest_shape(op)
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    assert inp.ndim == 2 and inp.shape[1] == iw, inp.shape
    out = np.zeros((inp.shape[0], ow), dtype=np.uint32)
    _check(_selftest_op(op, _ptr(inp), inp.shape[0], _ptr(out), 1 if on_device else 0))
    return out


def int_to_limbs(v: int, n: int = 4) -> np.ndarray:
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)], dtype=np.uint64)


def synth_points_walk_device(k: int, q: int, n: int, d_out: int) -> None:
    """P_i = (k + i*q) * G for i < n, written as gnark G1Affine into device memory at d_out
    (n * 96 bytes).  k, q are canonical integers < r."""
    ka, qa = int_to_limbs(k), int_to_limbs(q)
    _check(_synth_walk(_ptr(ka), _ptr(qa), n, d_out))


# ---------------------------------------------------------------------------
# Protocol layers (host restatement of curdleproof.Prove / Verify; include/curdle_msm.h)
# ---------------------------------------------------------------------------
CRS_N_BLINDERS = 4                                    # CURDLE_CRS_N_BLINDERS
CRS_MAX_ELL = 1 << 20                                 # CURDLE_CRS_MAX_ELL
CRS_TRUSTED = 1                                       # CURDLE_CRS_TRUSTED
CRS_GS, CRS_HS, CRS_H, CRS_GT, CRS_GU, CRS_GSUM, CRS_HSUM = range(7)      # CURDLE_CRS_GS ... CURDLE_CRS_HSUM
CRS_FIELDS = ("Gs", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum")
CRS_DUPLICATE, CRS_SUM_MISMATCH = 16, 17              # CURDLE_CRS_DUPLICATE, CURDLE_CRS_SUM_MISMATCH


class CrsPoints(C.Structure):                         # curdle_crs_points
    _fields_ = [("Gs", _vp), ("ell", C.c_size_t), ("Hs", _vp), ("H", _vp), ("Gt", _vp), ("Gu", _vp), ("Gsum", _vp),
                ("Hsum", _vp)]


class CrsFaultRecord(C.Structure):                    # curdle_crs_fault
    _fields_ = [("field", C.c_int), ("index", C.c_size_t), ("reason", C.c_int)]


class CrsFault(CurdleError):
    """A validated CRS import found a fault: which field (CRS_GS ... CRS_HSUM), which index within Gs or Hs, and why
    (a CURDLE_DECODE_* code, CRS_DUPLICATE or CRS_SUM_MISMATCH)."""

    def __init__(self, code: int, msg: str, field: int, index: int, reason: int):
        super().__init__(code, msg)
        self.field, self.index, self.reason = field, index, reason


_crs_from_points = _sig("curdle_crs_from_points", C.c_int, C.POINTER(CrsPoints), C.c_uint, C.POINTER(_vp),
                        C.POINTER(CrsFaultRecord))
_crs_from_bytes = _sig("curdle_crs_from_bytes", C.c_int, _vp, C.c_size_t, C.POINTER(_vp), C.POINTER(CrsFaultRecord))
_crs_export_points = _sig("curdle_crs_export_points", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
_crs_to_bytes = _sig("curdle_crs_to_bytes", C.c_int, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t))


class CRS:
    """curdleproof.CRS: from GenerateCRS(ell, rand) (crs.go:20), or imported with from_points / from_bytes."""

    def __init__(self, ell: int, rand: Rand):
        self._h = _crs_generate(ell, rand._h)
        if not self._h:
            raise MemoryError("curdle_crs_generate")
        self.ell = ell

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _crs_free is not None:
            _crs_free(h)

    @classmethod
    def _imported(cls, rc: int, handle, fault: CrsFaultRecord) -> "CRS":
        if rc != OK:
            if fault.field >= 0:
                raise CrsFault(rc, last_error(), fault.field, fault.index, fault.reason)
            raise CurdleError(rc, last_error())
        crs = cls.__new__(cls)
        crs._h = handle.value
        crs.ell = _crs_size(crs._h)
        return crs

    @classmethod
    def from_points(cls, Gs, Hs, H, Gt, Gu, Gsum, Hsum, flags: int = 0) -> "CRS":
        """curdle_crs_from_points: Gs uint64[ell, 12], Hs uint64[4, 12], H / Gt / Gu uint64[18] (G1Jac, any Z), Gsum /
        Hsum uint64[12].  Validated on the GPU (CrsFault names the first fault) unless flags = CRS_TRUSTED."""
        Gs, Hs, Gsum, Hsum = _as_u64(Gs, 12), _as_u64(Hs, 12), _as_u64(Gsum, 12), _as_u64(Hsum, 12)
        H, Gt, Gu = _as_u64(H, 18), _as_u64(Gt, 18), _as_u64(Gu, 18)
        if Hs.size != 12 * CRS_N_BLINDERS:
            raise ValueError(f"Hs holds {CRS_N_BLINDERS} points")
        pts = CrsPoints(_ptr(Gs), Gs.size // 12, _ptr(Hs), _ptr(H), _ptr(Gt), _ptr(Gu), _ptr(Gsum), _ptr(Hsum))
        handle, fault = _vp(), CrsFaultRecord(-1, 0, 0)
        rc = _crs_from_points(C.byref(pts), int(flags), C.byref(handle), C.byref(fault))
        return cls._imported(rc, handle, fault)

    @classmethod
    def from_bytes(cls, data: bytes) -> "CRS":
        """curdle_crs_from_bytes: the library's own wire form, 48 (ell + 9) bytes; always validated on the GPU."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        handle, fault = _vp(), CrsFaultRecord(-1, 0, 0)
        rc = _crs_from_bytes(_ptr(buf) if buf.size else None, buf.size, C.byref(handle), C.byref(fault))
        return cls._imported(rc, handle, fault)

    def points(self) -> dict:
        """curdle_crs_export_points: the seven fields by name, in the layouts from_points takes (H, Gt, Gu with Z = 1)."""
        out = {"Gs": np.zeros((self.ell, 12), np.uint64), "Hs": np.zeros((CRS_N_BLINDERS, 12), np.uint64),
               "H": np.zeros(18, np.uint64), "Gt": np.zeros(18, np.uint64), "Gu": np.zeros(18, np.uint64),
               "Gsum": np.zeros(12, np.uint64), "Hsum": np.zeros(12, np.uint64)}
        _check(_crs_export_points(self._h, *(_ptr(out[k]) for k in CRS_FIELDS)))
        return out

    def to_bytes(self) -> bytes:
        """curdle_crs_to_bytes: 48 (ell + 9) bytes."""
        buf = np.zeros(48 * (self.ell + CRS_N_BLINDERS + 5), dtype=np.uint8)
        n = C.c_size_t(0)
        _check(_crs_to_bytes(self._h, _ptr(buf), buf.size, C.byref(n)))
        return bytes(buf[: n.value])


SHUFFLE_CONSTANT_TIME = 1                             # CURDLE_SHUFFLE_CONSTANT_TIME


def shuffle_permute_commit(crs: CRS, Rs, Ss, perm, k, rand: Rand, flags=None):
    """common.ShufflePermuteCommit (common/util.go:45) -> (Ts, Us, M, rs_m).  flags: None calls the entry point without
    flags; an integer (0, SHUFFLE_CONSTANT_TIME) calls curdle_shuffle_permute_commit_ex with it."""
    Rs, Ss = _as_u64(Rs, 12), _as_u64(Ss, 12)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    k = _as_u64(k)
    ell = crs.ell
    Ts = np.zeros((ell, 12), dtype=np.uint64)
    Us = np.zeros((ell, 12), dtype=np.uint64)
    M = np.zeros(18, dtype=np.uint64)
    rs_m = np.zeros((4, 4), dtype=np.uint64)
    if flags is None:
        _check(_spc(crs._h, _ptr(Rs), _ptr(Ss), ell, _ptr(perm), _ptr(k), rand._h, _ptr(Ts), _ptr(Us), _ptr(M), _ptr(rs_m)))
    else:
        _check(_spc_ex(crs._h, _ptr(Rs), _ptr(Ss), ell, _ptr(perm), _ptr(k), rand._h, int(flags), _ptr(Ts), _ptr(Us), _ptr(M),
                       _ptr(rs_m)))
    return Ts, Us, M, rs_m


PROVE_MSM_CONSTANT_TIME = 1                           # CURDLE_PROVE_MSM_CONSTANT_TIME
_prove_ex = _sig("curdle_prove_ex", C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, C.c_uint, _vp,
                 C.c_size_t, C.POINTER(C.c_size_t))


def prove(crs: CRS, Rs, Ss, Ts, Us, M, perm, k, rs_m, rand: Rand, flags=None) -> bytes:
    """curdleproof.Prove (curdleproof.go:38); returns the serialised proof.  flags: None calls the entry point without
    flags; an integer (0, PROVE_MSM_CONSTANT_TIME) calls curdle_prove_ex with it."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M, k, rs_m = _as_u64(M), _as_u64(k), _as_u64(rs_m)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    cap = 1 << 16
    buf = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    if flags is None:
        _check(_prove(crs._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), _ptr(perm), _ptr(k), _ptr(rs_m),
                      rand._h, _ptr(buf), cap, C.byref(n)))
    else:
        _check(_prove_ex(crs._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), _ptr(perm), _ptr(k),
                         _ptr(rs_m), rand._h, int(flags), _ptr(buf), cap, C.byref(n)))
    return bytes(buf[: n.value])


_prove_ct = _sig("curdle_prove_ct", C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t,
                 C.POINTER(C.c_size_t))
_stat_host_point_mul = _sig("curdle_stat_host_point_mul", C.c_int, C.POINTER(C.c_ulonglong))
_fr_permute_ct = _sig("curdle_fr_permute_ct", C.c_int, _vp, _vp, C.c_size_t, _vp)
_fr_permute_ct_device = _sig("curdle_fr_permute_ct_device", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp)
_stat_fr_permute_ct = _sig("curdle_stat_fr_permute_ct", C.c_int, C.POINTER(C.c_ulonglong))


def prove_ct(crs: CRS, Rs, Ss, Ts, Us, M, perm, k, rs_m, rand: Rand) -> bytes:
    """prove() in constant-time form (curdle_prove_ct): the same proof bytes and the same draws from rand, with the
    prover's MSMs, its scalar multiplications by secrets and its gathers by the permutation on kernels whose
    instruction and address streams do not depend on them.  ell <= 4,096; no fallback without a device."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M, k, rs_m = _as_u64(M), _as_u64(k), _as_u64(rs_m)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    cap = 1 << 16
    buf = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    _check(_prove_ct(crs._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), _ptr(perm), _ptr(k), _ptr(rs_m),
                     rand._h, _ptr(buf), cap, C.byref(n)))
    return bytes(buf[: n.value])


def stat_host_point_mul() -> int:
    """Calls of the host's double-and-add scalar multiplication (alg::Point::Mul) on the CALLING THREAD so far."""
    out = C.c_ulonglong(0)
    _check(_stat_host_point_mul(C.byref(out)))
    return int(out.value)


def fr_permute_ct(records, perm) -> np.ndarray:
    """out[i] = records[perm[i]] over 32-byte records with perm secret (curdle_fr_permute_ct): every output reads every
    record and no address is made of perm; an entry at or above n gives a zero record.  n <= 4,096."""
    records = _as_u64(records, 4)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    n = records.shape[0] if records.size else 0
    if len(perm) != n:
        raise CurdleError(EINVAL, "len(perm) != len(records)")
    out = np.zeros((n, 4), dtype=np.uint64)
    _check(_fr_permute_ct(_ptr(records), _ptr(perm), n, _ptr(out)))
    return out


def fr_permute_ct_device(d_in: int, d_perm: int, n: int, d_out: int, stream: int = 0) -> None:
    """fr_permute_ct on device-resident arrays (curdle_fr_permute_ct_device; raw device pointers, the records'
    multiples of 16 and not overlapping, the permutation's a multiple of 4)."""
    _check(_fr_permute_ct_device(d_in or None, d_perm or None, n, d_out or None, stream or None))


def stat_fr_permute_ct() -> dict:
    """Records gathered by the oblivious scalar gather and its launches since the library was loaded."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_fr_permute_ct(out))
    return {"records": int(out[0]), "launches": int(out[1])}


_fr_permute_ct_batch = _sig("curdle_fr_permute_ct_batch", C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp)
_fr_permute_ct_batch_device = _sig("curdle_fr_permute_ct_batch_device", C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp)
_g1_permute_ct_batch_device = _sig("curdle_g1_permute_ct_batch_device", C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp)


def fr_permute_ct_batch(records, perm, n: int, k: int) -> np.ndarray:
    """k oblivious gathers of one n in one launch (curdle_fr_permute_ct_batch): out[j n + i] = records[j n + perm[j n + i]]
    over 32-byte records; an entry at or above n gives a zero record, never another member's.  records: (k n, 4) uint64,
    perm: k n uint32.  n <= 4,096, k <= 4,096, k n <= 2^20."""
    records = _as_u64(records, 4)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    if k * n and (records.shape[0] != k * n or len(perm) != k * n):
        raise CurdleError(EINVAL, "records and perm need k n entries")
    out = np.zeros((k * n, 4), dtype=np.uint64)
    _check(_fr_permute_ct_batch(_ptr(records), _ptr(perm), n, k, _ptr(out)))
    return out


def fr_permute_ct_batch_device(d_in: int, d_perm: int, n: int, k: int, d_out: int, stream: int = 0) -> None:
    """fr_permute_ct_batch on device-resident arrays (curdle_fr_permute_ct_batch_device; the pointer rules of
    fr_permute_ct_device)."""
    _check(_fr_permute_ct_batch_device(d_in or None, d_perm or None, n, k, d_out or None, stream or None))


def g1_permute_ct_batch_device(d_in: int, d_perm: int, n: int, k: int, d_out: int, stream: int = 0) -> None:
    """The same batched gather over 96-byte records, device-resident (curdle_g1_permute_ct_batch_device)."""
    _check(_g1_permute_ct_batch_device(d_in or None, d_perm or None, n, k, d_out or None, stream or None))


PROVE_BATCH_CONSTANT_TIME = 1                         # CURDLE_PROVE_BATCH_CONSTANT_TIME
_prove_batch = _sig("curdle_prove_batch", C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                    C.c_uint, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int))
_stat_prove_batch = _sig("curdle_stat_prove_batch", C.c_int, C.POINTER(C.c_ulonglong))


def prove_batch(crs: CRS, members, flags: int = 0):
    """k proofs over one CRS in lockstep (curdle_prove_batch): members is a list of (Rs, Ss, Ts, Us, M, perm, k, rs_m,
    rand) as prove() takes them, with k distinct Rand objects.  flags: 0 gives prove()'s bytes per member,
    PROVE_BATCH_CONSTANT_TIME prove_ct()'s.  Returns (proofs, status): a list of bytes (empty for a member that failed
    on its own) and the list of per-member codes; raises CurdleError when the call itself is refused or the device fails."""
    k = len(members)
    keep, cols = [], [[] for _ in range(6)]
    Ms = np.zeros((k, 18), dtype=np.uint64)
    ks = np.zeros((k, 4), dtype=np.uint64)
    rs_ms = np.zeros((k, 16), dtype=np.uint64)
    rands = (C.c_void_p * max(k, 1))()
    for i, (Rs, Ss, Ts, Us, M, perm, kk, rs_m, rand) in enumerate(members):
        arrs = [_as_u64(a, 12) for a in (Rs, Ss, Ts, Us)] + [np.ascontiguousarray(perm, dtype=np.uint32)]
        keep.append(arrs)
        for c, a in zip(cols, arrs):
            c.append(a.ctypes.data)
        Ms[i], ks[i], rs_ms[i] = _as_u64(M).reshape(18), _as_u64(kk).reshape(4), _as_u64(rs_m).reshape(16)
        rands[i] = rand._h
    ptrs = [(C.c_void_p * max(k, 1))(*c) for c in cols[:5]]
    stride = 1 << 16
    buf = np.zeros(max(k, 1) * stride, dtype=np.uint8)
    lens = (C.c_size_t * max(k, 1))()
    status = (C.c_int * max(k, 1))()
    ell = keep[0][0].shape[0] if k else crs.ell          # the members' ell: the call checks it against the CRS
    if any(a.shape[0] != ell for arrs in keep for a in arrs):
        raise CurdleError(EINVAL, "every member needs ell points in Rs, Ss, Ts, Us and ell entries in perm")
    _check(_prove_batch(crs._h, k, ell, ptrs[0], ptrs[1], ptrs[2], ptrs[3], _ptr(Ms), ptrs[4], _ptr(ks), _ptr(rs_ms),
                        rands, int(flags), _ptr(buf), stride, lens, status))
    return [bytes(buf[stride * i: stride * i + lens[i]]) for i in range(k)], [int(status[i]) for i in range(k)]


def stat_prove_batch() -> dict:
    """Batch proving since the library was loaded: calls, members, lockstep groups, coalesced device calls."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_prove_batch(out))
    return {"calls": int(out[0]), "members": int(out[1]), "groups": int(out[2]), "device_calls": int(out[3])}


def verify(crs: CRS, proof: bytes, Rs, Ss, Ts, Us, M, rand: Rand) -> bool:
    """curdleproof.Verify (curdleproof.go:199): the accept bit; raises CurdleError for (false, err)."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M = _as_u64(M)
    pb = np.frombuffer(proof, dtype=np.uint8).copy()
    ok = C.c_int(0)
    _check(_verify(crs._h, _ptr(pb), len(pb), _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), rand._h,
                   C.byref(ok)))
    return bool(ok.value)


_verify_checked = _sig("curdle_verify_checked", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                       C.POINTER(C.c_int))
_verify_proof_checked = _sig("curdle_verify_proof_checked", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp,
                             C.POINTER(C.c_int))
_stat_check_paths = _sig("curdle_stat_check_paths", C.c_int, C.POINTER(C.c_ulonglong))


def verify_checked(crs: CRS, proof: bytes, Rs, Ss, Ts, Us, M, rand: Rand) -> bool:
    """verify() with the instance points checked (range, curve, subgroup; g1_check_batch) on the GPU beside the
    verification and M on the host: CurdleError(EINVAL, "Ss[17]: not in the prime-order subgroup") for a bad one."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M = _as_u64(M)
    pb = np.frombuffer(proof, dtype=np.uint8).copy()
    ok = C.c_int(0)
    _check(_verify_checked(crs._h, _ptr(pb), len(pb), _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), rand._h,
                           C.byref(ok)))
    return bool(ok.value)


def stat_check_paths() -> dict:
    """Checked verifications so far whose point check ran beside the verification / ran to its end first; the second
    also counts every g1_check_batch / g1_check_jac_batch call (a validated CRS.from_points makes one of each)."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_check_paths(out))
    return {"beside": int(out[0]), "first": int(out[1])}


class Proof:
    """A decoded curdleproof.Proof (Proof.FromReader, curdleproof.go:320: every point curve- and
    subgroup-checked).  verify_proof() is the reference's Verify(proof Proof, ...) on it."""

    def __init__(self, data: bytes):
        pb = np.frombuffer(data, dtype=np.uint8).copy()
        h = _vp()
        _check(_proof_from_bytes(_ptr(pb), len(pb), C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _proof_free is not None:
            _proof_free(h)


def verify_proof(crs: CRS, proof: Proof, Rs, Ss, Ts, Us, M, rand: Rand) -> bool:
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M = _as_u64(M)
    ok = C.c_int(0)
    _check(_verify_proof(crs._h, proof._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), rand._h, C.byref(ok)))
    return bool(ok.value)


def verify_proof_checked(crs: CRS, proof: Proof, Rs, Ss, Ts, Us, M, rand: Rand) -> bool:
    """verify_proof() with the instance points checked, as verify_checked()."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M = _as_u64(M)
    ok = C.c_int(0)
    _check(_verify_proof_checked(crs._h, proof._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), rand._h,
                                 C.byref(ok)))
    return bool(ok.value)


class PreparedVerify:
    """The arguments of curdle_verify_proof marshalled once (the instance arrays as C pointers), so that run() is
    the C call and nothing else: what a benchmark of the verifier should time -- the reference's BenchmarkVerifier
    (curdleproof_test.go:210-237) times Verify on values that are already in memory, and five numpy -> ctypes
    conversions per call are ~15 us of a 0.8 ms verification."""

    def __init__(self, crs: CRS, proof: Proof, Rs, Ss, Ts, Us, M):
        self._keep = [_as_u64(a, 12) for a in (Rs, Ss, Ts, Us)] + [_as_u64(M)]
        self._args = (crs._h, proof._h, *[_ptr(a) for a in self._keep[:4]], crs.ell, _ptr(self._keep[4]))
        self._crs, self._proof = crs, proof      # keep the handles alive
        self._ok = C.c_int(0)
        self._okref = C.byref(self._ok)

    def run(self, rand: Rand) -> bool:
        _check(_verify_proof(*self._args, rand._h, self._okref))
        return bool(self._ok.value)


class PreparedVerifyBatch:
    """The arguments of curdle_verify_batch marshalled once (pointer tables over contiguous
    arrays), so that run() is the C call and nothing else -- what a benchmark should time, and
    what a caller verifying the same batch layout repeatedly wants."""

    def __init__(self, proofs, Rs, Ss, Ts, Us, Ms):
        k = self.k = len(proofs)
        self._keep = []

        def ptr_array(arrs, width):
            a = [_as_u64(x, width) for x in arrs]
            self._keep.append(a)
            return (C.c_void_p * k)(*[x.ctypes.data for x in a])

        self._pbufs = [np.frombuffer(p, dtype=np.uint8).copy() for p in proofs]
        self._pp = (C.c_void_p * k)(*[b.ctypes.data for b in self._pbufs])
        self._lens = (C.c_size_t * k)(*[len(b) for b in self._pbufs])
        self._ms = np.ascontiguousarray(np.stack([_as_u64(m) for m in Ms]) if k else np.zeros((0, 18), dtype=np.uint64))
        self._inst = [ptr_array(v, 12) for v in (Rs, Ss, Ts, Us)]

    def run(self, crs: CRS, rand: Rand, nthreads: int = 8):
        oks = (C.c_int * self.k)()
        _check(_verify_batch(crs._h, self.k, self._pp, self._lens, *self._inst, crs.ell, _ptr(self._ms), rand._h,
                             int(nthreads), oks))
        return [bool(v) for v in oks]

    def run_checked(self, crs: CRS, rand: Rand, nthreads: int = 8):
        """curdle_verify_batch_checked on the same arguments: (accept bits, the curdle_point_fault records)."""
        oks = (C.c_int * self.k)()
        faults = np.zeros(self.k, dtype=POINT_FAULT)
        _check(_verify_batch_checked(crs._h, self.k, self._pp, self._lens, *self._inst, crs.ell, _ptr(self._ms), rand._h,
                                     int(nthreads), oks, _ptr(faults)))
        return [bool(v) for v in oks], faults


def verify_batch(crs: CRS, proofs, Rs, Ss, Ts, Us, Ms, rand: Rand, nthreads: int = 8):
    """Cross-proof batch verification: k proofs over one CRS, one shared accumulator, one MSM.
    proofs: list of bytes; Rs/Ss/Ts/Us: lists of (ell, 12) arrays; Ms: list of 18-limb points.
    Returns the list of accept bits (exact: a failing group is settled by one sum per member, curdle_dacc_run_members)."""
    return PreparedVerifyBatch(proofs, Rs, Ss, Ts, Us, Ms).run(crs, rand, nthreads)


_verify_batch_checked = _sig("curdle_verify_batch_checked", C.c_int, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp,
                             _vp, C.c_int, _vp, _vp)
_stat_batch_checked = _sig("curdle_stat_batch_checked", C.c_int, C.POINTER(C.c_ulonglong))
POINT_FAULT = np.dtype([("code", np.uint8), ("vector", np.uint8), ("pad", np.uint16), ("index", np.uint32)])  # curdle_point_fault
FAULT_VECTORS = ("Rs", "Ss", "Ts", "Us", "M")


def verify_batch_checked(crs: CRS, proofs, Rs, Ss, Ts, Us, Ms, rand: Rand, nthreads: int = 8):
    """verify_batch() with every member's 4 ell instance points and its M checked (range, curve, subgroup) on the GPU,
    in chunks beside the verification.  Returns (oks, faults): faults[i] is None, or (vector name, index, DECODE_*
    code) of member i's first failed point in the order Rs, Ss, Ts, Us, M -- such a member is never verified and has
    oks[i] False; every other member has the bit verify_batch() gives it from the same rand state."""
    oks, faults = PreparedVerifyBatch(proofs, Rs, Ss, Ts, Us, Ms).run_checked(crs, rand, nthreads)
    return (oks, [None if f["code"] <= DECODE_INFINITY else (FAULT_VECTORS[f["vector"]], int(f["index"]), int(f["code"]))
                  for f in faults])


def stat_batch_checked() -> dict:
    """Checked batches since the library was loaded, members their point check rejected, chunks checked."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_batch_checked(out))
    return {"batches": out[0], "rejected": out[1], "chunks": out[2]}


# ---- batched Merlin transcripts (curdle_transcript_batch / _host) ----
TRANSCRIPT_STATE_SIZE = 208
TR_APPEND, TR_CHALLENGES = 1, 2
TRANSCRIPT_MAX_TRIES = 256
TRANSCRIPT_MAX_MEMBERS, TRANSCRIPT_MAX_BYTES, TRANSCRIPT_MAX_CHALLENGES, TRANSCRIPT_MAX_MESSAGES = 65536, 1 << 20, 4096, 65536


class _TranscriptStep(C.Structure):      # curdle_transcript_step
    _fields_ = [("op", C.c_uint32), ("count", C.c_uint32), ("len", C.c_uint32), ("label_len", C.c_uint32), ("label", C.c_char * 32)]


_tr_args = (C.c_char_p, _vp, C.POINTER(_TranscriptStep), C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp)
_transcript_batch = _sig("curdle_transcript_batch", C.c_int, *_tr_args)
_transcript_batch_host = _sig("curdle_transcript_batch_host", C.c_int, *_tr_args, C.c_int)
_stat_transcript = _sig("curdle_stat_transcript", C.c_int, C.POINTER(C.c_ulonglong))
_transcript_last_kernel_ms = _sig("curdle_transcript_last_kernel_ms", C.c_int, C.POINTER(C.c_double))


def transcript_steps(program):
    """program: [(op, label: bytes, count, len)] -> (curdle_transcript_step array, bytes a member's program reads,
    challenges per member).  Nothing is checked here: the library refuses what is malformed."""
    steps = (_TranscriptStep * max(1, len(program)))()
    consumed = n_ch = 0
    for s, (op, label, count, ln) in zip(steps, program):
        s.op, s.count, s.len, s.label_len = op, count, ln, len(label)
        s.label = bytes(label[:32])
        consumed += count * ln if op == TR_APPEND else 0
        n_ch += count if op == TR_CHALLENGES else 0
    return steps, consumed, n_ch


def transcript_batch(program, data, label=None, init_states=None, want_states=True, host=False, nthreads=1, data_stride=None):
    """curdle_transcript_batch (host=True: curdle_transcript_batch_host on nthreads threads): the program
    [(TR_APPEND | TR_CHALLENGES, label, count, len)] over the k rows of `data` (k x stride uint8; a fresh transcript
    `label` for every member, or k exported states in init_states).  Returns (challenges k x n x 32 big-endian bytes,
    states k x 208 or None, status k)."""
    steps, _, n_ch = transcript_steps(program)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    k = data.shape[0]
    stride = data.shape[1] if data_stride is None else data_stride
    init = None if init_states is None else np.ascontiguousarray(init_states, dtype=np.uint8)
    ch = np.zeros((k, n_ch, 32), dtype=np.uint8)
    st = np.zeros((k, TRANSCRIPT_STATE_SIZE), dtype=np.uint8) if want_states else None
    status = np.zeros(k, dtype=np.uint8)
    args = (label, None if init is None else _ptr(init), steps, len(program), _ptr(data) if data.size else None, stride, k,
            _ptr(ch) if ch.size else None, None if st is None else _ptr(st), _ptr(status))
    _check(_transcript_batch_host(*args, nthreads) if host else _transcript_batch(*args))
    return ch, st, status


def stat_transcript() -> dict:
    """Members hashed on the device since the library was loaded, and members handed back with a non-zero status."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_transcript(out))
    return {"members": out[0], "handed_back": out[1]}


def transcript_last_kernel_ms() -> float:
    out = C.c_double()
    _check(_transcript_last_kernel_ms(C.byref(out)))
    return out.value


_stat_transcript_paths = _sig("curdle_stat_transcript_paths", C.c_int, C.POINTER(C.c_ulonglong))
_keccak_permute_batch = _sig("curdle_keccak_permute_batch", C.c_int, _vp, C.c_size_t, C.c_uint, C.c_uint, _vp, C.POINTER(C.c_double))
KECCAK_PERMUTE_MAX_REPS, KECCAK_PERMUTE_MAX_STATES = 4096, 65536
KECCAK_LANE, KECCAK_SHEET = 0, 1


def stat_transcript_paths() -> dict:
    """Members since the library was loaded whose transcripts the lane kernel hashed, and the sheet kernel (knob
    TRANSCRIPT_SHEET), counted at the launch: the tracker batches' device-hashed members are in it."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_transcript_paths(out))
    return {"lane": out[0], "sheet": out[1]}


_msm_reduce_plan = _sig("curdle_msm_reduce_plan", C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32))


def msm_reduce_plan(n: int, window_bits: int = 0, win_begin: int = 0, win_end: int = -1, pipelined: bool = False) -> dict:
    """What the plan of one device-resident MSM of n pairs decides about its bucket reduction (curdle_msm_reduce_plan),
    under the knobs as they stand; no device needed."""
    out = (C.c_uint32 * 8)()
    _check(_msm_reduce_plan(n, window_bits, win_begin, win_end, 1 if pipelined else 0, out))
    names = ("reduce_bits", "two_level", "seg", "G", "NS", "window_bits", "max_small", "L")
    return {k: int(v) for k, v in zip(names, out)}


_msm_stream_plan = _sig("curdle_msm_stream_plan", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32))
STREAM_PLAN_AUTO, STREAM_PLAN_WIDE, STREAM_PLAN_COMPACT = 0, 1, 2      # values of the STREAM_PLAN knob


def msm_stream_plan(hw_queues: int, window_range: bool = False) -> dict:
    """The streams pipelined calls keep busy on a context created in a process with `hw_queues` hardware queues
    (GPU_MAX_HW_QUEUES; the HIP runtime's default is 4), for whole MSMs or window ranges, under the knobs as they
    stand (curdle_msm_stream_plan); no device needed."""
    out = (C.c_uint32 * 4)()
    _check(_msm_stream_plan(int(hw_queues), 1 if window_range else 0, out))
    plan = {"plan": {STREAM_PLAN_WIDE: "wide", STREAM_PLAN_COMPACT: "compact"}[int(out[0])],
            "main_streams": int(out[1]), "pre_streams": int(out[2]), "tail_streams": int(out[3])}
    plan["busy_streams"] = plan["main_streams"] + plan["pre_streams"] + plan["tail_streams"]
    return plan


def keccak_permute_batch(states, form: int, reps: int = 1, want_ms: bool = False):
    """curdle_keccak_permute_batch: `reps` dependent Keccak-f[1600] on each row of `states` (n x 25 uint64) on the
    device; form KECCAK_LANE (a state per lane, one per wave) or KECCAK_SHEET (a state spread over lanes).  Returns
    the n x 25 result, with want_ms (result, the kernel's ms by HIP events)."""
    a = np.ascontiguousarray(states, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 25:
        raise ValueError(f"expected n x 25 words, got {a.shape}")
    out = np.zeros_like(a)
    ms = C.c_double()
    _check(_keccak_permute_batch(_ptr(a), a.shape[0], form, reps, _ptr(out), C.byref(ms)))
    return (out, ms.value) if want_ms else out


# ---- whisk package (whisk/whisk.go, whisk/types.go): trackers are 96-byte strings rG || krG ----
WHISK_ELL = 124
WHISK_TRACKER_PROOF_SIZE = 128
WHISK_SHUFFLE_PROOF_SIZE = 4576


def _bytes_arr(b: bytes) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


def whisk_is_valid_shuffle_proof(crs: CRS, pre_trackers, post_trackers, proof: bytes, rand: Rand) -> bool:
    """IsValidWhiskShuffleProof (whisk.go:20): trackers are lists of 96-byte strings."""
    if len(proof) != WHISK_SHUFFLE_PROOF_SIZE:
        raise ValueError("a whisk shuffle proof is %d bytes" % WHISK_SHUFFLE_PROOF_SIZE)
    pre, post, pb = _bytes_arr(b"".join(pre_trackers)), _bytes_arr(b"".join(post_trackers)), _bytes_arr(proof)
    ok = C.c_int(0)
    _check(_whisk_valid_shuffle(crs._h, _ptr(pre), _ptr(post), len(pre_trackers), len(post_trackers), _ptr(pb), rand._h,
                                C.byref(ok)))
    return bool(ok.value)


class PreparedWhiskBatch:
    """The arguments of curdle_whisk_is_valid_shuffle_proof_batch marshalled once; run() is the
    C call and nothing else (see PreparedVerifyBatch)."""

    def __init__(self, pre_sets, post_sets, proofs):
        k = self.k = len(proofs)
        n = self.n = len(pre_sets[0]) if k else 0
        self._pre = [_bytes_arr(b"".join(s)) for s in pre_sets]
        self._post = [_bytes_arr(b"".join(s)) for s in post_sets]
        self._pb = [_bytes_arr(p) for p in proofs]
        if any(len(a) != 96 * n for a in self._pre + self._post) or any(len(p) != WHISK_SHUFFLE_PROOF_SIZE for p in self._pb):
            raise ValueError("every tracker set needs the same length; proofs are %d bytes" % WHISK_SHUFFLE_PROOF_SIZE)
        arr = lambda bufs: (C.c_void_p * k)(*[b.ctypes.data for b in bufs])
        self._ptrs = (arr(self._pre), arr(self._post), arr(self._pb))

    def run(self, crs: CRS, rand: Rand, nthreads: int = 16):
        oks = (C.c_int * self.k)()
        _check(_whisk_valid_shuffle_batch(crs._h, self.k, self._ptrs[0], self._ptrs[1], self.n, self._ptrs[2], rand._h,
                                          int(nthreads), oks))
        return [bool(v) for v in oks]


def whisk_is_valid_shuffle_proof_batch(crs: CRS, pre_sets, post_sets, proofs, rand: Rand, nthreads: int = 16):
    """k shuffle proofs at once: pre_sets / post_sets are lists of tracker lists (all the same
    length), proofs a list of 4,576-byte strings.  Returns the list of accept bits."""
    return PreparedWhiskBatch(pre_sets, post_sets, proofs).run(crs, rand, nthreads)


def whisk_generate_shuffle_proof(crs: CRS, pre_trackers, rand: Rand):
    """GenerateWhiskShuffleProof (whisk.go:63) -> (post_trackers, proof bytes)."""
    pre = _bytes_arr(b"".join(pre_trackers))
    post = np.zeros(96 * len(pre_trackers), dtype=np.uint8)
    proof = np.zeros(WHISK_SHUFFLE_PROOF_SIZE, dtype=np.uint8)
    _check(_whisk_gen_shuffle(crs._h, _ptr(pre), len(pre_trackers), rand._h, _ptr(post), _ptr(proof)))
    pb = post.tobytes()
    return [pb[96 * i: 96 * (i + 1)] for i in range(len(pre_trackers))], proof.tobytes()


_whisk_gen_shuffle_ct = _sig("curdle_whisk_generate_shuffle_proof_ct", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp)


def whisk_generate_shuffle_proof_ct(crs: CRS, pre_trackers, rand: Rand):
    """whisk_generate_shuffle_proof in constant-time form (curdle_whisk_generate_shuffle_proof_ct): the same
    post-trackers, proof bytes and draws, through the flagged shuffle step and prove_ct."""
    pre = _bytes_arr(b"".join(pre_trackers))
    post = np.zeros(96 * len(pre_trackers), dtype=np.uint8)
    proof = np.zeros(WHISK_SHUFFLE_PROOF_SIZE, dtype=np.uint8)
    _check(_whisk_gen_shuffle_ct(crs._h, _ptr(pre), len(pre_trackers), rand._h, _ptr(post), _ptr(proof)))
    pb = post.tobytes()
    return [pb[96 * i: 96 * (i + 1)] for i in range(len(pre_trackers))], proof.tobytes()


_prover_ct_create = _sig("curdle_prover_ct_create", C.c_int, _vp, C.c_uint, C.POINTER(C.c_void_p))
_prover_ct_free = _sig("curdle_prover_ct_free", None, _vp)
_prover_ct_prove = _sig("curdle_prover_ct_prove", C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp,
                        C.c_size_t, C.POINTER(C.c_size_t))
_prover_ct_whisk = _sig("curdle_prover_ct_whisk_shuffle_proof", C.c_int, _vp, _vp, C.c_size_t, _vp, _vp, _vp)
_stat_alg_msm_resident = _sig("curdle_stat_alg_msm_resident", C.c_int, C.POINTER(C.c_ulonglong))


class ProverCt:
    """A constant-time prover over one CRS (curdle_prover_ct): the CRS's points live in a constant-time base table made
    once, and every MSM of a Prove walks chunk_bits steps over resident tables instead of 255.  prove() and
    whisk_shuffle_proof() give prove_ct's and whisk_generate_shuffle_proof_ct's bytes and draws.  The CRS must outlive
    the handle (this object keeps a reference)."""

    def __init__(self, crs: CRS, chunk_bits: int = 0):
        self._h = C.c_void_p()
        self.crs = crs
        _check(_prover_ct_create(crs._h, int(chunk_bits), C.byref(self._h)))

    def free(self):
        if self._h:
            _prover_ct_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:       # noqa: BLE001 -- interpreter shutdown
            pass

    def prove(self, Rs, Ss, Ts, Us, M, perm, k, rs_m, rand: Rand) -> bytes:
        Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
        M, k, rs_m = _as_u64(M), _as_u64(k), _as_u64(rs_m)
        perm = np.ascontiguousarray(perm, dtype=np.uint32)
        cap = 1 << 16
        buf = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t(0)
        _check(_prover_ct_prove(self._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), self.crs.ell, _ptr(M), _ptr(perm), _ptr(k),
                                _ptr(rs_m), rand._h, _ptr(buf), cap, C.byref(n)))
        return bytes(buf[: n.value])

    def whisk_shuffle_proof(self, pre_trackers, rand: Rand):
        pre = _bytes_arr(b"".join(pre_trackers))
        post = np.zeros(96 * len(pre_trackers), dtype=np.uint8)
        proof = np.zeros(WHISK_SHUFFLE_PROOF_SIZE, dtype=np.uint8)
        _check(_prover_ct_whisk(self._h, _ptr(pre), len(pre_trackers), rand._h, _ptr(post), _ptr(proof)))
        pb = post.tobytes()
        return [pb[96 * i: 96 * (i + 1)] for i in range(len(pre_trackers))], proof.tobytes()


def stat_alg_msm_resident() -> dict:
    """The funnel's calls under an alg::ResidentBasesScope: those that went to the MSM over resident tables and their
    pairs, and those that took the unchunked constant-time path and their pairs."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_alg_msm_resident(out))
    return {"resident_calls": int(out[0]), "resident_pairs": int(out[1]), "fallback_calls": int(out[2]),
            "fallback_pairs": int(out[3])}


_whisk_gen_shuffle_batch = _sig("curdle_whisk_generate_shuffle_proof_batch", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp,
                                C.c_uint, _vp, _vp, C.POINTER(C.c_int))


def whisk_generate_shuffle_proof_batch(crs: CRS, pre_sets, rands, flags: int = 0):
    """whisk_generate_shuffle_proof for k pre-tracker lists of one length in lockstep
    (curdle_whisk_generate_shuffle_proof_batch), with k distinct Rand objects; under PROVE_BATCH_CONSTANT_TIME
    whisk_generate_shuffle_proof_ct's results.  Returns (post_sets, proofs, status); a member with a non-zero status has
    None for both."""
    k = len(pre_sets)
    n = len(pre_sets[0]) if k else 0
    pre = [_bytes_arr(b"".join(s)) for s in pre_sets]
    if any(len(a) != 96 * n for a in pre):
        raise ValueError("every tracker set needs the same length")
    ptrs = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in pre])
    rh = (C.c_void_p * max(k, 1))(*[r._h for r in rands])
    post = np.zeros(max(1, 96 * n * k), dtype=np.uint8)
    proofs = np.zeros(max(1, WHISK_SHUFFLE_PROOF_SIZE * k), dtype=np.uint8)
    status = (C.c_int * max(k, 1))()
    _check(_whisk_gen_shuffle_batch(crs._h, k, ptrs, n, rh, int(flags), _ptr(post), _ptr(proofs), status))
    pb, fb = post.tobytes(), proofs.tobytes()
    posts = [[pb[96 * (n * i + t): 96 * (n * i + t + 1)] for t in range(n)] if status[i] == 0 else None for i in range(k)]
    prs = [fb[WHISK_SHUFFLE_PROOF_SIZE * i: WHISK_SHUFFLE_PROOF_SIZE * (i + 1)] if status[i] == 0 else None for i in range(k)]
    return posts, prs, [int(status[i]) for i in range(k)]


def whisk_is_valid_tracker_proof(tracker: bytes, k_commitment: bytes, proof: bytes) -> bool:
    """IsValidWhiskTrackerProof (whisk.go:116)."""
    if len(tracker) != 96 or len(k_commitment) != 48 or len(proof) != WHISK_TRACKER_PROOF_SIZE:
        raise ValueError("tracker 96 B, k commitment 48 B, tracker proof 128 B")
    t, kc, pb = _bytes_arr(tracker), _bytes_arr(k_commitment), _bytes_arr(proof)
    ok = C.c_int(0)
    _check(_whisk_valid_tracker(_ptr(t), _ptr(kc), _ptr(pb), C.byref(ok)))
    return bool(ok.value)


TRACKER_HASH_DEFAULT, TRACKER_HASH_HOST, TRACKER_HASH_DEVICE = 0, 1, 2


def whisk_is_valid_tracker_proof_batch(trackers, k_commitments, proofs, flags=None) -> np.ndarray:
    """k tracker proofs at once on the GPU (curdle_whisk_is_valid_tracker_proof_batch): lists of
    96-byte trackers, 48-byte k commitments and 128-byte proofs.  Returns int32[k]: 1 accept,
    0 reject, EINVAL where whisk_is_valid_tracker_proof raises CurdleError with EINVAL.
    flags: TRACKER_HASH_* (curdle_whisk_is_valid_tracker_proof_batch_ex); None is the plain call."""
    k = len(trackers)
    if len(k_commitments) != k or len(proofs) != k:
        raise ValueError("trackers, k commitments and proofs need the same count")
    if (any(len(t) != 96 for t in trackers) or any(len(c) != 48 for c in k_commitments)
            or any(len(p) != WHISK_TRACKER_PROOF_SIZE for p in proofs)):
        raise ValueError("tracker 96 B, k commitment 48 B, tracker proof 128 B")
    out = np.zeros(k, dtype=np.int32)
    if k == 0:
        return out
    t, kc, pb = _bytes_arr(b"".join(trackers)), _bytes_arr(b"".join(k_commitments)), _bytes_arr(b"".join(proofs))
    if flags is None:
        _check(_whisk_valid_tracker_batch(_ptr(t), _ptr(kc), _ptr(pb), k, _ptr(out)))
    else:
        _check(_whisk_valid_tracker_batch_ex(_ptr(t), _ptr(kc), _ptr(pb), k, flags, _ptr(out)))
    return out


def whisk_is_valid_tracker_proof_batch_device(d_trackers: int, d_k_commitments: int, d_proofs: int, k: int,
                                              stream: int = 0) -> np.ndarray:
    """The same over resident arrays (curdle_whisk_is_valid_tracker_proof_batch_device): HIP device pointers to
    k x 96, k x 48 and k x 128 bytes; stream: a hipStream_t or 0.  Transcripts are hashed on the device."""
    out = np.zeros(k, dtype=np.int32)
    _check(_whisk_valid_tracker_batch_device(d_trackers, d_k_commitments, d_proofs, k, _ptr(out) if k else None,
                                             stream or None))
    return out


def stat_tracker() -> dict:
    """Members of tracker batches hashed on the device, on the host, and handed back to the host."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_tracker(out))
    return {"device": out[0], "host": out[1], "handed_back": out[2]}


def _tracker_members(trackers, k_commitments, proofs, seed):
    k = len(trackers)
    if len(k_commitments) != k or len(proofs) != k:
        raise ValueError("trackers, k commitments and proofs need the same count")
    if (any(len(t) != 96 for t in trackers) or any(len(c) != 48 for c in k_commitments)
            or any(len(p) != WHISK_TRACKER_PROOF_SIZE for p in proofs)):
        raise ValueError("tracker 96 B, k commitment 48 B, tracker proof 128 B")
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    return k


def whisk_is_valid_tracker_proof_batch_combined(trackers, k_commitments, proofs, seed: bytes) -> np.ndarray:
    """The tracker batch settled per pass by one randomly weighted MSM
    (curdle_whisk_is_valid_tracker_proof_batch_combined).  seed: 32 bytes, unpredictable to whoever made the proofs
    and fresh per call (os.urandom(32)).  Returns int32[k] as whisk_is_valid_tracker_proof_batch does."""
    k = _tracker_members(trackers, k_commitments, proofs, seed)
    out = np.zeros(k, dtype=np.int32)
    if k == 0:
        return out
    t, kc, pb = _bytes_arr(b"".join(trackers)), _bytes_arr(b"".join(k_commitments)), _bytes_arr(b"".join(proofs))
    sd = _bytes_arr(seed)
    _check(_whisk_valid_tracker_batch_combined(_ptr(t), _ptr(kc), _ptr(pb), k, _ptr(sd), _ptr(out)))
    return out


def whisk_is_valid_tracker_proof_batch_combined_device(d_trackers: int, d_k_commitments: int, d_proofs: int, k: int,
                                                       seed: bytes, stream: int = 0) -> np.ndarray:
    """The same over resident arrays (curdle_whisk_is_valid_tracker_proof_batch_combined_device); the seed is host
    memory."""
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes")
    out = np.zeros(k, dtype=np.int32)
    sd = _bytes_arr(seed)
    _check(_whisk_valid_tracker_batch_combined_device(d_trackers or None, d_k_commitments or None, d_proofs or None, k,
                                                      _ptr(sd), _ptr(out) if k else None, stream or None))
    return out


def stat_tracker_combined() -> dict:
    """Combined tracker batches: passes settled by the sum, passes that fell back to the chains, members accepted by a
    sum, members excluded from one."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_tracker_combined(out))
    return {"settled": out[0], "fell_back": out[1], "accepted": out[2], "excluded": out[3]}


def tracker_combined_last_kernel_ms() -> float:
    """k_tracker_combine in the last whisk_tracker_combined_scalars, by HIP events."""
    out = C.c_double()
    _check(_tracker_combined_last_kernel_ms(C.byref(out)))
    return out.value


def whisk_tracker_combined_scalars(trackers, k_commitments, proofs, seed: bytes):
    """Diagnostic (curdle_whisk_tracker_combined_scalars): the MSM scalars of the combined form for at most one pass,
    (uint64[k, 5, 4], uint64[4]): Montgomery fr limbs per record, and the generator's total."""
    k = _tracker_members(trackers, k_commitments, proofs, seed)
    scalars = np.zeros((k, 5, 4), dtype=np.uint64)
    g = np.zeros(4, dtype=np.uint64)
    if k == 0:
        return scalars, g
    t, kc, pb = _bytes_arr(b"".join(trackers)), _bytes_arr(b"".join(k_commitments)), _bytes_arr(b"".join(proofs))
    sd = _bytes_arr(seed)
    _check(_whisk_tracker_combined_scalars(_ptr(t), _ptr(kc), _ptr(pb), k, _ptr(sd), _ptr(scalars), _ptr(g)))
    return scalars, g


def whisk_generate_tracker_proof(tracker: bytes, k, rand: Rand) -> bytes:
    """GenerateWhiskTrackerProof (whisk.go:149); k = Montgomery fr limbs."""
    t, kk = _bytes_arr(tracker), _as_u64(k)
    out = np.zeros(WHISK_TRACKER_PROOF_SIZE, dtype=np.uint8)
    _check(_whisk_gen_tracker(_ptr(t), _ptr(kk), rand._h, _ptr(out)))
    return out.tobytes()


TRACKER_PROVE_CONSTANT_TIME = 1                       # CURDLE_TRACKER_PROVE_CONSTANT_TIME


def whisk_generate_tracker_proof_batch(trackers, ks, rand: "Rand" = None, blinders=None, flags=None):
    """k tracker proofs at once on the GPU (curdle_whisk_generate_tracker_proof_batch / _blinders): a list of 96-byte
    trackers and ks (k, 4), Montgomery fr limbs.  Exactly one of rand (the blinders are drawn as k single calls on it
    would draw them) and blinders (k, 4) is given.  Returns (proofs uint8[k, 128], results int32[k]): results[i] is OK,
    or EINVAL with a zero proof where whisk_generate_tracker_proof raises CurdleError with EINVAL.  flags: None calls
    the entry point without flags; an integer (0, TRACKER_PROVE_CONSTANT_TIME) calls the _ex one with it."""
    if (rand is None) == (blinders is None):
        raise ValueError("give either rand or blinders")
    k = len(trackers)
    if any(len(t) != 96 for t in trackers):
        raise ValueError("tracker 96 B")
    kk = _as_u64(ks, 4).reshape(-1, 4)
    if kk.shape[0] != k:
        raise ValueError("trackers and ks need the same count")
    proofs = np.zeros((k, WHISK_TRACKER_PROOF_SIZE), dtype=np.uint8)
    results = np.zeros(k, dtype=np.int32)
    if k == 0 and flags is None:
        return proofs, results
    t = _bytes_arr(b"".join(trackers)) if k else None
    ptrs = (_ptr(t) if k else None, _ptr(kk) if k else None)
    outs = (_ptr(proofs) if k else None, _ptr(results) if k else None)
    if blinders is not None:
        bb = _as_u64(blinders, 4).reshape(-1, 4)
        if bb.shape[0] != k:
            raise ValueError("trackers and blinders need the same count")
        if flags is None:
            _check(_whisk_gen_tracker_batch_blinders(*ptrs, _ptr(bb), k, *outs))
        else:
            _check(_whisk_gen_tracker_batch_blinders_ex(*ptrs, _ptr(bb) if k else None, k, int(flags), *outs))
    elif flags is None:
        _check(_whisk_gen_tracker_batch(*ptrs, rand._h, k, *outs))
    else:
        _check(_whisk_gen_tracker_batch_ex(*ptrs, rand._h, k, int(flags), *outs))
    return proofs, results


def stat_tracker_prove() -> dict:
    """Members of generated tracker-proof batches: generated on the device, handed to the host single path."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_tracker_prove(out))
    return {"device": out[0], "host": out[1]}


TRACKER_NOT_OWNED, TRACKER_OWNED, TRACKER_BAD, TRACKER_UNKNOWN = 0, 1, 2, 255
TRACKER_OWN_CONSTANT_TIME = 1                         # CURDLE_TRACKER_OWN_CONSTANT_TIME


def whisk_is_own_tracker(tracker: bytes, k) -> bool:
    """Does k (Montgomery fr limbs) own the 96-byte tracker rG || krG: k rG == krG, infinity included
    (curdle_whisk_is_own_tracker; host only).  CurdleError with EINVAL if a record does not decode."""
    if len(tracker) != 96:
        raise ValueError("tracker 96 B")
    t, kk = _bytes_arr(tracker), _as_u64(k, 4)
    owned = C.c_int(0)
    _check(_whisk_is_own_tracker(_ptr(t), _ptr(kk), C.byref(owned)))
    return bool(owned.value)


def whisk_find_own_trackers(trackers, ks, flags=None) -> np.ndarray:
    """m keys against n trackers on the GPU (curdle_whisk_find_own_trackers): a list of 96-byte trackers (or a uint8
    array of n x 96 bytes) and ks (m, 4), Montgomery fr limbs.  Returns uint8[m, n]: TRACKER_OWNED, TRACKER_NOT_OWNED,
    or TRACKER_BAD in the whole column of a tracker with a record that does not decode.  flags: None calls the entry
    point without flags; an integer (0, TRACKER_OWN_CONSTANT_TIME) calls curdle_whisk_find_own_trackers_ex with it."""
    if isinstance(trackers, np.ndarray):
        t = np.ascontiguousarray(trackers, dtype=np.uint8).reshape(-1)
        if t.size % 96:
            raise ValueError("tracker 96 B")
    else:
        if any(len(x) != 96 for x in trackers):
            raise ValueError("tracker 96 B")
        t = _bytes_arr(b"".join(trackers))
    kk = _as_u64(ks, 4).reshape(-1, 4)
    n, m = t.size // 96, len(kk)
    owned = np.full((m, n), TRACKER_UNKNOWN, dtype=np.uint8)
    args = (_ptr(t) if n else None, n, _ptr(kk) if m else None, m, _ptr(owned) if m * n else None)
    _check(_whisk_find_own(*args) if flags is None else _whisk_find_own_ex(*args, flags))
    return owned


def whisk_find_own_trackers_device(d_trackers: int, n: int, d_ks: int, m: int, d_owned: int, stream=None, flags=None) -> None:
    """The same over resident arrays (curdle_whisk_find_own_trackers_device): HIP device pointers to n x 96 bytes,
    m x 32 bytes (both multiples of 16) and m x n bytes; stream: a hipStream_t or None.  d_owned is complete when the
    call returns.  flags: as in whisk_find_own_trackers (curdle_whisk_find_own_trackers_device_ex)."""
    args = (d_trackers or None, n, d_ks or None, m, d_owned or None, stream or None)
    _check(_whisk_find_own_device(*args) if flags is None else _whisk_find_own_device_ex(*args, flags))


def stat_tracker_own() -> dict:
    """(key, tracker) pairs answered on the device, launches of the ownership kernel, pairs answered TRACKER_BAD."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_tracker_own(out))
    return {"pairs": int(out[0]), "launches": int(out[1]), "bad": int(out[2])}


def stat_tracker_own_ct() -> dict:
    """stat_tracker_own's counters for the passes under TRACKER_OWN_CONSTANT_TIME (k_tracker_own_ct)."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_tracker_own_ct(out))
    return {"pairs": int(out[0]), "launches": int(out[1]), "bad": int(out[2])}


G1_OUT_AFFINE, G1_OUT_COMPRESSED = 0, 1
FBASE_CONSTANT_TIME = 1                               # CURDLE_FBASE_CONSTANT_TIME


class FBase:
    """One G1 point's table of 8,160 multiples on the device (curdle_fbase): point is a gnark G1Affine, 12 Montgomery
    limbs, on the curve, in the subgroup and not infinity (CurdleError with EINVAL otherwise)."""

    def __init__(self, point):
        p = _as_u64(point, 12).reshape(12)
        h = _vp()
        _check(_fbase_create(_ptr(p), C.byref(h)))
        self._h = h

    def free(self) -> None:
        if self._h:
            _fbase_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def fbase_create(point) -> FBase:
    return FBase(point)


def _fbase_handle(base):
    if base is None:
        return None                                   # the generator's table
    if not base._h:
        raise ValueError("the FBase was freed")
    return base._h


def g1_fixed_base_mul_batch(scalars, multipliers=None, base=None, out_form=G1_OUT_AFFINE, flags=None) -> np.ndarray:
    """out[i] = (scalars[i] * multipliers[i] mod r) * P on the GPU (curdle_g1_fixed_base_mul_batch): scalars and
    multipliers (n, 4) Montgomery fr limbs, multipliers may be None; base an FBase or None for the generator.  Returns
    (n, 12) uint64 affine records or (n, 48) uint8 compressed encodings.  flags: None calls the entry point without
    flags; an integer (0, FBASE_CONSTANT_TIME) calls curdle_g1_fixed_base_mul_batch_ex with it."""
    sc = _as_u64(scalars, 4).reshape(-1, 4)
    n = len(sc)
    mu = _as_u64(multipliers, 4).reshape(-1, 4) if multipliers is not None else None
    if mu is not None and len(mu) != n:
        raise ValueError("one multiplier per scalar")
    out = np.zeros((n, 48), dtype=np.uint8) if out_form == G1_OUT_COMPRESSED else np.zeros((n, 12), dtype=np.uint64)
    args = (_fbase_handle(base), _ptr(sc) if n else None, _ptr(mu) if mu is not None and n else None, n, int(out_form))
    if flags is None:
        _check(_fbase_mul(*args, _ptr(out) if n else None))
    else:
        _check(_fbase_mul_ex(*args, int(flags), _ptr(out) if n else None))
    return out


def g1_fixed_base_mul_batch_device(d_scalars: int, d_multipliers: int, n: int, d_out: int, base=None,
                                   out_form=G1_OUT_AFFINE, stream=None, flags=None) -> None:
    """The same over resident arrays (curdle_g1_fixed_base_mul_batch_device): HIP device pointers, multiples of 16
    except a compressed d_out; d_multipliers may be 0.  d_out is complete when the call returns and must not overlap
    the inputs.  flags: as in g1_fixed_base_mul_batch (curdle_g1_fixed_base_mul_batch_device_ex)."""
    args = (_fbase_handle(base), d_scalars or None, d_multipliers or None, n, int(out_form))
    if flags is None:
        _check(_fbase_mul_device(*args, d_out or None, stream or None))
    else:
        _check(_fbase_mul_device_ex(*args, int(flags), d_out or None, stream or None))


def stat_fbase() -> dict:
    """Scalars multiplied by the fixed-base kernel, its launches, and tables built since the library was loaded."""
    out = (C.c_ulonglong * 3)()
    _check(_stat_fbase(out))
    return {"scalars": int(out[0]), "launches": int(out[1]), "tables": int(out[2])}


def stat_fbase_ct() -> dict:
    """Scalars multiplied by the constant-time fixed-base kernel and its launches since the library was loaded."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_fbase_ct(out))
    return {"scalars": int(out[0]), "launches": int(out[1])}


def whisk_compute_tracker(k, r) -> bytes:
    """computeTracker (whisk_test.go:98-104) on the host: the 96 bytes r G | k r G for Montgomery fr limbs k, r."""
    kk, rr = _as_u64(k, 4).reshape(4), _as_u64(r, 4).reshape(4)
    out = np.zeros(96, dtype=np.uint8)
    _check(_whisk_compute_tracker(_ptr(kk), _ptr(rr), _ptr(out)))
    return bytes(out)


def whisk_k_commitment(k) -> bytes:
    """getKComm (whisk_test.go:106-109) on the host: the 48 bytes of k G."""
    kk = _as_u64(k, 4).reshape(4)
    out = np.zeros(48, dtype=np.uint8)
    _check(_whisk_k_commitment(_ptr(kk), _ptr(out)))
    return bytes(out)


def whisk_compute_trackers_batch(ks, rs=None, commitments=True, flags=None):
    """n trackers and key commitments on the GPU (curdle_whisk_compute_trackers_batch): ks, rs (n, 4) Montgomery fr
    limbs; rs None means r = 1.  Returns (trackers uint8[n, 96], commitments uint8[n, 48] or None).  flags: None calls
    the entry point without flags; an integer (0, FBASE_CONSTANT_TIME) calls curdle_whisk_compute_trackers_batch_ex."""
    kk = _as_u64(ks, 4).reshape(-1, 4)
    n = len(kk)
    rr = _as_u64(rs, 4).reshape(-1, 4) if rs is not None else None
    if rr is not None and len(rr) != n:
        raise ValueError("one r per k")
    trackers = np.zeros((n, 96), dtype=np.uint8)
    comms = np.zeros((n, 48), dtype=np.uint8) if commitments else None
    outs = (_ptr(trackers) if n else None, _ptr(comms) if comms is not None and n else None)
    if flags is None:
        _check(_whisk_compute_trackers_batch(_ptr(kk) if n else None, _ptr(rr) if rr is not None and n else None, n, *outs))
    else:
        _check(_whisk_compute_trackers_batch_ex(_ptr(kk) if n else None, _ptr(rr) if rr is not None and n else None, n,
                                                int(flags), *outs))
    return trackers, comms


_set_dev_acc = _sig("curdle_verify_set_device_acc", C.c_int, C.c_int)
_export_acc = _sig("curdle_verify_export_accumulator", C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, C.c_int,
                   _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int))


def verify_set_device_acc(on: bool) -> bool:
    """Keep curdleproof.Verify's accumulator on the device (default) or on the host mirror;
    returns the previous setting."""
    return bool(_set_dev_acc(1 if on else 0))


def verify_export_accumulator(crs: "CRS", proof: "Proof", Rs, Ss, Ts, Us, M, rand: "Rand", device: bool):
    """(points[n, 12], scalars[n, 4], accept) accumulated by one verification before its final
    MSM, from the host mirror (device=False) or the device accumulator (device=True)."""
    Rs, Ss, Ts, Us = (_as_u64(a, 12) for a in (Rs, Ss, Ts, Us))
    M = _as_u64(M)
    cap = 6 * crs.ell + 8192
    pts = np.zeros((cap, 12), dtype=np.uint64)
    sc = np.zeros((cap, 4), dtype=np.uint64)
    n, ok = C.c_size_t(0), C.c_int(0)
    _check(_export_acc(crs._h, proof._h, _ptr(Rs), _ptr(Ss), _ptr(Ts), _ptr(Us), crs.ell, _ptr(M), rand._h,
                       1 if device else 0, _ptr(pts), _ptr(sc), cap, C.byref(n), C.byref(ok)))
    return pts[: n.value].copy(), sc[: n.value].copy(), bool(ok.value)


def verify_set_eager(eager: bool) -> bool:
    """Evaluate the verifier's check points eagerly (the reference's order of operations)
    instead of deferring them into the accumulator's one MSM; returns the previous mode."""
    return bool(_verify_set_eager(1 if eager else 0))


def proof_reencode(proof: bytes) -> bytes:
    pb = np.frombuffer(proof, dtype=np.uint8).copy()
    out = np.zeros(len(pb) + 64, dtype=np.uint8)
    n = C.c_size_t(0)
    _check(_reencode(_ptr(pb), len(pb), _ptr(out), len(out), C.byref(n)))
    return bytes(out[: n.value])


_fr_ip = _sig("curdle_fr_inner_product", C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp)


def fr_inner_product(a, b) -> np.ndarray:
    """common.IPA (reference common/util.go:26): Montgomery-form Fr vectors in, Montgomery Fr out."""
    a = _as_u64(a, 4)
    b = _as_u64(b, 4)
    out = np.zeros(4, dtype=np.uint64)
    _check(_fr_ip(_ptr(a), len(a), _ptr(b), len(b), _ptr(out)))
    return out


def merlin_test_vector(protocol: bytes, label: bytes, msg: bytes, challenge_label: bytes, n: int) -> bytes:
    m = np.frombuffer(msg, dtype=np.uint8).copy()
    out = np.zeros(n, dtype=np.uint8)
    _check(_merlin_tv(protocol, label, _ptr(m), len(m), challenge_label, _ptr(out), n))
    return bytes(out)


_decompress_batch = _sig("curdle_g1_decompress_batch", C.c_int, _vp, C.c_size_t, C.c_int, _vp, _vp)
DECODE_OK, DECODE_INFINITY, DECODE_BAD_ENCODING, DECODE_NOT_ON_CURVE, DECODE_NOT_IN_SUBGROUP = range(5)


_decompress_begin = _sig("curdle_g1_decompress_begin", C.c_int, _vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_int))
_decompress_finish = _sig("curdle_g1_decompress_finish", C.c_int, C.c_int, _vp)


def g1_decompress_begin(data: bytes):
    """Two-step decode: returns (points, preliminary status, ticket); the subgroup test keeps
    running on the GPU until g1_decompress_finish(ticket, n) returns the final status bytes."""
    b = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    n = len(b) // 48
    out = np.zeros((n, 12), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    t = C.c_int(-1)
    _check(_decompress_begin(_ptr(b), n, _ptr(out), _ptr(st), C.byref(t)))
    return out, st, t.value


_decompress_start = _sig("curdle_g1_decompress_start", C.c_int, _vp, C.c_size_t, C.POINTER(C.c_int))
_decompress_points = _sig("curdle_g1_decompress_points", C.c_int, C.c_int, _vp, _vp)


def g1_decompress_start(data: bytes) -> int:
    """Three-step decode, step one: launches the decoding and returns a ticket at once."""
    b = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    t = C.c_int(-1)
    _check(_decompress_start(_ptr(b), len(b) // 48, C.byref(t)))
    return t.value


def g1_decompress_points(ticket: int, n: int):
    """Step two: (points, preliminary status) of the ticket's n records; g1_decompress_finish is step three."""
    out = np.zeros((n, 12), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _check(_decompress_points(ticket, _ptr(out), _ptr(st)))
    return out, st


def g1_decompress_finish(ticket: int, n: int) -> np.ndarray:
    st = np.zeros(n, dtype=np.uint8)
    _check(_decompress_finish(ticket, _ptr(st)))
    return st


def g1_decompress_batch(data: bytes, subgroup_check: bool = True):
    """n x 48 bytes of compressed points -> ((n, 12) gnark affine points, (n,) status bytes), on the GPU."""
    b = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    if len(b) % 48:
        raise ValueError("compressed G1 points are 48 bytes each")
    n = len(b) // 48
    out = np.zeros((n, 12), dtype=np.uint64)
    st = np.zeros(n, dtype=np.uint8)
    _check(_decompress_batch(_ptr(b), n, 1 if subgroup_check else 0, _ptr(out), _ptr(st)))
    return out, st


_check_batch = _sig("curdle_g1_check_batch", C.c_int, _vp, C.c_size_t, C.c_int, _vp)
_check_batch_device = _sig("curdle_g1_check_batch_device", C.c_int, _vp, C.c_size_t, C.c_int, _vp, _vp)


def g1_check_batch(points, subgroup_check: bool = True) -> np.ndarray:
    """(n, 12) gnark affine points in memory -> (n,) DECODE_* status bytes, on the GPU: infinity, a coordinate >= p,
    off the curve y^2 = x^3 + 4, and with subgroup_check outside the prime-order subgroup."""
    points = _as_u64(points, 12)
    n = points.shape[0] if points.size else 0
    st = np.zeros(n, dtype=np.uint8)
    _check(_check_batch(_ptr(points), n, 1 if subgroup_check else 0, _ptr(st)))
    return st


def g1_check_batch_device(ptr: int, n: int, subgroup_check: bool = True, stream=None) -> np.ndarray:
    """The same for n points resident in device memory at `ptr`; the status bytes come back to host memory."""
    st = np.zeros(n, dtype=np.uint8)
    _check(_check_batch_device(ptr, n, 1 if subgroup_check else 0, _ptr(st), stream or None))
    return st


_check_jac_batch = _sig("curdle_g1_check_jac_batch", C.c_int, _vp, C.c_size_t, C.c_int, _vp)
_check_jac_batch_device = _sig("curdle_g1_check_jac_batch_device", C.c_int, _vp, C.c_size_t, C.c_int, _vp, _vp)


def g1_check_jac_batch(jac_points, subgroup_check: bool = True) -> np.ndarray:
    """(n, 18) gnark G1Jac points in memory -> (n,) DECODE_* status bytes, on the GPU: Z = 0 is infinity, then a
    coordinate >= p, off the curve Y^2 = X^3 + 4 Z^6, and with subgroup_check outside the prime-order subgroup."""
    jac_points = _as_u64(jac_points, 18)
    n = jac_points.shape[0] if jac_points.size else 0
    st = np.zeros(n, dtype=np.uint8)
    _check(_check_jac_batch(_ptr(jac_points), n, 1 if subgroup_check else 0, _ptr(st)))
    return st


def g1_check_jac_batch_device(ptr: int, n: int, subgroup_check: bool = True, stream=None) -> np.ndarray:
    """The same for n points resident in device memory at `ptr`; the status bytes come back to host memory."""
    st = np.zeros(n, dtype=np.uint8)
    _check(_check_jac_batch_device(ptr, n, 1 if subgroup_check else 0, _ptr(st), stream or None))
    return st


_scalar_mul_batch = _sig("curdle_g1_scalar_mul_batch", C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp)


G1_MUL_CONSTANT_TIME = 1                              # CURDLE_G1_MUL_CONSTANT_TIME


def g1_scalar_mul_batch(points, scalars, addends=None, flags=None) -> np.ndarray:
    """out[i] = addends[i] + scalars[i] * points[i] on the GPU; scalars (n, 4) or one shared (4,).  flags: None calls
    the entry point without flags; an integer (0, G1_MUL_CONSTANT_TIME) calls curdle_g1_scalar_mul_batch_ex with it
    (the constant-time kernel takes no addends)."""
    points = _as_u64(points, 12)
    n = points.shape[0] if points.size else 0
    sc = _as_u64(scalars, 4)
    ns = (1 if sc.ndim == 1 else sc.shape[0]) if sc.size else 0
    add = _as_u64(addends, 12) if addends is not None else None
    out = np.zeros((n, 12), dtype=np.uint64)
    if flags is None:
        _check(_scalar_mul_batch(_ptr(points), _ptr(sc), ns, _ptr(add) if add is not None else None, n, _ptr(out)))
    else:
        _check(_scalar_mul_batch_ex(_ptr(points), _ptr(sc), ns, _ptr(add) if add is not None else None, n, int(flags),
                                    _ptr(out)))
    return out


def g1_compress(jac) -> bytes:
    jac = _as_u64(jac)
    out = np.zeros(48, dtype=np.uint8)
    _check(_g1_compress(_ptr(jac), _ptr(out)))
    return bytes(out)


def g1_compress_batch(jac_points) -> np.ndarray:
    """(n, 18) gnark G1Jac points -> (n, 48) bytes of gnark's compressed encoding, on the GPU
    (curdle_g1_compress_batch): row i is g1_compress(jac_points[i])."""
    jac_points = _as_u64(jac_points, 18)
    n = jac_points.shape[0] if jac_points.size else 0
    out = np.zeros((n, 48), dtype=np.uint8)
    _check(_g1_compress_batch(_ptr(jac_points), n, _ptr(out)))
    return out


def g1_compress_batch_device(ptr: int, n: int, out_ptr: int, stream=None) -> None:
    """The same for n points resident in device memory at `ptr` (any alignment); the n x 48 bytes are written to
    device memory at `out_ptr` in the stream's order and are complete when the call returns."""
    _check(_g1_compress_batch_device(ptr or None, n, out_ptr or None, stream or None))


def g1_normalize_batch(points, form=None) -> np.ndarray:
    """(n, 18) gnark G1Jac or (n, 24) XYZZ points -> (n, 12) gnark affine points on the GPU with a shared inversion
    (curdle_g1_normalize_batch; gnark's BatchJacobianToAffineG1).  form: G1_FORM_JAC / G1_FORM_XYZZ, or None to take
    it from the row length.  A denominator that is 0 mod p gives (0, 0)."""
    points = np.ascontiguousarray(points, dtype=np.uint64)
    if form is None:
        form = {18: G1_FORM_JAC, 24: G1_FORM_XYZZ}[points.shape[-1]]
    n = points.shape[0] if points.size else 0
    out = np.zeros((n, 12), dtype=np.uint64)
    _check(_g1_normalize_batch(_ptr(points), int(form), n, _ptr(out)))
    return out


def g1_normalize_batch_device(ptr: int, form: int, n: int, out_ptr: int, stream=None) -> None:
    """The same for n points resident in device memory at `ptr`; the n x 96 bytes are written to device memory at
    `out_ptr` in the stream's order and are complete when the call returns.  Both pointers are multiples of 16."""
    _check(_g1_normalize_batch_device(ptr or None, int(form), n, out_ptr or None, stream or None))


def g1_scalar_mul_batch_device(d_points: int, d_scalars: int, n_scalars: int, d_addends: int, n: int, d_out: int,
                               stream=None, flags=None) -> None:
    """g1_scalar_mul_batch with everything resident (curdle_g1_scalar_mul_batch_device): d_out[i] = d_addends[i] +
    d_scalars[i or 0] * d_points[i] as gnark affine records; d_addends may be 0, d_out may be d_points or d_addends.
    flags: as in g1_scalar_mul_batch (curdle_g1_scalar_mul_batch_device_ex; with G1_MUL_CONSTANT_TIME d_addends is 0)."""
    if flags is None:
        _check(_scalar_mul_batch_device(d_points or None, d_scalars or None, n_scalars, d_addends or None, n, d_out or None,
                                        stream or None))
    else:
        _check(_scalar_mul_batch_device_ex(d_points or None, d_scalars or None, n_scalars, d_addends or None, n, int(flags),
                                           d_out or None, stream or None))


def stat_g1_mul_ct() -> dict:
    """Scalars multiplied by the constant-time variable-base kernel and its launches since the library was loaded."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_g1_mul_ct(out))
    return {"scalars": int(out[0]), "launches": int(out[1])}


_fp_invert_batch = _sig("curdle_fp_invert_batch", C.c_int, _vp, C.c_size_t, _vp, C.c_uint)
_fp_invert_batch_device = _sig("curdle_fp_invert_batch_device", C.c_int, _vp, C.c_size_t, _vp, C.c_uint, _vp)
_stat_fp_invert = _sig("curdle_stat_fp_invert", C.c_int, C.POINTER(C.c_ulonglong))

FP_INVERT_FERMAT = 1                                  # CURDLE_FP_INVERT_FERMAT
FP_INVERT_RAW28 = 2                                   # CURDLE_FP_INVERT_RAW28


def fp_invert_batch(elements, flags: int = 0, out=None) -> np.ndarray:
    """out[i] = elements[i]^-1 in Fp on the GPU, 0 -> 0, constant time in the elements (curdle_fp_invert_batch).
    elements: (n, 6) uint64 gnark fp.Elements (Montgomery, canonical), or under FP_INVERT_RAW28 (n, 7) uint64 holding
    the 14 uint32 limbs of the internal field layer.  flags: 0 inverts by division steps, FP_INVERT_FERMAT by the
    exponent chain (bit-identical).  out: an array to write into (it may be `elements`); a new one by default.  An
    element out of range raises CurdleError(EINVAL) and leaves `out` untouched."""
    cols = 7 if int(flags) & FP_INVERT_RAW28 else 6
    elements = _as_u64(elements, cols)
    n = elements.shape[0] if elements.size else 0
    if out is None:
        out = np.zeros((n, cols), dtype=np.uint64)
    _check(_fp_invert_batch(_ptr(elements), n, _ptr(out), int(flags)))
    return out


def fp_invert_batch_device(d_in: int, n: int, d_out: int, flags: int = 0, stream=None) -> None:
    """The same for n elements resident in device memory at d_in (curdle_fp_invert_batch_device): the inverses are
    written to d_out (which may be d_in) in the stream's order and are complete when the call returns.  Both pointers
    are multiples of 16.  After CurdleError(EINVAL) for an element out of range d_out's contents are unspecified."""
    _check(_fp_invert_batch_device(d_in or None, n, d_out or None, int(flags), stream or None))


def stat_fp_invert() -> dict:
    """Completed calls of fp_invert_batch / _device and their elements, and the finish launches of the constant-time
    MSM by the inversion their exit took (division steps under knob CT_FINISH_DIVSTEPS, or the Fermat chain), since
    the library was loaded."""
    out = (C.c_ulonglong * 4)()
    _check(_stat_fp_invert(out))
    return {"calls": int(out[0]), "elements": int(out[1]), "finish_divsteps": int(out[2]), "finish_fermat": int(out[3])}


def stat_normalize() -> dict:
    """Points normalised on the device and inversion groups run since the library was loaded."""
    out = (C.c_ulonglong * 2)()
    _check(_stat_normalize(out))
    return {"points": int(out[0]), "groups": int(out[1])}


def g1_decompress(data: bytes, subgroup_check: bool = True) -> np.ndarray:
    b = np.frombuffer(data, dtype=np.uint8).copy()
    out = np.zeros(18, dtype=np.uint64)
    _check(_g1_decompress(_ptr(b), 1 if subgroup_check else 0, _ptr(out)))
    return out
