"""ctypes binding of libplaysnark_hip.so.  Fails loudly: no library => ImportError, there is
no Python/CPU implementation behind these calls."""
from __future__ import annotations

import ctypes as C
import os

from .build import library_path

PS_OK = 0
PS_ERR_LENGTH = -1
PS_ERR_NOT_DIVISIBLE = -2
PS_ERR_ENCODING = -3
PS_ERR_HIP = -4
PS_ERR_ARG = -5
PS_ERR_NO_DEVICE = -6
PS_FMT_AFFINE, PS_FMT_COMPRESSED = 0, 1
PS_G1, PS_G2 = 1, 2

# every symbol include/playsnark_hip.h declares (tests/test_abi.py checks the header against this)
SYMBOLS = [
    "ps_abi_version", "ps_last_error", "ps_version", "ps_device_count",
    "ps_ctx_create", "ps_ctx_destroy", "ps_ctx_sync", "ps_ctx_stream", "ps_ctx_set_tables", "ps_ctx_set_table_budget",
    "ps_points_upload", "ps_points_from_scalars", "ps_points_download", "ps_points_download_fmt", "ps_points_len", "ps_points_group",
    "ps_points_slice", "ps_points_free", "ps_points_check_subgroup", "ps_points_precompute", "ps_points_table_window",
    "ps_scalars_upload", "ps_scalars_upload_i64", "ps_scalars_from_device_be32", "ps_scalars_download",
    "ps_scalars_len", "ps_scalars_slice", "ps_scalars_free",
    "ps_msm", "ps_msm_be32", "ps_msm_i64", "ps_msm_launch", "ps_msm_finish", "ps_msm_multi", "ps_points_sum", "ps_point_convert",
    "ps_msm_last_info", "ps_msm_set_window", "ps_msm_set_slice", "ps_msm_set_tail", "ps_microbench_mad", "ps_ctx_set_timing", "ps_msm_last_stage_ms",
    "ps_qap_create", "ps_qap_free", "ps_qap_quotient", "ps_qap_is_valid", "ps_qap_interpolate", "ps_poly_mul",
    "ps_points_lincomb", "ps_msm_multi_device", "ps_groth16_prove_multi", "ps_points_monomial_to_lagrange",
    "ps_groth16_setup", "ps_phgr13_setup", "ps_phgr13_crs_free", "ps_groth16_prove", "ps_groth16_prove_shard", "ps_groth16_prove_local", "ps_phgr13_prove", "ps_phgr13_prove_shard", "ps_phgr13_prove_multi", "ps_groth16_verify", "ps_phgr13_verify", "ps_pairing_equal", "ps_prove_last_phase_ms",
    "ps_pairing_product_is_one", "ps_groth16_verify_batch", "ps_groth16_verify_batch_locate", "ps_groth16_verify_batch_locate_info",
    "ps_qap_column_sums", "ps_groth16_setup_from_srs", "ps_groth16_crs_contribute", "ps_groth16_crs_check_update",
    "ps_scalars_powers", "ps_groth16_srs_contribute", "ps_groth16_srs_check", "ps_groth16_srs_check_update",
    "ps_points_lagrange_check", "ps_groth16_crs_check_from_srs",
    "ps_qap_create_fr", "ps_qap_wide_entries",
    "ps_msm_batch", "ps_msm_batch_set_chunk", "ps_groth16_prove_batch",
    "ps_msm_batch_multi", "ps_phgr13_prove_batch",
    "ps_msm_set_accumulate", "ps_msm_last_accumulate",
    "ps_msm_batch_set_table",
    "ps_phgr13_verify_batch", "ps_phgr13_verify_batch_info",
    "ps_msm_prediction_counts",
    "ps_phgr13_verify_batch_locate", "ps_phgr13_verify_batch_locate_info",
    "ps_poly_scan_tile", "ps_poly_eval", "ps_poly_div_linear", "ps_kzg_commit", "ps_kzg_open", "ps_kzg_verify", "ps_kzg_verify_batch",
    "ps_scalars_lincomb", "ps_kzg_open_multi", "ps_kzg_verify_multi",
    "ps_poly_scan_set_group", "ps_poly_div_roots", "ps_kzg_open_set", "ps_kzg_verify_set",
    "ps_poly_lagrange_tile", "ps_qap_gate_values", "ps_poly_eval_lagrange", "ps_poly_div_linear_lagrange", "ps_kzg_commit_lagrange",
    "ps_kzg_open_lagrange",
    "ps_poly_lagrange_set_group", "ps_poly_div_roots_lagrange", "ps_kzg_open_set_lagrange",
    "ps_kzg_all_key_lagrange", "ps_kzg_open_all_lagrange",
]


PS_MSM_QUEUE = 4  # pending sums per context (include/playsnark_hip.h)


class MsmInfo(C.Structure):
    _fields_ = [("window_bits", C.c_int), ("windows", C.c_int), ("entries", C.c_uint64),
                ("buckets", C.c_uint64), ("slice", C.c_int), ("window_table", C.c_int)]


class VerifyLocateInfo(C.Structure):  # ps_verify_locate_info
    _fields_ = [("checks", C.c_uint32), ("levels", C.c_uint32), ("invalid", C.c_uint32), ("reserved", C.c_uint32)]


class Phgr13BatchInfo(C.Structure):  # ps_phgr13_batch_info
    _fields_ = [("failed", C.c_uint32), ("device_loops", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Phgr13LocateInfo(C.Structure):  # ps_phgr13_locate_info
    _fields_ = [("checks", C.c_uint32), ("products", C.c_uint32), ("levels", C.c_uint32), ("invalid", C.c_uint32), ("failed", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class Csr(C.Structure):
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p)]


class CsrFr(C.Structure):  # ps_csr_fr: val_be32 = nnz x 32 B, canonical big-endian Fr elements
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("val_be32", C.c_void_p)]


class Groth16Pk(C.Structure):
    _fields_ = [("alpha", C.c_uint8 * 96), ("beta", C.c_uint8 * 96), ("delta", C.c_uint8 * 96),
                ("beta2", C.c_uint8 * 192), ("delta2", C.c_uint8 * 192),
                ("xi", C.c_void_p), ("xi2", C.c_void_p), ("nio_lp", C.c_void_p), ("xi_t", C.c_void_p),
                ("lxi", C.c_void_p), ("lxi2", C.c_void_p), ("lxi_t", C.c_void_p)]  # the Lagrange form, NULL = absent


class Groth16Device(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("qap", C.c_void_p), ("sol", C.c_void_p), ("pk", Groth16Pk)]


class Groth16Toxic(C.Structure):
    _fields_ = [(n, C.c_uint8 * 32) for n in ("alpha", "beta", "delta", "x", "gamma")]


class Groth16Crs(C.Structure):
    _fields_ = [("alpha", C.c_uint8 * 96), ("beta", C.c_uint8 * 96), ("delta", C.c_uint8 * 96),
                ("beta2", C.c_uint8 * 192), ("delta2", C.c_uint8 * 192), ("gamma", C.c_uint8 * 192),
                ("xi", C.c_void_p), ("xi2", C.c_void_p), ("io_lp", C.c_void_p), ("nio_lp", C.c_void_p), ("xi_t", C.c_void_p),
                ("lxi", C.c_void_p), ("lxi2", C.c_void_p), ("lxi_t", C.c_void_p)]


class Groth16Vk(C.Structure):
    _fields_ = [("alpha", C.c_uint8 * 96), ("beta2", C.c_uint8 * 192), ("gamma", C.c_uint8 * 192),
                ("delta2", C.c_uint8 * 192), ("io_lp", C.c_void_p)]


class Phgr13Vk(C.Structure):
    _fields_ = [("av", C.c_uint8 * 192), ("aw", C.c_uint8 * 96), ("ay", C.c_uint8 * 192), ("gamma", C.c_uint8 * 192),
                ("bgamma", C.c_uint8 * 96), ("bgamma2", C.c_uint8 * 192), ("yts", C.c_uint8 * 192),
                ("vs_io", C.c_void_p), ("ws_io", C.c_void_p), ("ys_io", C.c_void_p)]


class Phgr13Ek(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("vs", "ws", "ys", "vas", "was", "yas", "gsi", "vbs", "wbs", "ybs", "lgsi")]


class Phgr13Device(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("qap", C.c_void_p), ("sol", C.c_void_p), ("ek", Phgr13Ek)]


class Phgr13Toxic(C.Structure):
    _fields_ = [(n, C.c_uint8 * 32) for n in ("s", "av", "aw", "ay", "rv", "rw", "beta", "gamma")]


class Phgr13Crs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("gsi", "vs", "ws", "ys", "vas", "was", "yas", "vbs", "wbs", "ybs")] +
                [("av", C.c_uint8 * 192), ("aw", C.c_uint8 * 96), ("ay", C.c_uint8 * 192), ("gamma", C.c_uint8 * 192),
                 ("bgamma", C.c_uint8 * 96), ("bgamma2", C.c_uint8 * 192), ("yts", C.c_uint8 * 192)] +
                [(n, C.c_void_p) for n in ("vk_vs", "vk_ws", "vk_ys", "lgsi")])


class Phgr13Proof(C.Structure):
    _fields_ = [("vss", C.c_uint8 * 96), ("vass", C.c_uint8 * 96), ("wss", C.c_uint8 * 192),
                ("wass", C.c_uint8 * 96), ("yss", C.c_uint8 * 96), ("yass", C.c_uint8 * 96),
                ("hs", C.c_uint8 * 96), ("gz", C.c_uint8 * 96)]


class Groth16Srs(C.Structure):  # phase-1 output (ps_groth16_srs): x^i G1 (2n-1), x^i G2 (n), alpha x^i G1 (n), beta x^i G1 (n), beta G2
    _fields_ = [("tau_g1", C.c_void_p), ("tau_g2", C.c_void_p), ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p),
                ("beta_g2", C.c_uint8 * 192)]


class Groth16SrsShare(C.Structure):  # a phase-1 contributor's public values (ps_groth16_srs_share): t G2, a G2, b G2
    _fields_ = [("t_g2", C.c_uint8 * 192), ("a_g2", C.c_uint8 * 192), ("b_g2", C.c_uint8 * 192)]


def _load():
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  playsnark_amd has no CPU fallback."
        )
    lib = C.CDLL(path)
    lib.ps_last_error.restype = C.c_char_p
    lib.ps_version.restype = C.c_char_p
    lib.ps_ctx_stream.restype = C.c_void_p
    lib.ps_points_len.restype = C.c_size_t
    lib.ps_scalars_len.restype = C.c_size_t
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    pp = C.POINTER(C.c_void_p)
    lib.ps_ctx_create.argtypes = [i, pp]
    lib.ps_ctx_destroy.argtypes = [vp]
    lib.ps_ctx_destroy.restype = None
    lib.ps_ctx_sync.argtypes = [vp]
    lib.ps_ctx_stream.argtypes = [vp]
    lib.ps_ctx_set_tables.argtypes = [vp, i]
    lib.ps_points_upload.argtypes = [vp, i, C.c_char_p, sz, i, pp]
    lib.ps_points_from_scalars.argtypes = [vp, i, vp, pp]
    lib.ps_points_download.argtypes = [vp, vp, sz, sz, C.c_char_p]
    lib.ps_points_download_fmt.argtypes = [vp, vp, sz, sz, i, C.c_char_p]
    lib.ps_points_len.argtypes = [vp]
    lib.ps_points_group.argtypes = [vp]
    lib.ps_points_slice.argtypes = [vp, sz, sz, pp]
    lib.ps_points_check_subgroup.argtypes = [vp, vp, C.POINTER(C.c_int)]
    lib.ps_points_precompute.argtypes = [vp, vp, i]
    lib.ps_points_table_window.argtypes = [vp]
    lib.ps_points_free.argtypes = [vp]
    lib.ps_points_free.restype = None
    lib.ps_scalars_upload.argtypes = [vp, C.c_char_p, sz, pp]
    lib.ps_scalars_upload_i64.argtypes = [vp, vp, sz, pp]
    lib.ps_scalars_from_device_be32.argtypes = [vp, vp, sz, pp]
    lib.ps_scalars_download.argtypes = [vp, vp, sz, sz, C.c_char_p]
    lib.ps_scalars_len.argtypes = [vp]
    lib.ps_scalars_slice.argtypes = [vp, sz, sz, pp]
    lib.ps_scalars_free.argtypes = [vp]
    lib.ps_scalars_free.restype = None
    lib.ps_msm.argtypes = [vp, vp, vp, C.c_char_p]
    lib.ps_msm_be32.argtypes = [vp, vp, C.c_char_p, sz, C.c_char_p]
    lib.ps_msm_i64.argtypes = [vp, vp, vp, sz, C.c_char_p]
    lib.ps_msm_launch.argtypes = [vp, vp, vp]
    lib.ps_msm_finish.argtypes = [vp, C.c_char_p]
    lib.ps_msm_multi.argtypes = [vp, C.POINTER(vp), C.c_size_t, vp, C.POINTER(vp)]
    lib.ps_msm_batch.argtypes = [vp, vp, vp, sz, C.c_char_p]
    lib.ps_msm_batch_set_chunk.argtypes = [vp, i]
    if hasattr(lib, "ps_msm_batch_set_table"):  # found by symbol, as ps_msm_set_accumulate below
        lib.ps_msm_batch_set_table.argtypes = [vp, i]
    lib.ps_msm_batch_multi.argtypes = [vp, C.POINTER(vp), sz, vp, sz, sz, sz, C.POINTER(vp)]
    lib.ps_points_sum.argtypes = [i, C.c_char_p, sz, C.c_char_p]
    lib.ps_point_convert.argtypes = [i, i, i, C.c_char_p, C.c_char_p]
    lib.ps_msm_last_info.argtypes = [vp, C.POINTER(MsmInfo)]
    lib.ps_msm_set_window.argtypes = [vp, i]
    lib.ps_ctx_set_timing.argtypes = [vp, i]
    lib.ps_msm_set_slice.argtypes = [vp, i]
    lib.ps_msm_set_tail.argtypes = [vp, i]
    if hasattr(lib, "ps_msm_set_accumulate"):  # found by symbol: an older build named by PLAYSNARK_HIP_LIB (A/B runs) loads without the knob
        lib.ps_msm_set_accumulate.argtypes = [vp, i]
        lib.ps_msm_last_accumulate.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(lib, "ps_msm_prediction_counts"):  # found by symbol, as above
        lib.ps_msm_prediction_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.ps_microbench_mad.argtypes = [vp, C.POINTER(C.c_double)]
    lib.ps_ctx_set_table_budget.argtypes = [vp, C.c_longlong]
    lib.ps_qap_is_valid.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    lib.ps_msm_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.ps_qap_create.argtypes = [vp, sz, sz, sz, C.POINTER(Csr), C.POINTER(Csr), C.POINTER(Csr), pp]
    lib.ps_qap_create_fr.argtypes = [vp, sz, sz, sz, C.POINTER(CsrFr), C.POINTER(CsrFr), C.POINTER(CsrFr), pp]
    lib.ps_qap_wide_entries.argtypes = [vp, C.POINTER(sz)]
    lib.ps_qap_free.argtypes = [vp]
    lib.ps_qap_free.restype = None
    lib.ps_qap_quotient.argtypes = [vp, vp, vp, pp, pp, pp, pp]
    lib.ps_poly_mul.argtypes = [vp, vp, vp, pp]
    lib.ps_qap_interpolate.argtypes = [vp, vp, vp, i, pp]
    lib.ps_points_lincomb.argtypes = [i, C.c_char_p, C.c_char_p, sz, C.c_char_p]
    lib.ps_points_monomial_to_lagrange.argtypes = [vp, vp, vp, i, C.POINTER(vp)]
    lib.ps_msm_multi_device.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), sz, C.c_char_p]
    lib.ps_groth16_prove_multi.argtypes = [C.POINTER(Groth16Device), sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.ps_groth16_prove.argtypes = [vp, C.POINTER(Groth16Pk), vp, vp, C.c_char_p, C.c_char_p, C.c_char_p,
                                     C.c_char_p, C.c_char_p]
    lib.ps_groth16_prove_batch.argtypes = [vp, C.POINTER(Groth16Pk), vp, vp, sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                           C.POINTER(C.c_int)]
    lib.ps_groth16_prove_shard.argtypes = [vp, C.POINTER(Groth16Pk), vp, vp, C.c_char_p, C.c_char_p, i, i, C.c_char_p,
                                           C.c_char_p, C.c_char_p]
    lib.ps_groth16_prove_local.argtypes = [vp, C.POINTER(Groth16Pk), vp, vp, C.c_char_p, C.c_char_p, i, i, C.c_char_p,
                                           C.c_char_p, C.c_char_p]
    lib.ps_phgr13_prove.argtypes = [vp, C.POINTER(Phgr13Ek), vp, vp, C.POINTER(Phgr13Proof)]
    lib.ps_phgr13_prove_batch.argtypes = [vp, C.POINTER(Phgr13Ek), vp, vp, sz, C.POINTER(Phgr13Proof), C.POINTER(C.c_int)]
    lib.ps_phgr13_prove_shard.argtypes = [vp, C.POINTER(Phgr13Ek), vp, vp, i, i, C.POINTER(Phgr13Proof)]
    lib.ps_phgr13_prove_multi.argtypes = [C.POINTER(Phgr13Device), sz, C.POINTER(Phgr13Proof)]
    lib.ps_groth16_setup.argtypes = [vp, vp, C.POINTER(Groth16Toxic), C.POINTER(Groth16Crs)]
    lib.ps_phgr13_setup.argtypes = [vp, vp, C.POINTER(Phgr13Toxic), C.POINTER(Phgr13Crs)]
    lib.ps_phgr13_crs_free.argtypes = [C.POINTER(Phgr13Crs)]
    lib.ps_phgr13_crs_free.restype = None
    lib.ps_prove_last_phase_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.ps_groth16_verify.argtypes = [vp, C.POINTER(Groth16Vk), vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.ps_phgr13_verify.argtypes = [vp, C.POINTER(Phgr13Vk), vp, C.POINTER(Phgr13Proof), C.POINTER(C.c_int)]
    lib.ps_pairing_equal.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.ps_pairing_product_is_one.argtypes = [vp, vp, vp, i, C.POINTER(C.c_int)]
    lib.ps_groth16_verify_batch.argtypes = [vp, C.POINTER(Groth16Vk), vp, C.c_char_p, sz, C.c_char_p, C.POINTER(C.c_int)]
    lib.ps_groth16_verify_batch_locate.argtypes = [vp, C.POINTER(Groth16Vk), vp, C.c_char_p, sz, C.c_char_p, C.c_char_p, C.POINTER(sz)]
    lib.ps_groth16_verify_batch_locate_info.argtypes = [vp, C.POINTER(VerifyLocateInfo)]
    lib.ps_phgr13_verify_batch.argtypes = [vp, C.POINTER(Phgr13Vk), vp, C.POINTER(Phgr13Proof), sz, C.c_char_p, C.POINTER(C.c_int)]
    lib.ps_phgr13_verify_batch_info.argtypes = [vp, C.POINTER(Phgr13BatchInfo)]
    if hasattr(lib, "ps_phgr13_verify_batch_locate"):  # found by symbol: an older build named by PLAYSNARK_HIP_LIB (A/B runs) loads without it
        lib.ps_phgr13_verify_batch_locate.argtypes = [vp, C.POINTER(Phgr13Vk), vp, C.POINTER(Phgr13Proof), sz, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(sz)]
        lib.ps_phgr13_verify_batch_locate_info.argtypes = [vp, C.POINTER(Phgr13LocateInfo)]
    lib.ps_qap_column_sums.argtypes = [vp, vp, i, vp, pp]
    lib.ps_groth16_setup_from_srs.argtypes = [vp, vp, C.POINTER(Groth16Srs), C.POINTER(Groth16Crs)]
    lib.ps_groth16_crs_contribute.argtypes = [vp, C.POINTER(Groth16Crs), C.c_char_p, C.c_char_p, C.POINTER(Groth16Crs)]
    lib.ps_groth16_crs_check_update.argtypes = [vp, C.POINTER(Groth16Crs), C.POINTER(Groth16Crs), C.c_char_p, sz, C.POINTER(C.c_int)]
    lib.ps_scalars_powers.argtypes = [vp, C.c_char_p, C.c_char_p, sz, pp]
    lib.ps_groth16_srs_contribute.argtypes = [vp, C.POINTER(Groth16Srs), C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(Groth16Srs),
                                              C.POINTER(Groth16SrsShare)]
    lib.ps_groth16_srs_check.argtypes = [vp, C.POINTER(Groth16Srs), C.c_char_p, sz, i, C.POINTER(C.c_int)]
    lib.ps_groth16_srs_check_update.argtypes = [vp, C.POINTER(Groth16Srs), C.POINTER(Groth16Srs), C.POINTER(Groth16SrsShare), C.c_char_p, sz,
                                                C.POINTER(C.c_int)]
    lib.ps_points_lagrange_check.argtypes = [vp, vp, vp, vp, i, C.c_char_p, sz, C.POINTER(C.c_int)]
    lib.ps_groth16_crs_check_from_srs.argtypes = [vp, vp, C.POINTER(Groth16Srs), C.POINTER(Groth16Crs), C.c_char_p, sz, i, C.POINTER(C.c_int)]
    if hasattr(lib, "ps_kzg_open"):  # found by symbol: an older build named by PLAYSNARK_HIP_LIB (A/B runs) loads without KZG
        lib.ps_poly_scan_tile.argtypes = []
        lib.ps_poly_eval.argtypes = [vp, vp, C.c_char_p, sz, C.c_char_p]
        lib.ps_poly_div_linear.argtypes = [vp, vp, C.c_char_p, sz, pp, C.c_char_p]
        lib.ps_kzg_commit.argtypes = [vp, vp, vp, C.c_char_p]
        lib.ps_kzg_open.argtypes = [vp, vp, vp, C.c_char_p, sz, C.c_char_p, C.c_char_p]
        lib.ps_kzg_verify.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
        lib.ps_kzg_verify_batch.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, i, C.POINTER(C.c_int)]
    if hasattr(lib, "ps_kzg_open_multi"):  # likewise: added after the KZG block, within revision 5
        lib.ps_scalars_lincomb.argtypes = [vp, C.POINTER(vp), sz, C.c_char_p, sz, pp]
        lib.ps_kzg_open_multi.argtypes = [vp, vp, C.POINTER(vp), sz, C.c_char_p, sz, C.c_char_p, C.c_char_p, C.c_char_p]
        lib.ps_kzg_verify_multi.argtypes = [vp, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, i,
                                            C.POINTER(C.c_int)]
    if hasattr(lib, "ps_kzg_open_set"):  # likewise: one polynomial at a set of points, within revision 5
        lib.ps_poly_scan_set_group.argtypes = []
        lib.ps_poly_div_roots.argtypes = [vp, vp, C.c_char_p, sz, pp, C.c_char_p, C.c_char_p]
        lib.ps_kzg_open_set.argtypes = [vp, vp, vp, C.c_char_p, sz, C.c_char_p, C.c_char_p]
        lib.ps_kzg_verify_set.argtypes = [vp, vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, sz, C.c_char_p, i, C.POINTER(C.c_int)]
    if hasattr(lib, "ps_kzg_open_lagrange"):  # likewise: polynomials given by their values on 1..n, within revision 5
        lib.ps_poly_lagrange_tile.argtypes = []
        lib.ps_qap_gate_values.argtypes = [vp, vp, vp, i, pp]
        lib.ps_poly_eval_lagrange.argtypes = [vp, vp, vp, C.c_char_p, sz, C.c_char_p]
        lib.ps_poly_div_linear_lagrange.argtypes = [vp, vp, vp, C.c_char_p, sz, pp, C.c_char_p]
        lib.ps_kzg_commit_lagrange.argtypes = [vp, vp, vp, C.c_char_p]
        lib.ps_kzg_open_lagrange.argtypes = [vp, vp, vp, vp, C.c_char_p, sz, C.c_char_p, C.c_char_p]
    if hasattr(lib, "ps_kzg_open_set_lagrange"):  # likewise: a set of points of a value-form polynomial, within revision 5
        lib.ps_poly_lagrange_set_group.argtypes = []
        lib.ps_poly_div_roots_lagrange.argtypes = [vp, vp, vp, C.c_char_p, sz, pp, C.c_char_p, C.c_char_p]
        lib.ps_kzg_open_set_lagrange.argtypes = [vp, vp, vp, vp, C.c_char_p, sz, C.c_char_p, C.c_char_p]
    if hasattr(lib, "ps_kzg_open_all_lagrange"):  # likewise: the proofs of every node of the domain, within revision 5
        lib.ps_kzg_all_key_lagrange.argtypes = [vp, vp, vp, pp]
        lib.ps_kzg_open_all_lagrange.argtypes = [vp, vp, vp, vp, vp, pp]
    return lib


PS_ABI_VERSION = 5  # include/playsnark_hip.h: the structs above mirror that revision

lib = _load()
if lib.ps_abi_version() != PS_ABI_VERSION:
    raise ImportError("libplaysnark_hip.so has ABI %d, this binding is written for %d" % (lib.ps_abi_version(), PS_ABI_VERSION))
