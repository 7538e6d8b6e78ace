"""ddshe — Python binding of the MI355X homomorphic-aggregation engine (C-ABI in include/ddshe.h).

The engine replaces the BigInteger fold/filter loops of the reference REST proxy
(``src/main/scala/dds/http/DDSRestServer.scala``) and hlib's ``HomoAdd`` /
``HomoMult`` primitives. This module only marshals arguments; every arithmetic
entry point runs HIP kernels inside ``libddshe.so``. There is no CPU fallback:
importing this package fails loudly if the shared library is missing, and every
call raises :class:`DDSError` on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DDSHE_LIB") or os.path.join(_HERE, "libddshe.so")  # DDSHE_LIB: A/B builds

if not os.path.exists(LIB_PATH):
    raise ImportError(f"libddshe.so not built at {LIB_PATH}: run `make -C dependable-data-storage-csd2017_amd/csrc` "
                      "or __graft_entry__.build()")
# One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 (same soname as
# /opt/rocm's). Loading torch first makes libddshe.so bind to that copy, so device pointers and
# streams are shared with torch; loading ours first would start a second runtime that torch
# then cannot initialise beside ("No HIP GPUs are available").
try:
    import torch  # noqa: F401
except ImportError:  # plain C-ABI use without PyTorch: /opt/rocm's runtime
    pass
_lib = C.CDLL(LIB_PATH)

# status codes (include/ddshe.h)
DDS_OK, DDS_E_EMPTY, DDS_E_RANGE, DDS_E_HIP, DDS_E_ARG = 0, 1, 2, 3, 4
DDS_E_NOMEM, DDS_E_UNSUPPORTED, DDS_E_BUFSIZE, DDS_E_FORMAT = 5, 6, 7, 8
OPE_OPS = {"gt": 0, "ge": 1, "lt": 2, "le": 3}
DDS_PAIR_GPU, DDS_PAIR_LONE, DDS_PAIR_HOST = 0, 1, 2  # dds_pair_set_policy

# every symbol the header declares (checked by tests/test_abi.py without a GPU)
EXPORTS = [
    "dds_ctx_create", "dds_ctx_destroy", "dds_strerror", "dds_last_error", "dds_max_modulus_bits",
    "dds_ctx_set_stream", "dds_ctx_set_timing", "dds_ctx_get_timing", "dds_ctx_reset_timing", "dds_ctx_get_fold_work",
    "dds_modmul_fold", "dds_paillier_sum", "dds_rsa_product", "dds_modmul_pairs", "dds_bigint_sum",
    "dds_bigint_product",
    "dds_col_create", "dds_col_destroy", "dds_col_append", "dds_col_append_dec", "dds_col_count", "dds_col_read", "dds_col_fold",
    "dds_col_fold_partial", "dds_col_partial_words", "dds_combine_partials", "dds_col_fill_paillier_synth",
    "dds_ope_filter", "dds_ope_filter_device", "dds_paillier_encrypt_batch", "dds_modexp_batch", "dds_sum_all_dec",
    "dds_mult_all_dec", "dds_paillier_encrypt_batch_crt", "dds_col_fill_random", "dds_col_encrypt_paillier",
    "dds_col_fill_table_synth", "dds_col_truncate",
    "dds_ope_order", "dds_ope_order_device", "dds_strtab_create", "dds_strtab_destroy", "dds_search_eq",
    "dds_search_entry", "dds_is_element",
    "dds_col_fold_rows", "dds_col_fold_dec", "dds_col_fold_partial_device", "dds_combine_partials_device",
    "dds_opecol_create", "dds_opecol_destroy", "dds_opecol_count", "dds_opecol_truncate", "dds_opecol_append",
    "dds_opecol_append_dec", "dds_opecol_search", "dds_opecol_order",
    "dds_mctx_create", "dds_mctx_create_devices", "dds_mctx_destroy", "dds_mctx_shards", "dds_mcol_create",
    "dds_mcol_destroy", "dds_mcol_count", "dds_mcol_append", "dds_mcol_append_dec", "dds_mcol_fill_paillier_synth",
    "dds_mcol_fold", "dds_mcol_fold_rows", "dds_mcol_fold_dec",
    "dds_pair_modmul_dec", "dds_pair_stats", "dds_pair_timing", "dds_pair_set_policy", "dds_pair_cpu",
    "dds_col_write_rows", "dds_col_write_rows_dec", "dds_col_set_live", "dds_col_live_count", "dds_col_digit_rows",
    "dds_col_unit_rows",
    "dds_mcol_write_rows", "dds_mcol_write_rows_dec", "dds_mcol_set_live", "dds_mcol_live_count",
    "dds_opecol_write_rows", "dds_opecol_write_rows_dec", "dds_opecol_set_live", "dds_opecol_live_count",
    "dds_opecol_search_mask", "dds_ctx_cache_stats",
    "dds_strtab_append", "dds_strtab_write_rows", "dds_strtab_set_live", "dds_strtab_rows", "dds_strtab_live_count",
    "dds_strtab_stats", "dds_strtab_truncate", "dds_host_register", "dds_host_unregister", "dds_host_alloc",
    "dds_host_free", "dds_paillier_decrypt_batch_crt", "dds_col_decrypt_paillier",
    "dds_col_dec_width", "dds_col_read_dec", "dds_paillier_encrypt_batch_dec",
    "dds_rsa_decrypt_batch_crt", "dds_col_decrypt_rsa", "dds_rsa_crt_plan",
    "dds_max_prime_bits", "dds_strong_probable_prime_batch", "dds_probable_prime_batch", "dds_next_prime_batch",
    "dds_paillier_keygen_batch", "dds_rsa_keygen_batch", "dds_ctx_get_prime_timing",
    "dds_modexp_rows", "dds_col_append_pow", "dds_exprows_plan", "dds_col_fold_weighted",
    "dds_col_fold_weighted_dec", "dds_fold_weighted_plan",
    "dds_modinv_rows", "dds_col_append_inv", "dds_col_append_quot", "dds_col_append_mul",
    "dds_col_fold_groups", "dds_col_fold_groups_be", "dds_fold_groups_plan",
    "dds_ope_rank", "dds_ope_rank_device", "dds_col_fold_by_ope", "dds_col_fold_by_ope_be",
    "dds_col_append_scan", "dds_col_scan_be", "dds_scan_plan", "dds_col_scan_by_ope", "dds_col_scan_by_ope_be",
    "dds_col_append_scan_seg", "dds_col_scan_seg_be", "dds_segscan_plan", "dds_col_scan_part_by_ope",
    "dds_col_scan_part_by_ope_be", "dds_col_append_window", "dds_col_window_be", "dds_window_plan",
    "dds_col_fold_by_str", "dds_col_fold_by_str_be", "dds_strtab_read_elems",
]

_u8p = C.POINTER(C.c_uint8)
_sz = C.c_size_t
_szp = C.POINTER(C.c_size_t)


def _sig(name, res, *args):
    f = getattr(_lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_sig("dds_ctx_create", C.c_int, C.c_int, C.POINTER(C.c_void_p))
_sig("dds_ctx_destroy", C.c_int, C.c_void_p)
_sig("dds_strerror", C.c_char_p, C.c_int)
_sig("dds_last_error", C.c_char_p)
_sig("dds_max_modulus_bits", _sz)
_sig("dds_ctx_set_stream", C.c_int, C.c_void_p, C.c_void_p)
_sig("dds_ctx_set_timing", C.c_int, C.c_void_p, C.c_int)
_sig("dds_ctx_get_timing", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double))
_sig("dds_ctx_reset_timing", C.c_int, C.c_void_p)
_sig("dds_ctx_get_fold_work", C.c_int, C.c_void_p, C.POINTER(C.c_uint64))
for _n in ("dds_modmul_fold", "dds_paillier_sum", "dds_rsa_product"):
    _sig(_n, C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_void_p, _sz, _sz, _u8p, _sz, _szp)
_sig("dds_modmul_pairs", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, C.c_char_p, _sz, _sz, _u8p)
_sig("dds_bigint_sum", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, _u8p, _sz, _szp)
_sig("dds_bigint_product", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, _u8p, _sz, _szp)
_sig("dds_col_create", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, C.POINTER(C.c_void_p))
_sig("dds_col_destroy", C.c_int, C.c_void_p)
_sig("dds_col_append", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz)
_sig("dds_col_append_dec", C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), _sz)
_sig("dds_col_count", _sz, C.c_void_p)
_sig("dds_col_digit_rows", _sz, C.c_void_p)
_sig("dds_col_unit_rows", _sz, C.c_void_p)
_sig("dds_col_truncate", C.c_int, C.c_void_p, _sz)
_sig("dds_col_read", C.c_int, C.c_void_p, _sz, _sz, _u8p)
_sig("dds_col_dec_width", _sz, C.c_void_p)
_sig("dds_col_read_dec", C.c_int, C.c_void_p, _sz, _sz, C.c_void_p, _sz, C.POINTER(C.c_uint64), _szp)
_sig("dds_paillier_encrypt_batch_dec", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     C.c_char_p, _sz, C.POINTER(C.c_uint32), C.c_char_p, _sz, _sz, C.c_void_p, _sz, C.POINTER(C.c_uint64), _szp)
_sig("dds_col_fold", C.c_int, C.c_void_p, _sz, _sz, _u8p, _sz, _szp)
_sig("dds_col_fold_partial", C.c_int, C.c_void_p, _sz, _sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64))
_sig("dds_col_partial_words", _sz, C.c_void_p)
_sig("dds_combine_partials", C.c_int, C.c_void_p, C.c_char_p, _sz, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), _sz,
     _u8p, _sz, _szp)
_sig("dds_col_fill_paillier_synth", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_uint64, C.c_uint64,
     _sz, C.c_uint32)
_sig("dds_ope_filter", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_int64, C.c_int, C.c_void_p, _szp)
_sig("dds_ope_filter_device", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_int64, C.c_int, C.c_void_p, _szp)
_sig("dds_ope_order", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_int, C.c_void_p)
_sig("dds_ope_order_device", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_int, C.c_void_p)
_sig("dds_strtab_create", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz, C.POINTER(C.c_void_p))
_sig("dds_strtab_destroy", C.c_int, C.c_void_p)
_sig("dds_strtab_append", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz)
_sig("dds_strtab_write_rows", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p, C.c_void_p, _sz, C.c_void_p)
_sig("dds_strtab_set_live", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p)
_sig("dds_strtab_rows", _sz, C.c_void_p)
_sig("dds_strtab_live_count", _sz, C.c_void_p)
_sig("dds_strtab_stats", C.c_int, C.c_void_p, C.c_void_p, _sz)
_sig("dds_strtab_truncate", C.c_int, C.c_void_p, _sz)
_sig("dds_host_register", C.c_int, C.c_void_p, C.c_void_p, _sz)
_sig("dds_host_unregister", C.c_int, C.c_void_p, C.c_void_p)
_sig("dds_host_alloc", C.c_int, C.c_void_p, _sz, C.POINTER(C.c_void_p))
_sig("dds_host_free", C.c_int, C.c_void_p, C.c_void_p)
_sig("dds_search_eq", C.c_int, C.c_void_p, _sz, C.c_char_p, _sz, C.c_int, C.c_void_p, _szp)
_sig("dds_search_entry", C.c_int, C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), _sz, C.c_int, C.c_void_p,
     _szp)
_sig("dds_is_element", C.c_int, C.c_void_p, _sz, C.c_char_p, _sz, C.POINTER(C.c_int))
_sig("dds_paillier_encrypt_batch", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.POINTER(C.c_uint32),
     C.c_char_p, _sz, _sz, _u8p, _sz)
_sig("dds_paillier_encrypt_batch_crt", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     C.POINTER(C.c_uint32), C.c_char_p, _sz, _sz, _u8p, _sz)
_sig("dds_col_fill_table_synth", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, C.c_uint64, C.c_uint64, _sz)
_sig("dds_col_fill_random", C.c_int, C.c_void_p, _sz, C.c_uint64, C.c_uint64, _sz)
_sig("dds_col_encrypt_paillier", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz, C.c_char_p, _sz, C.c_char_p,
     _sz, C.c_char_p, _sz, C.c_char_p, _sz)
_sig("dds_paillier_decrypt_batch_crt", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     C.c_char_p, _sz, _sz, _u8p, _sz)
_sig("dds_col_decrypt_paillier", C.c_int, C.c_void_p, _sz, _sz, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     _u8p, _sz)
_sig("dds_rsa_decrypt_batch_crt", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     C.c_char_p, _sz, _sz, _u8p, _sz)
_sig("dds_col_decrypt_rsa", C.c_int, C.c_void_p, _sz, _sz, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz,
     _u8p, _sz)
_sig("dds_rsa_crt_plan", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int))
_sig("dds_max_prime_bits", _sz)
_sig("dds_strong_probable_prime_batch", C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, _sz, _sz, _u8p)
_sig("dds_probable_prime_batch", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, C.c_uint32, C.c_uint64, _u8p)
_sig("dds_next_prime_batch", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, C.c_uint32, C.c_uint64, _sz, _u8p, _sz)
_sig("dds_paillier_keygen_batch", C.c_int, C.c_void_p, _sz, C.c_uint64, C.c_uint64, _sz, C.c_uint32, _u8p, _u8p, _u8p,
     _u8p, _u8p, _sz, _sz, _sz)
_sig("dds_rsa_keygen_batch", C.c_int, C.c_void_p, _sz, C.c_char_p, _sz, C.c_uint64, C.c_uint64, _sz, C.c_uint32, _u8p,
     _u8p, _u8p, _sz, _sz)
_sig("dds_ctx_get_prime_timing", C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
     C.POINTER(C.c_double))
_sig("dds_modexp_batch", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_char_p, _sz, _sz, _u8p)
for _n in ("dds_sum_all_dec", "dds_mult_all_dec"):
    _sig(_n, C.c_int, C.c_void_p, C.POINTER(C.c_char_p), _sz, C.c_char_p, C.c_char_p, _sz, _szp)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_sig("dds_modexp_rows", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, _u64p, _sz, _u8p)
_sig("dds_col_append_pow", C.c_int, C.c_void_p, C.c_void_p, _sz, _sz, _u64p)
_sig("dds_exprows_plan", C.c_int, _sz, C.POINTER(C.c_int), _u64p)
_sig("dds_col_fold_weighted", C.c_int, C.c_void_p, _u64p, _sz, _sz, _i64p, _sz, _u8p, _sz, _szp)
_sig("dds_col_fold_weighted_dec", C.c_int, C.c_void_p, _u64p, _sz, _sz, _i64p, _sz, C.c_char_p, _sz, _szp)
_sig("dds_fold_weighted_plan", C.c_int, _sz, _sz, _sz, C.POINTER(C.c_int), _u64p, _u64p)
_sig("dds_modinv_rows", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, _sz, _u8p, _szp)
_sig("dds_col_append_inv", C.c_int, C.c_void_p, C.c_void_p, _sz, _sz, _szp)
_sig("dds_col_append_quot", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz, _sz, _szp)
_sig("dds_col_append_mul", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz, _sz)
_u32p = C.POINTER(C.c_uint32)
_sig("dds_col_fold_groups", C.c_int, C.c_void_p, _u64p, _sz, _sz, _u32p, _sz, C.c_void_p, _u64p)
_sig("dds_col_fold_groups_be", C.c_int, C.c_void_p, _u64p, _sz, _sz, _u32p, _sz, _u8p, _u64p)
_sig("dds_fold_groups_plan", C.c_int, _sz, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p, _u64p)
_sig("dds_ope_rank", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, _u32p, _i64p, _u64p, _szp)
_sig("dds_ope_rank_device", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz, C.c_void_p, C.c_void_p, C.c_void_p, _szp)
_sig("dds_col_fold_by_ope", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, C.c_void_p, _i64p, _u64p, _sz, _szp)
_sig("dds_col_fold_by_ope_be", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, _u8p, _i64p, _u64p, _sz, _szp)
_sig("dds_col_fold_by_str", C.c_int, C.c_void_p, C.c_void_p, _sz, _u64p, _sz, C.c_void_p, _u64p, _u64p, _sz, _szp,
     C.POINTER(C.c_int))
_sig("dds_col_fold_by_str_be", C.c_int, C.c_void_p, C.c_void_p, _sz, _u64p, _sz, _u8p, _u64p, _u64p, _sz, _szp,
     C.POINTER(C.c_int))
_sig("dds_strtab_read_elems", C.c_int, C.c_void_p, _u64p, _sz, _sz, C.c_void_p, _sz, _u64p, _u8p, _szp)
_sig("dds_col_append_scan", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, _sz, C.c_int)
_sig("dds_col_scan_be", C.c_int, C.c_void_p, _u64p, _sz, _sz, C.c_int, _u8p)
_sig("dds_scan_plan", C.c_int, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p, _u64p)
_sig("dds_col_scan_by_ope", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, C.c_int, C.c_void_p, _i64p, _u64p, _sz, _szp)
_sig("dds_col_scan_by_ope_be", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, C.c_int, _u8p, _i64p, _u64p, _sz, _szp)
_sig("dds_col_append_scan_seg", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, _sz, _u64p, _sz, C.c_int)
_sig("dds_col_scan_seg_be", C.c_int, C.c_void_p, _u64p, _sz, _sz, _u64p, _sz, C.c_int, _u8p)
_sig("dds_segscan_plan", C.c_int, _sz, _u64p, _sz, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p, _u64p)
_sig("dds_col_scan_part_by_ope", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, C.c_int, C.c_void_p, _u64p, _sz, _i64p,
     _u64p, _sz, _szp, _szp)
_sig("dds_col_scan_part_by_ope_be", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, C.c_int, _u8p, _u64p, _sz, _i64p,
     _u64p, _sz, _szp, _szp)
_sig("dds_col_append_window", C.c_int, C.c_void_p, C.c_void_p, _u64p, _sz, _sz, _sz)
_sig("dds_col_window_be", C.c_int, C.c_void_p, _u64p, _sz, _sz, _sz, _u8p)
_sig("dds_window_plan", C.c_int, _sz, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p, _u64p)
_sig("dds_pair_modmul_dec", C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, _sz, _szp)
_sig("dds_pair_stats", C.c_int, C.c_void_p, _u64p, _u64p)
_sig("dds_pair_timing", C.c_int, C.c_void_p, _u64p, _u64p, _u64p, _u64p)
_sig("dds_pair_set_policy", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int))
_sig("dds_pair_cpu", C.c_int, C.c_void_p, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p)
_sig("dds_ctx_cache_stats", C.c_int, C.c_void_p, _szp, _szp)
_sig("dds_col_fold_rows", C.c_int, C.c_void_p, _u64p, _sz, _u8p, _sz, _szp)
_sig("dds_col_fold_dec", C.c_int, C.c_void_p, _u64p, _sz, C.c_char_p, _sz, _szp)
_sig("dds_col_fold_partial_device", C.c_int, C.c_void_p, _sz, _sz, C.c_void_p)
_sig("dds_combine_partials_device", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_void_p, _u64p, _sz, _u8p, _sz, _szp)
_sig("dds_opecol_create", C.c_int, C.c_void_p, _sz, C.POINTER(C.c_void_p))
_sig("dds_opecol_destroy", C.c_int, C.c_void_p)
_sig("dds_opecol_count", _sz, C.c_void_p)
_sig("dds_opecol_truncate", C.c_int, C.c_void_p, _sz)
_sig("dds_opecol_append", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _sz)
_sig("dds_opecol_append_dec", C.c_int, C.c_void_p, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, _sz)
_sig("dds_opecol_search", C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, _szp)
_sig("dds_opecol_order", C.c_int, C.c_void_p, C.c_int, C.c_void_p, _szp)
_sig("dds_opecol_search_mask", C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, _sz, _szp)
_sig("dds_opecol_write_rows", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _sz)
_sig("dds_opecol_write_rows_dec", C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, _sz)
_sig("dds_opecol_set_live", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p)
_sig("dds_opecol_live_count", _sz, C.c_void_p)
for _p in ("dds_col", "dds_mcol"):
    _sig(_p + "_write_rows", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p, _sz)
    _sig(_p + "_write_rows_dec", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_char_p, C.c_void_p)
    _sig(_p + "_set_live", C.c_int, C.c_void_p, C.c_void_p, _sz, C.c_void_p)
    _sig(_p + "_live_count", _sz, C.c_void_p)
_sig("dds_mctx_create", C.c_int, C.c_uint64, C.POINTER(C.c_void_p))
_sig("dds_mctx_create_devices", C.c_int, C.POINTER(C.c_int), _sz, C.POINTER(C.c_void_p))
_sig("dds_mctx_destroy", C.c_int, C.c_void_p)
_sig("dds_mctx_shards", _sz, C.c_void_p)
_sig("dds_mcol_create", C.c_int, C.c_void_p, C.c_char_p, _sz, _sz, C.POINTER(C.c_void_p))
_sig("dds_mcol_destroy", C.c_int, C.c_void_p)
_sig("dds_mcol_count", _sz, C.c_void_p)
_sig("dds_mcol_append", C.c_int, C.c_void_p, C.c_void_p, _sz, _sz)
_sig("dds_mcol_append_dec", C.c_int, C.c_void_p, C.c_char_p, _u64p, _sz)
_sig("dds_mcol_fill_paillier_synth", C.c_int, C.c_void_p, C.c_char_p, _sz, C.c_char_p, _sz, C.c_uint64, _sz,
     C.c_uint32)
_sig("dds_mcol_fold", C.c_int, C.c_void_p, _u8p, _sz, _szp)
_sig("dds_mcol_fold_rows", C.c_int, C.c_void_p, _u64p, _sz, _u8p, _sz, _szp)
_sig("dds_mcol_fold_dec", C.c_int, C.c_void_p, _u64p, _sz, C.c_char_p, _sz, _szp)


class DDSError(RuntimeError):
    def __init__(self, status: int, where: str, row=None):
        self.status = status
        self.row = row  # the row-wise inversions' non-unit row (dds_modinv_rows, append_inv, append_quot), else None
        detail = _lib.dds_last_error().decode(errors="replace")
        super().__init__(f"{where}: {_lib.dds_strerror(status).decode()} ({detail})")


class NotFound(DDSError):
    """DDS_E_EMPTY: the reference route answers HTTP 404."""


def _be_int(buf, n: int) -> int:
    """Big-endian integer from the first n bytes of a ctypes buffer (one memcpy; slicing a ctypes array
    builds a Python list of ints first)."""
    return int.from_bytes(C.string_at(C.addressof(buf), n), "big")


def _check(rc: int, where: str):
    if rc == DDS_E_EMPTY:
        raise NotFound(rc, where)
    if rc != DDS_OK:
        raise DDSError(rc, where)


_NO_ROW = C.c_size_t(-1).value


def _check_row(rc: int, where: str, bad):
    """_check for the calls that name a row: a DDS_E_RANGE that set *bad_row carries it as .row"""
    if rc == DDS_E_RANGE and bad.value != _NO_ROW:
        raise DDSError(rc, where, bad.value)
    _check(rc, where)


def int_to_be(x: int, width: int) -> bytes:
    return int(x).to_bytes(width, "big")


def ints_to_be(xs, width: int) -> bytes:
    return b"".join(int(x).to_bytes(width, "big") for x in xs)


def nbytes(x: int) -> int:
    return max(1, (int(x).bit_length() + 7) // 8)


def _split_dec(chars: np.ndarray, offs: np.ndarray) -> list[str]:
    """The rows of an Arrow-style decimal column (uint8 chars, uint64 offsets[count+1]) as str."""
    raw = chars.tobytes().decode("ascii")
    o = offs.tolist()
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def _ids(row_ids) -> np.ndarray:
    return np.ascontiguousarray(row_ids, dtype=np.uint64)


def _u64_array(xs) -> np.ndarray:
    """Exponents below 2^64 as a contiguous uint64 array (an array of that type is taken as it is)."""
    if isinstance(xs, np.ndarray) and xs.dtype == np.uint64:
        return np.ascontiguousarray(xs)
    return np.ascontiguousarray([int(x) for x in xs], dtype=np.uint64)


def _dec_rows(rows):
    """(chars, uint64 offsets[len+1], count) of decimal rows (str / bytes) or an Arrow-style pair."""
    if isinstance(rows, tuple):
        chars, offs = rows
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        return chars, offs, len(offs) - 1
    enc = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    return b"".join(enc) or b"\0", offs, len(enc)


class _Mutable:
    """Row writes and the live mask of a resident ciphertext column (dds_col_* / dds_mcol_*): the
    write routes WriteElement / AddElement / RemoveSet (DDSRestServer.scala:207-321) applied in place."""
    _pre = ""

    def write_rows(self, row_ids, ops):
        ids = _ids(row_ids)
        ops = [int(x) for x in ops]
        assert len(ops) == len(ids)
        width = max([self.mb] + [nbytes(x) for x in ops])
        _check(getattr(_lib, self._pre + "_write_rows")(self._h, ids.ctypes.data, len(ids), ints_to_be(ops, width),
                                                        width), self._pre + "_write_rows")

    def write_rows_dec(self, row_ids, rows):
        ids = _ids(row_ids)
        chars, offs, n = _dec_rows(rows)
        assert n == len(ids)
        _check(getattr(_lib, self._pre + "_write_rows_dec")(self._h, ids.ctypes.data, n, chars, offs.ctypes.data),
               self._pre + "_write_rows_dec")

    def set_live(self, row_ids, live):
        ids = _ids(row_ids)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(live, dtype=np.uint8), ids.shape))
        _check(getattr(_lib, self._pre + "_set_live")(self._h, ids.ctypes.data, len(ids), flags.ctypes.data),
               self._pre + "_set_live")

    @property
    def live_count(self) -> int:
        return getattr(_lib, self._pre + "_live_count")(self._h)


class Engine:
    """One dds_ctx on one GPU."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(_lib.dds_ctx_create(device, C.byref(h)), "dds_ctx_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.dds_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- context controls ----
    def set_stream(self, stream_ptr: int | None):
        _check(_lib.dds_ctx_set_stream(self._h, C.c_void_p(stream_ptr or 0)), "set_stream")

    def set_timing(self, on: bool):
        _check(_lib.dds_ctx_set_timing(self._h, int(on)), "set_timing")

    def reset_timing(self):
        _check(_lib.dds_ctx_reset_timing(self._h), "reset_timing")

    def timing(self):
        """(fold_ms, fold_launches, other_ms, fold_modmuls) accumulated since reset_timing()."""
        ms, n, tot, mm = C.c_double(), C.c_uint64(), C.c_double(), C.c_uint64()
        _check(_lib.dds_ctx_get_timing(self._h, C.byref(ms), C.byref(n), C.byref(tot)), "get_timing")
        _check(_lib.dds_ctx_get_fold_work(self._h, C.byref(mm)), "get_fold_work")
        return ms.value, n.value, tot.value, mm.value

    # ---- folds ----
    def _fold(self, fn, modulus: int, ops, width: int | None = None) -> int:
        ops = [int(x) for x in ops]
        mb = nbytes(modulus)
        width = width or max([mb] + [nbytes(x) for x in ops])
        buf = ints_to_be(ops, width)
        out = (C.c_uint8 * max(width, mb))()
        olen = C.c_size_t()
        _check(fn(self._h, int_to_be(modulus, mb), mb, buf, width, len(ops), out, len(out), C.byref(olen)), fn.__name__)
        return _be_int(out, olen.value)

    def fold_buffer(self, modulus: int, buf: np.ndarray) -> int:
        """dds_modmul_fold over a host buffer of fixed-width big-endian rows (uint8 [count, width]):
        the binary boundary a JNA shim hands over, without per-row Python conversion."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        count, width = buf.shape
        mb = nbytes(modulus)
        out = (C.c_uint8 * max(width, mb))()
        olen = C.c_size_t()
        _check(_lib.dds_modmul_fold(self._h, int_to_be(modulus, mb), mb, buf.ctypes.data, width, count, out, len(out),
                                    C.byref(olen)), "dds_modmul_fold")
        return _be_int(out, olen.value)

    def modmul_fold(self, modulus: int, ops, width=None) -> int:
        return self._fold(_lib.dds_modmul_fold, modulus, ops, width)

    def paillier_sum(self, nsquare: int, ciphertexts, width=None) -> int:
        """HomoAdd fold: DDSRestServer.scala:412-430."""
        return self._fold(_lib.dds_paillier_sum, nsquare, ciphertexts, width)

    def rsa_product(self, n: int, ciphertexts, width=None) -> int:
        """HomoMult fold: DDSRestServer.scala:506-524."""
        return self._fold(_lib.dds_rsa_product, n, ciphertexts, width)

    def modmul_pairs(self, modulus: int, a, b) -> list[int]:
        a, b = [int(x) for x in a], [int(x) for x in b]
        assert len(a) == len(b)
        mb = nbytes(modulus)
        width = max([mb] + [nbytes(x) for x in a + b])
        out = (C.c_uint8 * (mb * max(1, len(a))))()
        _check(_lib.dds_modmul_pairs(self._h, int_to_be(modulus, mb), mb, ints_to_be(a, width), ints_to_be(b, width),
                                     width, len(a), out), "dds_modmul_pairs")
        raw = bytes(out)
        return [int.from_bytes(raw[i * mb:(i + 1) * mb], "big") for i in range(len(a))]

    def bigint_sum(self, ops) -> int:
        ops = [int(x) for x in ops]
        width = max([1] + [nbytes(x) for x in ops])
        out = (C.c_uint8 * (width + 16))()
        olen = C.c_size_t()
        _check(_lib.dds_bigint_sum(self._h, ints_to_be(ops, width), width, len(ops), out, len(out), C.byref(olen)),
               "dds_bigint_sum")
        return _be_int(out, olen.value)

    def bigint_product(self, ops) -> int:
        """Unbounded product (MultAll without pubkey, DDSRestServer.scala:520)."""
        ops = [int(x) for x in ops]
        width = max([1] + [nbytes(x) for x in ops])
        out = (C.c_uint8 * (width * max(1, len(ops)) + 8))()
        olen = C.c_size_t()
        _check(_lib.dds_bigint_product(self._h, ints_to_be(ops, width), width, len(ops), out, len(out),
                                       C.byref(olen)), "dds_bigint_product")
        return _be_int(out, olen.value)

    # ---- decimal route entry points ----
    def _dec(self, fn, values, modulus: str | None) -> str:
        arr = (C.c_char_p * max(1, len(values)))(*[str(v).encode() for v in values])
        cap = sum(len(str(v)) for v in values) * 2 + 64 + (len(modulus) * 2 if modulus else 0)
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _check(fn(self._h, arr, len(values), modulus.encode() if modulus is not None else None, out, cap,
                  C.byref(olen)), fn.__name__)
        return out.value.decode()

    def sum_all_dec(self, values, nsqr: str | None) -> str:
        return self._dec(_lib.dds_sum_all_dec, values, nsqr)

    def mult_all_dec(self, values, n: str | None) -> str:
        return self._dec(_lib.dds_mult_all_dec, values, n)

    def pair_modmul_dec(self, op1: str, op2: str, modulus: str) -> str:
        """op1*op2 mod modulus (BigInteger semantics): GET /Sum with nsqr, GET /Mult with a pubkey.
        Concurrent calls under one modulus share one k_pairs launch (dds_pair_modmul_dec)."""
        a, b, m = str(op1).encode(), str(op2).encode(), str(modulus).encode()
        cap = 2 * len(m) + 64
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _check(_lib.dds_pair_modmul_dec(self._h, a, b, m, out, cap, C.byref(olen)), "dds_pair_modmul_dec")
        return out.value.decode()

    def pair_stats(self):
        """(calls, k_pairs launches) of pair_modmul_dec on this engine."""
        calls, launches = C.c_uint64(), C.c_uint64()
        _check(_lib.dds_pair_stats(self._h, C.byref(calls), C.byref(launches)), "dds_pair_stats")
        return calls.value, launches.value

    def pair_timing(self):
        """(leader ns over all batches, GPU round-trip ns, longest batch ns and longest round trip ns
        since the last call) of pair_modmul_dec"""
        b, g, m, mg = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_pair_timing(self._h, C.byref(b), C.byref(g), C.byref(m), C.byref(mg)), "dds_pair_timing")
        return b.value, g.value, m.value, mg.value

    def pair_set_policy(self, policy: int) -> int:
        """Serve pair_modmul_dec by GPU batches (DDS_PAIR_GPU), lone requests on the host
        (DDS_PAIR_LONE) or every request on the host (DDS_PAIR_HOST); policy < 0 only queries.
        Returns the policy in force before the call."""
        prev = C.c_int()
        _check(_lib.dds_pair_set_policy(self._h, int(policy), C.byref(prev)), "dds_pair_set_policy")
        return prev.value

    def pair_cpu(self) -> dict:
        """Cumulative host CPU ns of pair_modmul_dec by phase (dds_pair_cpu) and host-served requests."""
        v = [C.c_uint64() for _ in range(6)]
        _check(_lib.dds_pair_cpu(self._h, *[C.byref(x) for x in v]), "dds_pair_cpu")
        return dict(zip(("codec_ns", "pack_ns", "queue_ns", "wait_ns", "host_ns", "host_calls"), (x.value for x in v)))

    def cache_stats(self):
        """(cached modulus constants, live pairwise queues) of this engine"""
        m, q = C.c_size_t(), C.c_size_t()
        _check(_lib.dds_ctx_cache_stats(self._h, C.byref(m), C.byref(q)), "dds_ctx_cache_stats")
        return m.value, q.value

    # ---- OPE filter ----
    def ope_filter(self, col, valid, bound: int, op: str) -> np.ndarray:
        col = np.ascontiguousarray(col, dtype=np.int64)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        out = np.empty(max(1, len(col)), dtype=np.uint32)
        got = C.c_size_t()
        _check(_lib.dds_ope_filter(self._h, col.ctypes.data, None if v is None else v.ctypes.data, len(col),
                                   int(bound), OPE_OPS[op], out.ctypes.data, C.byref(got)), "dds_ope_filter")
        return out[: got.value].copy()

    def ope_filter_device(self, d_col: int, d_valid: int | None, n: int, bound: int, op: str, d_out: int) -> int:
        got = C.c_size_t()
        _check(_lib.dds_ope_filter_device(self._h, C.c_void_p(d_col), C.c_void_p(d_valid or 0), n, int(bound),
                                          OPE_OPS[op], C.c_void_p(d_out), C.byref(got)), "dds_ope_filter_device")
        return got.value

    def ope_order(self, col, valid, descending: bool) -> np.ndarray:
        """OrderLS (descending=True) / OrderSL row permutation (dds_ope_order)."""
        col = np.ascontiguousarray(col, dtype=np.int64)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        out = np.empty(len(col), dtype=np.uint32)
        _check(_lib.dds_ope_order(self._h, col.ctypes.data_as(C.c_void_p),
                                  None if v is None else v.ctypes.data_as(C.c_void_p), len(col), int(descending),
                                  out.ctypes.data_as(C.c_void_p)), "dds_ope_order")
        return out

    def ope_order_device(self, d_col: int, d_valid: int | None, n: int, descending: bool, d_out: int):
        _check(_lib.dds_ope_order_device(self._h, C.c_void_p(d_col), C.c_void_p(d_valid or 0), n, int(descending),
                                         C.c_void_p(d_out)), "dds_ope_order_device")

    def ope_rank(self, col, valid=None):
        """dds_ope_rank: (labels, keys, counts) of the int64 keys `col` among the rows with valid[i] != 0 (None:
        every row): labels[i] (uint32) = the dense rank of col[i] in ascending order, 0xFFFFFFFF for an invalid
        row; keys (int64) = the distinct values; counts (uint64) = the rows holding each."""
        col = np.ascontiguousarray(col, dtype=np.int64)
        v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        n = len(col)
        labels = np.empty(max(1, n), dtype=np.uint32)
        keys = np.empty(max(1, n), dtype=np.int64)
        counts = np.empty(max(1, n), dtype=np.uint64)
        ng = C.c_size_t()
        _check(_lib.dds_ope_rank(self._h, col.ctypes.data, None if v is None else v.ctypes.data, n,
                                 labels.ctypes.data_as(_u32p), keys.ctypes.data_as(_i64p),
                                 counts.ctypes.data_as(_u64p), C.byref(ng)), "dds_ope_rank")
        return labels[:n], keys[:ng.value].copy(), counts[:ng.value].copy()

    def ope_rank_device(self, d_col: int, d_valid: int | None, n: int, d_labels: int | None, d_keys: int | None,
                        d_counts: int | None) -> int:
        """dds_ope_rank_device: the same on device pointers (uint32 labels and counts, int64 keys; any of the
        three may be None); returns the number of distinct keys."""
        ng = C.c_size_t()
        _check(_lib.dds_ope_rank_device(self._h, C.c_void_p(d_col), C.c_void_p(d_valid or 0), n,
                                        C.c_void_p(d_labels or 0), C.c_void_p(d_keys or 0),
                                        C.c_void_p(d_counts or 0), C.byref(ng)), "dds_ope_rank_device")
        return ng.value

    # ---- encryption ----
    def paillier_encrypt_batch(self, n: int, g: int, ms, rs) -> list[int]:
        ms = np.ascontiguousarray(ms, dtype=np.uint32)
        rs = [int(r) for r in rs]
        nsq = n * n
        nb, rw = nbytes(nsq), max([1] + [nbytes(r) for r in rs])
        out = (C.c_uint8 * (nb * max(1, len(rs))))()
        _check(_lib.dds_paillier_encrypt_batch(self._h, int_to_be(n, nbytes(n)), nbytes(n), int_to_be(g, nbytes(g)),
                                               nbytes(g), ms.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               ints_to_be(rs, rw), rw, len(rs), out, nb), "dds_paillier_encrypt_batch")
        raw = bytes(out)
        return [int.from_bytes(raw[i * nb:(i + 1) * nb], "big") for i in range(len(rs))]

    def paillier_encrypt_batch_crt(self, p: int, q: int, g: int, ms, rs) -> list[int]:
        """HomoAdd.encrypt(m, PaillierKey) with the private factors: same ciphertexts, CRT halves."""
        ms = np.ascontiguousarray(ms, dtype=np.uint32)
        rs = [int(r) for r in rs]
        nb, rw = nbytes((p * q) ** 2), max([1] + [nbytes(r) for r in rs])
        out = (C.c_uint8 * (nb * max(1, len(rs))))()
        _check(_lib.dds_paillier_encrypt_batch_crt(self._h, int_to_be(p, nbytes(p)), nbytes(p), int_to_be(q, nbytes(q)),
                                                   nbytes(q), int_to_be(g, nbytes(g)), nbytes(g),
                                                   ms.ctypes.data_as(C.POINTER(C.c_uint32)), ints_to_be(rs, rw), rw,
                                                   len(rs), out, nb), "dds_paillier_encrypt_batch_crt")
        raw = bytes(out)
        return [int.from_bytes(raw[i * nb:(i + 1) * nb], "big") for i in range(len(rs))]

    def paillier_encrypt_batch_dec(self, n: int, g: int, ms, rs, p: int | None = None, q: int | None = None) -> list[str]:
        """dds_paillier_encrypt_batch_dec: the ciphertexts of paillier_encrypt_batch (or, with p and q,
        of paillier_encrypt_batch_crt) as the BigInteger.toString text a PutSet carries, printed on the GPU."""
        ms = np.ascontiguousarray(ms, dtype=np.uint32)
        rs = [int(r) for r in rs]
        count, rw = len(rs), max([1] + [nbytes(r) for r in rs])
        pb = None if p is None else int_to_be(p, nbytes(p))
        qb = None if q is None else int_to_be(q, nbytes(q))
        chars = np.empty(max(1, count * len(str(n * n - 1))), dtype=np.uint8)
        offs = np.zeros(count + 1, dtype=np.uint64)
        used = C.c_size_t()
        _check(_lib.dds_paillier_encrypt_batch_dec(
            self._h, int_to_be(n, nbytes(n)), nbytes(n), int_to_be(g, nbytes(g)), nbytes(g), pb, len(pb or b""), qb,
            len(qb or b""), ms.ctypes.data_as(C.POINTER(C.c_uint32)), ints_to_be(rs, rw), rw, count,
            chars.ctypes.data, chars.nbytes, offs.ctypes.data_as(_u64p), C.byref(used)), "dds_paillier_encrypt_batch_dec")
        return _split_dec(chars[:used.value], offs)

    def paillier_decrypt_batch_crt(self, p: int, q: int, g: int, cs) -> list[int]:
        """HomoAdd.decrypt(c, PaillierKey) for each c in cs (values in [0, n^2), coprime to n)."""
        cs = [int(c) for c in cs]
        nb, cw = nbytes(p * q), max([1] + [nbytes(c) for c in cs])
        out = (C.c_uint8 * (nb * max(1, len(cs))))()
        _check(_lib.dds_paillier_decrypt_batch_crt(self._h, int_to_be(p, nbytes(p)), nbytes(p), int_to_be(q, nbytes(q)),
                                                   nbytes(q), int_to_be(g, nbytes(g)), nbytes(g), ints_to_be(cs, cw),
                                                   cw, len(cs), out, nb), "dds_paillier_decrypt_batch_crt")
        raw = bytes(out)
        return [int.from_bytes(raw[i * nb:(i + 1) * nb], "big") for i in range(len(cs))]

    def rsa_decrypt_batch_crt(self, p: int, q: int, d: int, cs) -> list[int]:
        """HomoMult.decrypt(priv, c) = c^d mod p*q for each c in cs (values in [0, p*q)) through the CRT halves."""
        cs = [int(c) for c in cs]
        nb, cw = nbytes(p * q), max([1] + [nbytes(c) for c in cs])
        out = (C.c_uint8 * (nb * max(1, len(cs))))()
        _check(_lib.dds_rsa_decrypt_batch_crt(self._h, int_to_be(p, nbytes(p)), nbytes(p), int_to_be(q, nbytes(q)),
                                              nbytes(q), int_to_be(d, nbytes(d)), nbytes(d), ints_to_be(cs, cw), cw,
                                              len(cs), out, nb), "dds_rsa_decrypt_batch_crt")
        raw = bytes(out)
        return [int.from_bytes(raw[i * nb:(i + 1) * nb], "big") for i in range(len(cs))]

    def rsa_crt_plan(self, p: int, q: int) -> tuple:
        """dds_rsa_crt_plan: ((s1_p, qp_p), (s1_q, qp_q)); s1 = 20 | 40 (one bignum per lane), 0 (lane groups),
        -1 (full width over n); qp: that ladder reduces against N*n'. No GPU work."""
        s1, qp = (C.c_int * 2)(), (C.c_int * 2)()
        _check(_lib.dds_rsa_crt_plan(self._h, int_to_be(p, nbytes(p)), nbytes(p), int_to_be(q, nbytes(q)), nbytes(q),
                                     s1, qp), "dds_rsa_crt_plan")
        return ((s1[0], bool(qp[0])), (s1[1], bool(qp[1])))

    # ---- prime search and key generation ----
    @staticmethod
    def _rows(buf, count: int, width: int) -> list[int]:
        raw = bytes(buf)
        return [int.from_bytes(raw[i * width:(i + 1) * width], "big") for i in range(count)]

    def strong_probable_prime_batch(self, ns, bases) -> list[int]:
        """flags[i] = 1 iff ns[i] (odd, >= 3) is a strong probable prime to bases[i] (in [1, ns[i] - 1])."""
        ns, bases = [int(x) for x in ns], [int(x) for x in bases]
        assert len(ns) == len(bases)
        width = max([1] + [nbytes(x) for x in ns + bases])
        flags = (C.c_uint8 * max(1, len(ns)))()
        _check(_lib.dds_strong_probable_prime_batch(self._h, ints_to_be(ns, width), ints_to_be(bases, width), width,
                                                    len(ns), flags), "dds_strong_probable_prime_batch")
        return list(flags)[:len(ns)]

    def probable_prime_batch(self, ns, rounds: int = 24, seed: int = 0) -> list[int]:
        """flags[i] = 1 iff ns[i] >= 0 is a probable prime: base 2, then `rounds` seeded witnesses."""
        ns = [int(x) for x in ns]
        width = max([1] + [nbytes(x) for x in ns])
        flags = (C.c_uint8 * max(1, len(ns)))()
        _check(_lib.dds_probable_prime_batch(self._h, ints_to_be(ns, width), width, len(ns), rounds, seed, flags),
               "dds_probable_prime_batch")
        return list(flags)[:len(ns)]

    def next_prime_batch(self, starts, rounds: int = 24, seed: int = 0, window: int = 0) -> list[int]:
        """The smallest probable prime >= each start (window: odd candidates sieved per pass, 0: the default)."""
        starts = [int(x) for x in starts]
        width = max([1] + [nbytes(x) for x in starts])
        ow = width + 1
        out = (C.c_uint8 * (ow * max(1, len(starts))))()
        _check(_lib.dds_next_prime_batch(self._h, ints_to_be(starts, width), width, len(starts), rounds, seed, window,
                                         out, ow), "dds_next_prime_batch")
        return self._rows(out, len(starts), ow)

    def paillier_keygen_batch(self, bits: int, seed: int, count: int = 1, first: int = 0, rounds: int = 24) -> list[dict]:
        """HomoAdd.generateKey for keys first .. first + count - 1 of (bits, seed): dicts with the fields of
        tests/golden/keys.json (g, lambda, mu, n, nsquare, p, q)."""
        fb, nb, gb = (bits + 15) // 16, (bits + 7) // 8, (bits + 3) // 4
        m = max(1, count)
        p, q, g = (C.c_uint8 * (fb * m))(), (C.c_uint8 * (fb * m))(), (C.c_uint8 * (gb * m))()
        lam, mu = (C.c_uint8 * (nb * m))(), (C.c_uint8 * (nb * m))()
        _check(_lib.dds_paillier_keygen_batch(self._h, bits, seed, first, count, rounds, p, q, g, lam, mu, fb, nb, gb),
               "dds_paillier_keygen_batch")
        cols = [self._rows(b, count, w) for b, w in ((p, fb), (q, fb), (g, gb), (lam, nb), (mu, nb))]
        return [{"g": gi, "lambda": li, "mu": mi, "n": pi * qi, "nsquare": (pi * qi) ** 2, "p": pi, "q": qi}
                for pi, qi, gi, li, mi in zip(*cols)]

    def rsa_keygen_batch(self, bits: int, seed: int, count: int = 1, first: int = 0, rounds: int = 24,
                         e: int = 65537) -> list[dict]:
        """HomoMult.generateKey for keys first .. first + count - 1 of (bits, seed): dicts n, e, d, p, q."""
        fb, nb = (bits + 15) // 16, (bits + 7) // 8
        m = max(1, count)
        p, q, d = (C.c_uint8 * (fb * m))(), (C.c_uint8 * (fb * m))(), (C.c_uint8 * (nb * m))()
        _check(_lib.dds_rsa_keygen_batch(self._h, bits, int_to_be(e, nbytes(e)), nbytes(e), seed, first, count, rounds,
                                         p, q, d, fb, nb), "dds_rsa_keygen_batch")
        cols = [self._rows(b, count, w) for b, w in ((p, fb), (q, fb), (d, nb))]
        return [{"n": pi * qi, "e": e, "d": di, "p": pi, "q": qi} for pi, qi, di in zip(*cols)]

    def prime_timing(self) -> tuple:
        """(sieve_ms, base2_ms, witness_ms) of the prime search since reset_timing(), with timing on."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(_lib.dds_ctx_get_prime_timing(self._h, C.byref(a), C.byref(b), C.byref(c)), "dds_ctx_get_prime_timing")
        return a.value, b.value, c.value

    def modexp_batch(self, modulus: int, exponent: int, bases) -> list[int]:
        """out[i] = bases[i]^exponent mod modulus (HomoMult.encrypt for an RSA key)."""
        bases = [int(x) for x in bases]
        mb = nbytes(modulus)
        width = max([mb] + [nbytes(x) for x in bases])
        out = (C.c_uint8 * (mb * max(1, len(bases))))()
        _check(_lib.dds_modexp_batch(self._h, int_to_be(modulus, mb), mb, int_to_be(exponent, nbytes(exponent)),
                                     nbytes(exponent), ints_to_be(bases, width), width, len(bases), out),
               "dds_modexp_batch")
        raw = bytes(out)
        return [int.from_bytes(raw[i * mb:(i + 1) * mb], "big") for i in range(len(bases))]

    def modexp_rows(self, modulus: int, bases, exps) -> list[int]:
        """dds_modexp_rows: out[i] = bases[i]^exps[i] mod modulus, an exponent below 2^64 of its own per row
        (Paillier's scalar multiple Enc(k m) = c^k mod n^2)."""
        bases = [int(x) for x in bases]
        e = _u64_array(exps)
        if len(e) != len(bases):
            raise ValueError("one exponent per base")
        mb = nbytes(modulus)
        width = max([mb] + [nbytes(x) for x in bases])
        out = (C.c_uint8 * (mb * max(1, len(bases))))()
        _check(_lib.dds_modexp_rows(self._h, int_to_be(modulus, mb), mb, ints_to_be(bases, width), width,
                                    e.ctypes.data_as(_u64p), len(bases), out), "dds_modexp_rows")
        raw = bytes(out)
        return [int.from_bytes(raw[i * mb:(i + 1) * mb], "big") for i in range(len(bases))]

    def modinv_rows(self, modulus: int, rows) -> list[int]:
        """dds_modinv_rows: out[i] = rows[i]^-1 mod modulus (Enc(-m) = c^-1 mod n^2 for a Paillier ciphertext), by
        one batch inversion on the GPU. A row that is not coprime to the modulus: DDSError with .row naming one."""
        rows = [int(x) for x in rows]
        mb = nbytes(modulus)
        width = max([mb] + [nbytes(x) for x in rows])
        out = (C.c_uint8 * (mb * max(1, len(rows))))()
        bad = C.c_size_t(_NO_ROW)
        _check_row(_lib.dds_modinv_rows(self._h, int_to_be(modulus, mb), mb, ints_to_be(rows, width), width, len(rows),
                                        out, C.byref(bad)), "dds_modinv_rows", bad)
        raw = bytes(out)
        return [int.from_bytes(raw[i * mb:(i + 1) * mb], "big") for i in range(len(rows))]

    @staticmethod
    def exprows_plan(bits: int) -> tuple:
        """dds_exprows_plan: (window, Montgomery products per row) of a per-row ladder call whose largest
        exponent has `bits` bits. No GPU work."""
        w, p = C.c_int(), C.c_uint64()
        _check(_lib.dds_exprows_plan(bits, C.byref(w), C.byref(p)), "dds_exprows_plan")
        return w.value, p.value

    @staticmethod
    def fold_weighted_plan(rows: int, bits: int, window: int = 0) -> tuple:
        """dds_fold_weighted_plan: (window, fold products, host products) the weighted fold's plan predicts for
        `rows` rows and weights of up to `bits` bits (window 0: the default). No GPU work."""
        c, rp, hp = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_fold_weighted_plan(rows, bits, window, C.byref(c), C.byref(rp), C.byref(hp)),
               "dds_fold_weighted_plan")
        return c.value, rp.value, hp.value

    @staticmethod
    def fold_groups_plan(n: int, max_group: int) -> tuple:
        """dds_fold_groups_plan: (fan, levels, products, workspace rows) of a grouped fold of n rows whose largest
        group has max_group rows. No GPU work."""
        f, lv, pr, ws = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_fold_groups_plan(n, max_group, C.byref(f), C.byref(lv), C.byref(pr), C.byref(ws)),
               "dds_fold_groups_plan")
        return f.value, lv.value, pr.value, ws.value

    @staticmethod
    def scan_plan(n: int) -> tuple:
        """dds_scan_plan: (fan, levels, products, workspace rows) of the running totals of n rows. No GPU work."""
        f, lv, pr, ws = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_scan_plan(n, C.byref(f), C.byref(lv), C.byref(pr), C.byref(ws)), "dds_scan_plan")
        return f.value, lv.value, pr.value, ws.value

    @staticmethod
    def segscan_plan(n: int, seg_starts, suffix: bool = False) -> tuple:
        """dds_segscan_plan: (fan, levels, products, workspace rows) of the segmented running totals of n rows
        whose segments begin at the positions seg_starts; the products are exact for this head pattern. No GPU
        work."""
        st = np.ascontiguousarray(seg_starts, dtype=np.uint64)
        f, lv, pr, ws = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_segscan_plan(n, st.ctypes.data_as(_u64p), len(st), int(bool(suffix)), C.byref(f), C.byref(lv),
                                     C.byref(pr), C.byref(ws)), "dds_segscan_plan")
        return f.value, lv.value, pr.value, ws.value

    @staticmethod
    def window_plan(n: int, w: int) -> tuple:
        """dds_window_plan: (fan, levels, products, workspace rows) of the moving windows of width w over n rows.
        No GPU work."""
        f, lv, pr, ws = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        _check(_lib.dds_window_plan(n, w, C.byref(f), C.byref(lv), C.byref(pr), C.byref(ws)), "dds_window_plan")
        return f.value, lv.value, pr.value, ws.value

    def host_register(self, arr: np.ndarray):
        """dds_host_register: page-lock a reusable output array (results DMA'd straight into it)."""
        _check(_lib.dds_host_register(self._h, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "dds_host_register")

    def host_unregister(self, arr: np.ndarray):
        _check(_lib.dds_host_unregister(self._h, arr.ctypes.data_as(C.c_void_p)), "dds_host_unregister")

    def host_alloc(self, count: int, dtype=np.uint64) -> np.ndarray:
        """dds_host_alloc: an engine-allocated reply array (page-locked, device-mapped, registered).
        Release it with host_free before dropping the engine (the array must not be used after)."""
        dt = np.dtype(dtype)
        p = C.c_void_p()
        _check(_lib.dds_host_alloc(self._h, max(1, count) * dt.itemsize, C.byref(p)), "dds_host_alloc")
        buf = (C.c_uint8 * (max(1, count) * dt.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt, count=max(1, count))

    def host_free(self, arr: np.ndarray):
        _check(_lib.dds_host_free(self._h, arr.ctypes.data_as(C.c_void_p)), "dds_host_free")

    def strtab(self, rows) -> "StrTable":
        """Device-resident string table of the rows' contents (lists of values, str()-ed)."""
        return StrTable(self, rows)

    def column(self, modulus: int, capacity: int) -> "Column":
        return Column(self, modulus, capacity)

    def opecol(self, capacity: int) -> "OpeColumn":
        return OpeColumn(self, capacity)

    def combine_partials_device(self, modulus: int, d_partials: int, rows) -> int:
        """dds_combine_partials_device: partials back to back in device memory (d_partials pointer)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        mb = nbytes(modulus)
        out = (C.c_uint8 * mb)()
        olen = C.c_size_t()
        _check(_lib.dds_combine_partials_device(self._h, int_to_be(modulus, mb), mb, C.c_void_p(d_partials),
                                                rows.ctypes.data_as(_u64p), len(rows), out, mb, C.byref(olen)),
               "dds_combine_partials_device")
        return _be_int(out, olen.value)

    def combine_partials(self, modulus: int, partials: np.ndarray, rows) -> int:
        partials = np.ascontiguousarray(partials, dtype=np.uint32)
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        mb = nbytes(modulus)
        out = (C.c_uint8 * mb)()
        olen = C.c_size_t()
        _check(_lib.dds_combine_partials(self._h, int_to_be(modulus, mb), mb,
                                         partials.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(rows), out, mb,
                                         C.byref(olen)), "dds_combine_partials")
        return _be_int(out, olen.value)


class Column(_Mutable):
    """Device-resident ciphertext column (dds_col)."""
    _pre = "dds_col"

    def __init__(self, eng: Engine, modulus: int, capacity: int):
        self.eng, self.modulus, self.mb = eng, int(modulus), nbytes(modulus)
        h = C.c_void_p()
        _check(_lib.dds_col_create(eng._h, int_to_be(modulus, self.mb), self.mb, capacity, C.byref(h)),
               "dds_col_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.dds_col_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return _lib.dds_col_count(self._h)

    @property
    def partial_words(self) -> int:
        return _lib.dds_col_partial_words(self._h)

    @property
    def digit_rows(self) -> int:
        """dds_col_digit_rows: rows of the base-n digit mirror that are current (0: no mirror in use)."""
        return _lib.dds_col_digit_rows(self._h)

    @property
    def unit_rows(self) -> int:
        """dds_col_unit_rows: rows of the mirror that are in unit form (0: not upgraded, or a non-unit row)."""
        return _lib.dds_col_unit_rows(self._h)

    def append(self, ops):
        ops = [int(x) for x in ops]
        width = max([self.mb] + [nbytes(x) for x in ops])
        _check(_lib.dds_col_append(self._h, ints_to_be(ops, width), width, len(ops)), "dds_col_append")

    def append_dec(self, rows):
        """Append decimal rows (str / bytes, BigInteger.toString text), parsed on the GPU.
        `rows` may also be a (chars: bytes, offsets: uint64 array of len+1) Arrow-style pair."""
        if isinstance(rows, tuple):
            chars, offs = rows
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
            n = len(offs) - 1
            if isinstance(chars, np.ndarray):  # read_dec_buffer's chars: passed by address, no copy
                keep = np.ascontiguousarray(chars, dtype=np.uint8)
                chars = C.cast(C.c_void_p(keep.ctypes.data), C.c_char_p)
        else:
            enc = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
            chars = b"".join(enc)
            offs = np.zeros(len(enc) + 1, dtype=np.uint64)
            np.cumsum([len(e) for e in enc], out=offs[1:])
            n = len(enc)
        _check(_lib.dds_col_append_dec(self._h, chars, offs.ctypes.data_as(C.POINTER(C.c_uint64)), n),
               "dds_col_append_dec")

    def read(self, first: int, count: int) -> list[int]:
        out = (C.c_uint8 * (self.mb * max(1, count)))()
        _check(_lib.dds_col_read(self._h, first, count, out), "dds_col_read")
        raw = bytes(out)
        return [int.from_bytes(raw[i * self.mb:(i + 1) * self.mb], "big") for i in range(count)]

    def read_buffer(self, first: int, count: int) -> np.ndarray:
        """Rows [first, first+count) as canonical big-endian bytes, uint8 [count, modulus bytes]."""
        out = np.empty((max(1, count), self.mb), dtype=np.uint8)
        _check(_lib.dds_col_read(self._h, first, count, out.ctypes.data_as(_u8p)), "dds_col_read")
        return out[:count]

    @property
    def dec_width(self) -> int:
        """dds_col_dec_width: decimal digits of modulus - 1 (no row's text is longer)."""
        return _lib.dds_col_dec_width(self._h)

    def read_dec_buffer(self, first: int, count: int):
        """dds_col_read_dec: rows [first, first+count) as BigInteger.toString text of their canonical
        residues, printed on the GPU: (uint8 chars, uint64 offsets[count+1]), the layout append_dec takes."""
        chars = np.empty(max(1, count * self.dec_width), dtype=np.uint8)
        offs = np.zeros(count + 1, dtype=np.uint64)
        used = C.c_size_t()
        _check(_lib.dds_col_read_dec(self._h, first, count, chars.ctypes.data, chars.nbytes,
                                     offs.ctypes.data_as(_u64p), C.byref(used)), "dds_col_read_dec")
        return chars[:used.value], offs

    def read_dec(self, first: int, count: int) -> list[str]:
        return _split_dec(*self.read_dec_buffer(first, count))

    def fold(self, first: int = 0, count: int | None = None) -> int:
        count = len(self) - first if count is None else count
        out = (C.c_uint8 * (self.mb + 4096))()  # a one-row fold returns the operand, which may be wider
        olen = C.c_size_t()
        _check(_lib.dds_col_fold(self._h, first, count, out, len(out), C.byref(olen)), "dds_col_fold")
        return _be_int(out, olen.value)

    def fold_rows(self, row_ids) -> int:
        """dds_col_fold_rows: SumAll/MultAll over the rows row_ids (a one-row fold returns the operand
        as appended, unreduced)."""
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
        out = (C.c_uint8 * (self.mb + 4096))()
        olen = C.c_size_t()
        _check(_lib.dds_col_fold_rows(self._h, ids.ctypes.data_as(_u64p), len(ids), out, len(out), C.byref(olen)),
               "dds_col_fold_rows")
        return _be_int(out, olen.value)

    def fold_dec(self, row_ids=None, count: int | None = None) -> str:
        """dds_col_fold_dec: the route's decimal reply over row_ids (or rows [0, count))."""
        if row_ids is None:
            ids, n = None, len(self) if count is None else count
        else:
            ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
            n = len(ids)
        cap = 4 * self.mb + 8192
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _check(_lib.dds_col_fold_dec(self._h, None if ids is None else ids.ctypes.data_as(_u64p), n, out, cap,
                                     C.byref(olen)), "dds_col_fold_dec")
        return out.value.decode()

    def append_pow(self, src: "Column", first: int, count: int, exps):
        """dds_col_append_pow: append rows [first, first+count) of src, each raised to its own exponent
        exps[i] < 2^64 (Enc(k_i m_i) for a Paillier column)."""
        e = _u64_array(exps)
        if len(e) != count:
            raise ValueError("one exponent per row")
        _check(_lib.dds_col_append_pow(self._h, src._h, first, count, e.ctypes.data_as(_u64p)), "dds_col_append_pow")

    def append_inv(self, src: "Column", first: int, count: int):
        """dds_col_append_inv: append the inverses of rows [first, first+count) of src (Enc(-m_i) for a Paillier
        column). A row that is not coprime to the modulus: DDSError with .row (relative to first), nothing appended."""
        bad = C.c_size_t(_NO_ROW)
        _check_row(_lib.dds_col_append_inv(self._h, src._h, first, count, C.byref(bad)), "dds_col_append_inv", bad)

    def append_quot(self, num: "Column", num_first: int, den: "Column", den_first: int, count: int):
        """dds_col_append_quot: append num[num_first+i] * den[den_first+i]^-1 (Enc(m_num - m_den) for Paillier
        columns). A den row that is not coprime to the modulus: DDSError with .row, nothing appended."""
        bad = C.c_size_t(_NO_ROW)
        _check_row(_lib.dds_col_append_quot(self._h, num._h, num_first, den._h, den_first, count, C.byref(bad)),
                   "dds_col_append_quot", bad)

    def append_mul(self, a: "Column", a_first: int, b: "Column", b_first: int, count: int):
        """dds_col_append_mul: append a[a_first+i] * b[b_first+i] (Enc(m_a + m_b) for Paillier columns)."""
        _check(_lib.dds_col_append_mul(self._h, a._h, a_first, b._h, b_first, count), "dds_col_append_mul")

    def _weighted_args(self, weights, row_ids, first, count):
        if isinstance(weights, np.ndarray) and weights.dtype == np.int64:
            wts = np.ascontiguousarray(weights)
        else:
            wts = np.ascontiguousarray([int(x) for x in weights], dtype=np.int64)
        if row_ids is None:
            ids, n = None, len(self) - first if count is None else count
        else:
            ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
            n = len(ids)
        if len(wts) != n:
            raise ValueError("one weight per listed row")
        return wts, ids, n

    def fold_weighted(self, weights, row_ids=None, first: int = 0, count: int | None = None, window: int = 0) -> int:
        """dds_col_fold_weighted: prod c_i^(w_i) mod N (Enc(sum w_i m_i) for a Paillier column) over the live
        rows among row_ids (or rows [first, first+count)), signed 64-bit weights, weights[i] for the i-th listed
        row. window: bits of the bucket digits, 1..8 (0: the plan's default); the value does not depend on it."""
        wts, ids, n = self._weighted_args(weights, row_ids, first, count)
        out = (C.c_uint8 * self.mb)()
        olen = C.c_size_t()
        _check(_lib.dds_col_fold_weighted(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                          wts.ctypes.data_as(_i64p), window, out, len(out), C.byref(olen)),
               "dds_col_fold_weighted")
        return _be_int(out, olen.value)

    def fold_weighted_dec(self, weights, row_ids=None, first: int = 0, count: int | None = None,
                          window: int = 0) -> str:
        """dds_col_fold_weighted_dec: the same value as the route's decimal reply."""
        wts, ids, n = self._weighted_args(weights, row_ids, first, count)
        cap = 4 * self.mb + 64
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _check(_lib.dds_col_fold_weighted_dec(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                              wts.ctypes.data_as(_i64p), window, out, cap, C.byref(olen)),
               "dds_col_fold_weighted_dec")
        return out.value.decode()

    def _groups_args(self, groups, ngroups, row_ids, first, count):
        labels = np.ascontiguousarray(groups, dtype=np.uint32)
        if row_ids is None:
            ids, n = None, len(self) - first if count is None else count
        else:
            ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
            n = len(ids)
        if len(labels) != n:
            raise ValueError("one label per listed row")
        return labels, ids, n, np.zeros(max(1, ngroups), dtype=np.uint64)

    def fold_groups(self, groups, ngroups: int, row_ids=None, first: int = 0, count: int | None = None):
        """dds_col_fold_groups_be: the grouped SumAll / MultAll. groups[i] < ngroups labels the i-th listed row
        (row_ids, or rows [first, first+count)); returns (values, counts): values[g] = the product mod N of the
        live rows labelled g as a canonical residue (1 for a group without a live row), counts[g] (uint64) how
        many rows that were."""
        labels, ids, n, counts = self._groups_args(groups, ngroups, row_ids, first, count)
        out = (C.c_uint8 * (self.mb * max(1, ngroups)))()
        _check(_lib.dds_col_fold_groups_be(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                           labels.ctypes.data_as(_u32p), ngroups, out, counts.ctypes.data_as(_u64p)),
               "dds_col_fold_groups_be")
        raw = bytes(out)
        return [int.from_bytes(raw[g * self.mb:(g + 1) * self.mb], "big") for g in range(ngroups)], counts[:ngroups]

    def append_fold_groups(self, src: "Column", groups, ngroups: int, row_ids=None, first: int = 0,
                           count: int | None = None) -> np.ndarray:
        """dds_col_fold_groups: the same values of src's rows appended to this column, group g at the old
        len(self) + g, canonical and live; returns the counts."""
        labels, ids, n, counts = src._groups_args(groups, ngroups, row_ids, first, count)
        _check(_lib.dds_col_fold_groups(src._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                        labels.ctypes.data_as(_u32p), ngroups, self._h,
                                        counts.ctypes.data_as(_u64p)), "dds_col_fold_groups")
        return counts[:ngroups]

    @staticmethod
    def _by_ope(by: "OpeColumn", mask, cap, call):
        """call(mask pointer, mask words, keys, counts, cap, ngroups) -> status, with room for `cap` groups
        (default: up to 4,096); a result with more groups is asked for again at the size the engine reports
        (DDS_E_BUFSIZE wrote nothing). Returns (keys, counts) of the groups."""
        words = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
        cap = max(1, min(len(by), 4096)) if cap is None else cap
        ng = C.c_size_t()
        while True:
            keys, counts = np.empty(max(1, cap), dtype=np.int64), np.empty(max(1, cap), dtype=np.uint64)
            rc = call(None if words is None else words.ctypes.data_as(_u64p), 0 if words is None else len(words),
                      keys.ctypes.data_as(_i64p), counts.ctypes.data_as(_u64p), cap, C.byref(ng))
            if rc != DDS_E_BUFSIZE or ng.value <= cap:
                return rc, keys[:ng.value], counts[:ng.value]
            cap = ng.value

    def fold_by_ope(self, by: "OpeColumn", mask=None, cap: int | None = None):
        """dds_col_fold_by_ope_be: SELECT key, SUM(x) GROUP BY key with the keys in the resident OPE column `by`
        (row r of both columns is the same stored set). mask: uint64 row-mask words as OpeColumn.search_mask
        returns them (a WHERE), or None. Returns (keys, values, counts): the distinct int64 keys of the
        participating rows in ascending order, the product mod N of each key's rows as a canonical residue, and
        how many rows that were."""
        out = None

        def call(m, mw, keys, counts, cap, ng):
            nonlocal out
            out = (C.c_uint8 * (self.mb * max(1, cap)))()
            return _lib.dds_col_fold_by_ope_be(self._h, by._h, m, mw, out, keys, counts, cap, ng)

        rc, keys, counts = self._by_ope(by, mask, cap, call)
        _check(rc, "dds_col_fold_by_ope_be")
        raw = C.string_at(C.addressof(out), self.mb * len(keys))
        return keys, [int.from_bytes(raw[g * self.mb:(g + 1) * self.mb], "big") for g in range(len(keys))], counts

    def append_fold_by_ope(self, src: "Column", by: "OpeColumn", mask=None, cap: int | None = None):
        """dds_col_fold_by_ope: the same values of src's rows appended to this column, group g at the old
        len(self) + g, canonical and live; returns (keys, counts)."""
        rc, keys, counts = self._by_ope(by, mask, cap, lambda m, mw, keys, counts, cap, ng: _lib.dds_col_fold_by_ope(
            src._h, by._h, m, mw, self._h, keys, counts, cap, ng))
        _check(rc, "dds_col_fold_by_ope")
        return keys, counts

    @staticmethod
    def _by_str(tab: "StrTable", mask, cap, call):
        """call(mask pointer, mask words, first_rows, counts, cap, ngroups, passes) -> status, with room for `cap`
        groups (default: up to 4,096); a result with more groups is asked for again at the size the engine reports
        (DDS_E_BUFSIZE wrote nothing). Returns (status, first_rows, counts, passes)."""
        words = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
        cap = max(1, min(tab.nrows, 4096)) if cap is None else cap
        ng, passes = C.c_size_t(), C.c_int()
        while True:
            first, counts = np.empty(max(1, cap), dtype=np.uint64), np.empty(max(1, cap), dtype=np.uint64)
            rc = call(None if words is None else words.ctypes.data_as(_u64p), 0 if words is None else len(words),
                      first.ctypes.data_as(_u64p), counts.ctypes.data_as(_u64p), cap, C.byref(ng), C.byref(passes))
            if rc != DDS_E_BUFSIZE or ng.value <= cap:
                n = ng.value if rc == DDS_OK else 0
                return rc, first[:n], counts[:n], passes.value
            cap = ng.value

    def fold_by_str(self, tab: "StrTable", position: int, mask=None, cap: int | None = None):
        """dds_col_fold_by_str_be: SELECT text, SUM(x) GROUP BY text with the keys in element `position` of the
        resident string table `tab` (row r of the column and of the table is the same stored set). mask: uint64
        row-mask words as OpeColumn.search_mask returns them (a WHERE), or None. Returns (first_rows, values, counts,
        passes): per distinct text in order of first occurrence the smallest participating row id holding it
        (StrTable.read_elems gives the texts), the product mod N of its rows as a canonical residue, how many rows
        that were, and the labelling passes the call ran (1 unless a digest collision was met)."""
        out = None

        def call(m, mw, first, counts, cap, ng, passes):
            nonlocal out
            out = (C.c_uint8 * (self.mb * max(1, cap)))()
            return _lib.dds_col_fold_by_str_be(self._h, tab._h, position, m, mw, out, first, counts, cap, ng, passes)

        rc, first, counts, passes = self._by_str(tab, mask, cap, call)
        _check(rc, "dds_col_fold_by_str_be")
        raw = C.string_at(C.addressof(out), self.mb * len(first))
        vals = [int.from_bytes(raw[g * self.mb:(g + 1) * self.mb], "big") for g in range(len(first))]
        return first, vals, counts, passes

    def append_fold_by_str(self, src: "Column", tab: "StrTable", position: int, mask=None, cap: int | None = None):
        """dds_col_fold_by_str: the same values of src's rows appended to this column, group g at the old
        len(self) + g, canonical and live; returns (first_rows, counts, passes)."""
        rc, first, counts, passes = self._by_str(tab, mask, cap, lambda m, mw, first, counts, cap, ng, passes:
                                                 _lib.dds_col_fold_by_str(src._h, tab._h, position, m, mw, self._h,
                                                                          first, counts, cap, ng, passes))
        _check(rc, "dds_col_fold_by_str")
        return first, counts, passes

    def _scan_args(self, row_ids, first, count):
        if row_ids is None:
            return None, len(self) - first if count is None else count
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
        return ids, len(ids)

    def append_scan(self, src: "Column", row_ids=None, first: int = 0, count: int | None = None,
                    suffix: bool = False):
        """dds_col_append_scan: append the running totals of src's rows row_ids (or [first, first+count)), taken in
        order: row j = x_0 * ... * x_j mod N (Enc(m_0 + ... + m_j) for a Paillier column), with suffix
        x_j * ... * x_(n-1); canonical and live, row j at the old len(self) + j. Positional: liveness is ignored."""
        ids, n = src._scan_args(row_ids, first, count)
        _check(_lib.dds_col_append_scan(self._h, src._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                        int(bool(suffix))), "dds_col_append_scan")

    def scan(self, row_ids=None, first: int = 0, count: int | None = None, suffix: bool = False) -> list:
        """dds_col_scan_be: the same running totals as a list of canonical residues."""
        ids, n = self._scan_args(row_ids, first, count)
        out = (C.c_uint8 * (self.mb * max(1, n)))()
        _check(_lib.dds_col_scan_be(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                    int(bool(suffix)), out), "dds_col_scan_be")
        raw = C.string_at(C.addressof(out), self.mb * n)
        return [int.from_bytes(raw[j * self.mb:(j + 1) * self.mb], "big") for j in range(n)]

    def scan_by_ope(self, by: "OpeColumn", mask=None, cap: int | None = None, suffix: bool = False):
        """dds_col_scan_by_ope_be: SELECT key, SUM(x) OVER (ORDER BY key) with the keys in the resident OPE column
        `by`; participation and mask as fold_by_ope. Returns (keys, values, counts): the distinct keys in
        ascending order, for each the product mod N of the participating rows with key <= it (suffix: >= it) as
        a canonical residue, and how many rows that were."""
        out = None

        def call(m, mw, keys, counts, cap, ng):
            nonlocal out
            out = (C.c_uint8 * (self.mb * max(1, cap)))()
            return _lib.dds_col_scan_by_ope_be(self._h, by._h, m, mw, int(bool(suffix)), out, keys, counts, cap, ng)

        rc, keys, counts = self._by_ope(by, mask, cap, call)
        _check(rc, "dds_col_scan_by_ope_be")
        raw = C.string_at(C.addressof(out), self.mb * len(keys))
        return keys, [int.from_bytes(raw[g * self.mb:(g + 1) * self.mb], "big") for g in range(len(keys))], counts

    def append_scan_by_ope(self, col: "Column", by: "OpeColumn", mask=None, suffix: bool = False):
        """dds_col_scan_by_ope: the same cumulative values of col's rows appended to this column, key g at the old
        len(self) + g, canonical and live; returns (keys, counts)."""
        rc, keys, counts = self._by_ope(by, mask, None, lambda m, mw, keys, counts, cap, ng: _lib.dds_col_scan_by_ope(
            col._h, by._h, m, mw, int(bool(suffix)), self._h, keys, counts, cap, ng))
        _check(rc, "dds_col_scan_by_ope")
        return keys, counts

    def _rows_of(self, out, n):
        raw = C.string_at(C.addressof(out), self.mb * n)
        return [int.from_bytes(raw[j * self.mb:(j + 1) * self.mb], "big") for j in range(n)]

    def append_scan_seg(self, src: "Column", seg_starts, row_ids=None, first: int = 0, count: int | None = None,
                        suffix: bool = False):
        """dds_col_append_scan_seg: append the running totals of src's rows, restarting at every position of
        seg_starts (positions in the call's order, the first 0, strictly ascending): row j = the product of the
        rows from its segment's start through j, with suffix from j through its segment's last row."""
        ids, n = src._scan_args(row_ids, first, count)
        st = np.ascontiguousarray(seg_starts, dtype=np.uint64)
        _check(_lib.dds_col_append_scan_seg(self._h, src._h, None if ids is None else ids.ctypes.data_as(_u64p), first,
                                            n, st.ctypes.data_as(_u64p), len(st), int(bool(suffix))),
               "dds_col_append_scan_seg")

    def scan_seg(self, seg_starts, row_ids=None, first: int = 0, count: int | None = None,
                 suffix: bool = False) -> list:
        """dds_col_scan_seg_be: the same segmented running totals as a list of canonical residues."""
        ids, n = self._scan_args(row_ids, first, count)
        st = np.ascontiguousarray(seg_starts, dtype=np.uint64)
        out = (C.c_uint8 * (self.mb * max(1, n)))()
        _check(_lib.dds_col_scan_seg_be(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n,
                                        st.ctypes.data_as(_u64p), len(st), int(bool(suffix)), out),
               "dds_col_scan_seg_be")
        return self._rows_of(out, n)

    def append_window(self, src: "Column", w: int, row_ids=None, first: int = 0, count: int | None = None):
        """dds_col_append_window: append the moving windows of width w over src's rows: row j = the product of the
        rows max(0, j - w + 1) .. j. No inverse is taken: zero rows and non-units are served."""
        ids, n = src._scan_args(row_ids, first, count)
        _check(_lib.dds_col_append_window(self._h, src._h, None if ids is None else ids.ctypes.data_as(_u64p), first,
                                          n, w), "dds_col_append_window")

    def window(self, w: int, row_ids=None, first: int = 0, count: int | None = None) -> list:
        """dds_col_window_be: the same moving windows as a list of canonical residues."""
        ids, n = self._scan_args(row_ids, first, count)
        out = (C.c_uint8 * (self.mb * max(1, n)))()
        _check(_lib.dds_col_window_be(self._h, None if ids is None else ids.ctypes.data_as(_u64p), first, n, w, out),
               "dds_col_window_be")
        return self._rows_of(out, n)

    @staticmethod
    def _part_by_ope(by: "OpeColumn", mask, call):
        """call(mask pointer, mask words, rows, cap_rows, keys, counts, cap_groups, nrows, ngroups) -> status, with
        room for every row of `by` and up to 4,096 groups; more groups are asked for again at the size the engine
        reports (DDS_E_BUFSIZE wrote nothing). Returns (status, rows, keys, counts)."""
        words = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint64)
        cap_rows, cap_groups = max(1, len(by)), max(1, min(len(by), 4096))
        nr, ng = C.c_size_t(), C.c_size_t()
        while True:
            rows = np.empty(cap_rows, dtype=np.uint64)
            keys, counts = np.empty(cap_groups, dtype=np.int64), np.empty(cap_groups, dtype=np.uint64)
            rc = call(None if words is None else words.ctypes.data_as(_u64p), 0 if words is None else len(words),
                      rows.ctypes.data_as(_u64p), cap_rows, keys.ctypes.data_as(_i64p), counts.ctypes.data_as(_u64p),
                      cap_groups, C.byref(nr), C.byref(ng))
            if rc != DDS_E_BUFSIZE or (ng.value <= cap_groups and nr.value <= cap_rows):
                return rc, rows[:nr.value], keys[:ng.value], counts[:ng.value]
            cap_rows, cap_groups = max(cap_rows, nr.value), max(cap_groups, ng.value)

    def scan_part_by_ope(self, by: "OpeColumn", mask=None, suffix: bool = False):
        """dds_col_scan_part_by_ope_be: SELECT row, SUM(x) OVER (PARTITION BY key ORDER BY row) with the keys in
        the resident OPE column `by`; participation and mask as fold_by_ope. Returns (rows, values, keys, counts):
        slot t is the t-th participating row in (key, row id) order, rows[t] its id, values[t] the product mod N
        of the participating rows of its key with row id <= it (suffix: >= it); keys ascending, counts[g] the rows
        of key g, whose slots start at counts[:g].sum()."""
        out = None

        def call(m, mw, rows, cap_rows, keys, counts, cap_groups, nr, ng):
            nonlocal out
            out = (C.c_uint8 * (self.mb * cap_rows))()
            return _lib.dds_col_scan_part_by_ope_be(self._h, by._h, m, mw, int(bool(suffix)), out, rows, cap_rows, keys,
                                                    counts, cap_groups, nr, ng)

        rc, rows, keys, counts = self._part_by_ope(by, mask, call)
        _check(rc, "dds_col_scan_part_by_ope_be")
        return rows, self._rows_of(out, len(rows)), keys, counts

    def append_scan_part_by_ope(self, col: "Column", by: "OpeColumn", mask=None, suffix: bool = False):
        """dds_col_scan_part_by_ope: the same values of col's rows appended to this column, slot t at the old
        len(self) + t, canonical and live; returns (rows, keys, counts)."""
        rc, rows, keys, counts = self._part_by_ope(
            by, mask, lambda m, mw, rows, cap_rows, keys, counts, cap_groups, nr, ng: _lib.dds_col_scan_part_by_ope(
                col._h, by._h, m, mw, int(bool(suffix)), self._h, rows, cap_rows, keys, counts, cap_groups, nr, ng))
        _check(rc, "dds_col_scan_part_by_ope")
        return rows, keys, counts

    def fold_partial_device(self, d_partial: int, first: int = 0, count: int | None = None):
        """dds_col_fold_partial_device: the partial (partial_words u32) into device memory at d_partial."""
        count = len(self) - first if count is None else count
        _check(_lib.dds_col_fold_partial_device(self._h, first, count, C.c_void_p(d_partial)),
               "dds_col_fold_partial_device")

    def fold_partial(self, first: int = 0, count: int | None = None):
        count = len(self) - first if count is None else count
        part = np.zeros(self.partial_words, dtype=np.uint32)
        rows = C.c_uint64()
        _check(_lib.dds_col_fold_partial(self._h, first, count, part.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         C.byref(rows)), "dds_col_fold_partial")
        return part, rows.value

    def fill_paillier_synth(self, n: int, g: int, seed: int, row0: int, count: int, pool: int = 1024):
        _check(_lib.dds_col_fill_paillier_synth(self._h, int_to_be(n, nbytes(n)), nbytes(n), int_to_be(g, nbytes(g)),
                                                nbytes(g), seed, row0, count, pool), "dds_col_fill_paillier_synth")


    def truncate(self, count: int = 0):
        _check(_lib.dds_col_truncate(self._h, count), "dds_col_truncate")

    def fill_table_synth(self, table, seed: int, row0: int, count: int):
        """Append rows table[h_i % len(table)] (dds_col_fill_table_synth); see synth_indices."""
        table = [int(x) for x in table]
        _check(_lib.dds_col_fill_table_synth(self._h, ints_to_be(table, self.mb), self.mb, len(table), seed, row0,
                                             count), "dds_col_fill_table_synth")

    def fill_random(self, bits: int, seed: int, row0: int, count: int):
        """Append seeded odd random rows < 2^bits (dds_col_fill_random)."""
        _check(_lib.dds_col_fill_random(self._h, bits, seed, row0, count), "dds_col_fill_random")

    def encrypt_paillier(self, rcol: "Column", r_first: int, d_m: int, count: int, n: int, g: int,
                         p: int | None = None, q: int | None = None):
        """Append Enc(m_i; r_i) for rows [r_first, r_first+count) of rcol; d_m: device uint32 pointer."""
        pb = int_to_be(p, nbytes(p)) if p else None
        qb = int_to_be(q, nbytes(q)) if q else None
        _check(_lib.dds_col_encrypt_paillier(self._h, rcol._h, r_first, C.c_void_p(d_m), count,
                                             int_to_be(n, nbytes(n)), nbytes(n), int_to_be(g, nbytes(g)), nbytes(g),
                                             pb, nbytes(p) if p else 0, qb, nbytes(q) if q else 0),
               "dds_col_encrypt_paillier")

    def decrypt_paillier_buffer(self, first: int, count: int, p: int, q: int, g: int,
                                n_bytes: int | None = None) -> np.ndarray:
        """HomoAdd.decrypt of rows [first, first+count) of a column over (p*q)^2 (dds_col_decrypt_paillier):
        big-endian plaintexts, uint8 [count, n_bytes] (n_bytes defaults to the byte length of n)."""
        nb = nbytes(p * q) if n_bytes is None else n_bytes
        out = np.empty((max(1, count), max(1, nb)), dtype=np.uint8)
        _check(_lib.dds_col_decrypt_paillier(self._h, first, count, int_to_be(p, nbytes(p)), nbytes(p),
                                             int_to_be(q, nbytes(q)), nbytes(q), int_to_be(g, nbytes(g)), nbytes(g),
                                             out.ctypes.data_as(_u8p), nb), "dds_col_decrypt_paillier")
        return out[:count]

    def decrypt_paillier(self, first: int, count: int, p: int, q: int, g: int) -> list[int]:
        return [int.from_bytes(r.tobytes(), "big") for r in self.decrypt_paillier_buffer(first, count, p, q, g)]

    def decrypt_rsa_buffer(self, first: int, count: int, p: int, q: int, d: int,
                           n_bytes: int | None = None) -> np.ndarray:
        """HomoMult.decrypt of rows [first, first+count) of a column over p*q (dds_col_decrypt_rsa): big-endian
        values c^d mod p*q, uint8 [count, n_bytes] (n_bytes defaults to the byte length of p*q)."""
        nb = nbytes(p * q) if n_bytes is None else n_bytes
        out = np.empty((max(1, count), max(1, nb)), dtype=np.uint8)
        _check(_lib.dds_col_decrypt_rsa(self._h, first, count, int_to_be(p, nbytes(p)), nbytes(p),
                                        int_to_be(q, nbytes(q)), nbytes(q), int_to_be(d, nbytes(d)), nbytes(d),
                                        out.ctypes.data_as(_u8p), nb), "dds_col_decrypt_rsa")
        return out[:count]

    def decrypt_rsa(self, first: int, count: int, p: int, q: int, d: int) -> list[int]:
        return [int.from_bytes(r.tobytes(), "big") for r in self.decrypt_rsa_buffer(first, count, p, q, d)]


OPE_CLS_LACKS, OPE_CLS_LAST, OPE_CLS_INNER = 0, 1, 2


class OpeColumn:
    """Resident OPE column (dds_opecol): Search{Gt,GtEq,Lt,LtEq} and OrderLS/OrderSL over it."""

    def __init__(self, eng: Engine, capacity: int):
        self.eng = eng
        h = C.c_void_p()
        _check(_lib.dds_opecol_create(eng._h, capacity, C.byref(h)), "dds_opecol_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.dds_opecol_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return _lib.dds_opecol_count(self._h)

    def truncate(self, count: int = 0):
        _check(_lib.dds_opecol_truncate(self._h, count), "dds_opecol_truncate")

    def append(self, values, cls=None):
        v = np.ascontiguousarray(values, dtype=np.int64)
        c = None if cls is None else np.ascontiguousarray(cls, dtype=np.uint8)
        _check(_lib.dds_opecol_append(self._h, v.ctypes.data_as(C.c_void_p),
                                      None if c is None else c.ctypes.data_as(C.c_void_p), len(v)),
               "dds_opecol_append")

    def append_dec(self, values, cls=None, is_string=None):
        """values: element texts (str, or None where the row lacks the position)."""
        n = len(values)
        arr = (C.c_char_p * max(1, n))(*[None if v is None else str(v).encode() for v in values])
        c = None if cls is None else np.ascontiguousarray(cls, dtype=np.uint8)
        st = None if is_string is None else np.ascontiguousarray(is_string, dtype=np.uint8)
        _check(_lib.dds_opecol_append_dec(self._h, arr, None if c is None else c.ctypes.data_as(C.c_void_p),
                                          None if st is None else st.ctypes.data_as(C.c_void_p), n),
               "dds_opecol_append_dec")

    def search(self, bound, op: str, out: np.ndarray | None = None) -> np.ndarray:
        """dds_opecol_search: matching row ids in row order. out: a reusable uint32 buffer of at least
        len(self) entries (Engine.host_register it once to have the ids DMA'd straight in); the result is
        then a view of it."""
        buf = np.empty(max(1, len(self)), dtype=np.uint32) if out is None else out
        if len(buf) < len(self):
            raise ValueError("out holds fewer entries than the column's rows")
        got = C.c_size_t()
        _check(_lib.dds_opecol_search(self._h, None if bound is None else str(bound).encode(), OPE_OPS[op],
                                      buf.ctypes.data_as(C.c_void_p), C.byref(got)), "dds_opecol_search")
        return buf[: got.value] if out is not None else buf[: got.value].copy()

    def search_mask(self, bound, op: str, out: np.ndarray | None = None):
        """dds_opecol_search_mask: (uint64 words, bit r%64 of word r/64 = row r matches; match count).
        out: a reusable uint64 buffer of at least ceil(rows / 64) words (Engine.host_register it once to
        have the mask DMA'd straight in)."""
        words = np.zeros(max(1, (len(self) + 63) // 64), dtype=np.uint64) if out is None else out
        got = C.c_size_t()
        _check(_lib.dds_opecol_search_mask(self._h, None if bound is None else str(bound).encode(), OPE_OPS[op],
                                           words.ctypes.data_as(C.c_void_p), len(words), C.byref(got)),
               "dds_opecol_search_mask")
        return words, got.value

    def order(self, descending: bool, out: np.ndarray | None = None) -> np.ndarray:
        """dds_opecol_order: the live rows' permutation. out: a reusable uint32 buffer of at least
        len(self) entries (Engine.host_register it once to have the ids DMA'd straight in); the result
        is then a view of it."""
        buf = np.empty(max(1, len(self)), dtype=np.uint32) if out is None else out
        got = C.c_size_t()
        _check(_lib.dds_opecol_order(self._h, int(descending), buf.ctypes.data_as(C.c_void_p), C.byref(got)),
               "dds_opecol_order")
        return buf[: got.value] if out is not None else buf[: got.value].copy()

    def write_rows(self, row_ids, values, cls=None):
        ids = _ids(row_ids)
        v = np.ascontiguousarray(values, dtype=np.int64)
        c = None if cls is None else np.ascontiguousarray(cls, dtype=np.uint8)
        _check(_lib.dds_opecol_write_rows(self._h, ids.ctypes.data, v.ctypes.data,
                                          None if c is None else c.ctypes.data, len(ids)), "dds_opecol_write_rows")

    def write_rows_dec(self, row_ids, values, cls=None, is_string=None):
        ids = _ids(row_ids)
        n = len(ids)
        arr = (C.c_char_p * max(1, n))(*[None if v is None else str(v).encode() for v in values])
        c = None if cls is None else np.ascontiguousarray(cls, dtype=np.uint8)
        st = None if is_string is None else np.ascontiguousarray(is_string, dtype=np.uint8)
        _check(_lib.dds_opecol_write_rows_dec(self._h, ids.ctypes.data, arr, None if c is None else c.ctypes.data,
                                              None if st is None else st.ctypes.data, n), "dds_opecol_write_rows_dec")

    def set_live(self, row_ids, live):
        ids = _ids(row_ids)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(live, dtype=np.uint8), ids.shape))
        _check(_lib.dds_opecol_set_live(self._h, ids.ctypes.data, len(ids), flags.ctypes.data), "dds_opecol_set_live")

    @property
    def live_count(self) -> int:
        return _lib.dds_opecol_live_count(self._h)


class MultiEngine:
    """dds_mctx: one caller driving several GPUs (devices may repeat: several shards on one GPU)."""

    def __init__(self, devices=None, mask: int | None = None):
        h = C.c_void_p()
        if mask is not None:
            _check(_lib.dds_mctx_create(int(mask), C.byref(h)), "dds_mctx_create")
        else:
            devs = (C.c_int * len(devices))(*devices)
            _check(_lib.dds_mctx_create_devices(devs, len(devices), C.byref(h)), "dds_mctx_create_devices")
        self._h = h

    @property
    def shards(self) -> int:
        return _lib.dds_mctx_shards(self._h)

    def close(self):
        if self._h:
            _lib.dds_mctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def column(self, modulus: int, capacity: int) -> "MColumn":
        return MColumn(self, modulus, capacity)


class MColumn(_Mutable):
    """dds_mcol: a column sharded over the devices of a MultiEngine (64-row blocks, round-robin)."""
    _pre = "dds_mcol"

    def __init__(self, m: MultiEngine, modulus: int, capacity: int):
        self.m, self.modulus, self.mb = m, int(modulus), nbytes(modulus)
        h = C.c_void_p()
        _check(_lib.dds_mcol_create(m._h, int_to_be(modulus, self.mb), self.mb, capacity, C.byref(h)),
               "dds_mcol_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.dds_mcol_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return _lib.dds_mcol_count(self._h)

    def append(self, ops):
        ops = [int(x) for x in ops]
        width = max([self.mb] + [nbytes(x) for x in ops])
        buf = ints_to_be(ops, width)
        _check(_lib.dds_mcol_append(self._h, buf, width, len(ops)), "dds_mcol_append")

    def append_buffer(self, buf: np.ndarray):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _check(_lib.dds_mcol_append(self._h, buf.ctypes.data, buf.shape[1], buf.shape[0]), "dds_mcol_append")

    def append_dec(self, rows):
        enc = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
        chars = b"".join(enc)
        offs = np.zeros(len(enc) + 1, dtype=np.uint64)
        np.cumsum([len(e) for e in enc], out=offs[1:])
        _check(_lib.dds_mcol_append_dec(self._h, chars, offs.ctypes.data_as(_u64p), len(enc)), "dds_mcol_append_dec")

    def fill_paillier_synth(self, n: int, g: int, seed: int, count: int, pool: int = 1024):
        _check(_lib.dds_mcol_fill_paillier_synth(self._h, int_to_be(n, nbytes(n)), nbytes(n), int_to_be(g, nbytes(g)),
                                                 nbytes(g), seed, count, pool), "dds_mcol_fill_paillier_synth")

    def fold(self) -> int:
        out = (C.c_uint8 * (self.mb + 4096))()
        olen = C.c_size_t()
        _check(_lib.dds_mcol_fold(self._h, out, len(out), C.byref(olen)), "dds_mcol_fold")
        return _be_int(out, olen.value)

    def fold_rows(self, row_ids) -> int:
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64)
        out = (C.c_uint8 * (self.mb + 4096))()
        olen = C.c_size_t()
        _check(_lib.dds_mcol_fold_rows(self._h, ids.ctypes.data_as(_u64p), len(ids), out, len(out), C.byref(olen)),
               "dds_mcol_fold_rows")
        return _be_int(out, olen.value)

    def fold_dec(self, row_ids=None) -> str:
        ids = None if row_ids is None else np.ascontiguousarray(row_ids, dtype=np.uint64)
        cap = 4 * self.mb + 8192
        out = C.create_string_buffer(cap)
        olen = C.c_size_t()
        _check(_lib.dds_mcol_fold_dec(self._h, None if ids is None else ids.ctypes.data_as(_u64p),
                                      0 if ids is None else len(ids), out, cap, C.byref(olen)), "dds_mcol_fold_dec")
        return out.value.decode()


def element_text(v) -> str:
    """``toString`` of a DDSSet element as AnyJsonFormat reads it (DDSJsonProtocol.scala:22-28): String as
    is, Int in decimal, Boolean ``true``/``false``, JsNull ``None`` (the text HomoDet.compare sees)."""
    if v is None:
        return "None"
    if isinstance(v, bool):
        return "true" if v else "false"
    return str(v)


def _flatten(rows):
    """(chars, elem_off, row_off) of rows (lists of elements) in the dds_strtab batch layout"""
    enc = [[element_text(v).encode() for v in row] for row in rows]
    lens = np.fromiter((len(x) for row in enc for x in row), dtype=np.uint64)
    elem_off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=elem_off[1:])
    row_off = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(r) for r in enc), dtype=np.uint64, count=len(enc)), out=row_off[1:])
    return b"".join(x for row in enc for x in row), elem_off, row_off


STRTAB_STATS = ("rows", "live", "heap_elems", "elems", "heap_bytes", "bytes", "compactions", "pos_indexes")


class StrTable:
    """Device-resident contents of DDSSet rows for the deterministic-equality scans (dds_strtab); follows
    the write routes in place (append / write_rows / set_live)."""

    def __init__(self, eng: Engine, rows=None, *, chars: bytes | None = None, elem_off=None, row_off=None):
        if rows is not None:
            chars, elem_off, row_off = _flatten(rows)
        elem_off = np.ascontiguousarray(elem_off, dtype=np.uint64)
        row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
        h = C.c_void_p()
        _check(_lib.dds_strtab_create(eng._h, C.c_char_p(chars or b"\0"), elem_off.ctypes.data_as(C.c_void_p),
                                      len(elem_off) - 1, row_off.ctypes.data_as(C.c_void_p), len(row_off) - 1,
                                      C.byref(h)), "dds_strtab_create")
        self._h = h
        self._tls = threading.local()  # per-thread reply buffer of the scans (reused across calls)

    @property
    def nrows(self) -> int:
        return _lib.dds_strtab_rows(self._h)

    def _reply(self) -> np.ndarray:
        # sized with slack: rows another thread appends between this read and the scan fit too
        n = max(1, self.nrows)
        buf = getattr(self._tls, "buf", None)
        if buf is None or len(buf) < n + n // 8 + 1024:
            buf = self._tls.buf = np.empty(n + n // 4 + 1024, dtype=np.uint32)
        return buf

    def live_count(self) -> int:
        return _lib.dds_strtab_live_count(self._h)

    def stats(self) -> dict:
        out = np.zeros(len(STRTAB_STATS), dtype=np.uint64)
        _check(_lib.dds_strtab_stats(self._h, out.ctypes.data_as(C.c_void_p), len(out)), "dds_strtab_stats")
        return dict(zip(STRTAB_STATS, (int(x) for x in out)))

    def append(self, rows):
        self.append_flat(*_flatten(rows))

    def append_flat(self, chars: bytes, elem_off, row_off):
        """dds_strtab_append on a batch already in the table layout"""
        eo = np.ascontiguousarray(elem_off, dtype=np.uint64)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        _check(_lib.dds_strtab_append(self._h, C.c_char_p(chars or b"\0"), eo.ctypes.data_as(C.c_void_p), len(eo) - 1,
                                      ro.ctypes.data_as(C.c_void_p), len(ro) - 1), "dds_strtab_append")

    def write_rows(self, ids, rows):
        self.write_rows_flat(ids, *_flatten(rows))

    def write_rows_flat(self, ids, chars: bytes, elem_off, row_off):
        """dds_strtab_write_rows on a batch already in the table layout (one batch row per id)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        eo = np.ascontiguousarray(elem_off, dtype=np.uint64)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        if len(ro) - 1 != len(ids):
            raise ValueError("one row per id")
        _check(_lib.dds_strtab_write_rows(self._h, ids.ctypes.data_as(C.c_void_p), len(ids), C.c_char_p(chars or b"\0"),
                                          eo.ctypes.data_as(C.c_void_p), len(eo) - 1, ro.ctypes.data_as(C.c_void_p)),
               "dds_strtab_write_rows")

    def truncate(self, rows: int = 0):
        _check(_lib.dds_strtab_truncate(self._h, rows), "dds_strtab_truncate")

    def set_live(self, ids, live):
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        lv = np.broadcast_to(np.asarray(live, dtype=np.uint8), ids.shape).copy()
        _check(_lib.dds_strtab_set_live(self._h, ids.ctypes.data_as(C.c_void_p), len(ids), lv.ctypes.data_as(C.c_void_p)),
               "dds_strtab_set_live")

    def close(self):
        if self._h:
            _lib.dds_strtab_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read_elems(self, rows, position: int) -> list:
        """dds_strtab_read_elems: the text of element `position` of the listed rows (ids may repeat) as bytes, None
        for a row that is dead or lacks the position."""
        ids = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(ids)
        offs, pres, need = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint8), C.c_size_t()
        cap = max(64, 32 * n)
        while True:
            buf = C.create_string_buffer(cap)
            rc = _lib.dds_strtab_read_elems(self._h, ids.ctypes.data_as(_u64p), n, position, buf, cap,
                                            offs.ctypes.data_as(_u64p), pres.ctypes.data_as(_u8p), C.byref(need))
            if rc != DDS_E_BUFSIZE or need.value <= cap:
                break
            cap = need.value
        _check(rc, "dds_strtab_read_elems")
        raw = buf.raw
        return [raw[int(offs[i]):int(offs[i + 1])] if pres[i] else None for i in range(n)]

    def search_eq(self, position: int, value, negate: bool = False) -> np.ndarray:
        v = element_text(value).encode()
        out = self._reply()
        n = C.c_size_t()
        _check(_lib.dds_search_eq(self._h, position, v, len(v), int(negate), out.ctypes.data_as(C.c_void_p),
                                  C.byref(n)), "dds_search_eq")
        return out[: n.value].copy()

    def search_entry(self, values, require_all: bool = False) -> np.ndarray:
        vs = [element_text(v).encode() for v in values]
        arr = (C.c_char_p * len(vs))(*vs)
        lens = (C.c_size_t * len(vs))(*[len(v) for v in vs])
        out = self._reply()
        n = C.c_size_t()
        _check(_lib.dds_search_entry(self._h, arr, lens, len(vs), int(require_all), out.ctypes.data_as(C.c_void_p),
                                     C.byref(n)), "dds_search_entry")
        return out[: n.value].copy()

    def is_element(self, row: int, value) -> bool:
        v = element_text(value).encode()
        f = C.c_int()
        _check(_lib.dds_is_element(self._h, row, v, len(v), C.byref(f)), "dds_is_element")
        return bool(f.value)


# ---- synthetic-row plaintexts (mirror of k_synth_rows' index derivation) ----
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def synth_indices(seed: int, row0: int, count: int, modulo: int, chunk: int = 1 << 22) -> np.ndarray:
    """splitmix64(seed ^ splitmix64(row)) % modulo for rows [row0, row0+count) (uint32): the index
    derivation of k_synth_rows / k_gather_rows."""
    out = np.empty(count, dtype=np.uint32)
    for s in range(0, count, chunk):
        idx = np.arange(row0 + s, row0 + min(count, s + chunk), dtype=np.uint64)
        h = _splitmix64_np(np.uint64(seed) ^ _splitmix64_np(idx))
        out[s:s + len(idx)] = (h % np.uint64(modulo)).astype(np.uint32)
    return out


def synth_plaintexts(seed: int, row0: int, count: int, chunk: int = 1 << 22) -> np.ndarray:
    """m_i of dds_col_fill_paillier_synth rows [row0, row0+count) (uint32)."""
    return synth_indices(seed, row0, count, 10000, chunk)
