"""ctypes binding of libfreud_sae.so (C ABI: include/freud_sae.h).

This is the only door between the Python host (orchestration, torch for device memory,
streams and torch.distributed) and the HIP engine that runs the SAE train step
(reference hot path: src/scripts/train_sae.py:421-453).  There is no CPU fallback: if the
shared library is missing the import of this module's `load()` fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from typing import Dict, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FREUD_SAE_LIB: development override (A/B timing of two builds of the engine on one GPU box)
LIB_PATH = os.environ.get("FREUD_SAE_LIB") or os.path.join(_HERE, "lib", "libfreud_sae.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

VARIANT = {"l1": 0, "topk": 1}
OPTIMIZER = {"radam": 0, "adam": 1}
DTYPE = {"float32": 0, "float16": 1, "bfloat16": 2}
PRECISION = {"bf16": 0, "fp8": 1, "fp8bwd": 2}      # fp8bwd: fp8 encoder / decoder AND dpre GEMMs (include/freud_sae.h)
NUM_METRICS = 8
M_LOSS_RECON, M_LOSS_L1, M_MSE, M_GRAD_NORM, M_COUNT, M_DEAD_PCT, M_MULTI_TOPK_FVU = 0, 1, 2, 3, 4, 5, 6


class SaeConfig(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("d_model", C.c_int32), ("n_dict", C.c_int32), ("k", C.c_int32),
        ("optimizer", C.c_int32), ("device_id", C.c_int32), ("max_rows", C.c_int64),
        ("recon_alpha", C.c_double), ("auxk_alpha", C.c_double), ("clip_thresh", C.c_double),
        ("weight_decay", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("force_generic", C.c_int32), ("debug_flags", C.c_int32), ("force_gemm128", C.c_int32),
        ("topk_dense_backward", C.c_int32), ("multi_topk", C.c_int32), ("precision", C.c_int32),
        ("reserved", C.c_int32 * 2),
    ]


class EngineError(RuntimeError):
    pass


_lib = None


def build(force: bool = False) -> str:
    """Compile the HIP engine for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    # one compile job per translation unit (csrc/Makefile: SRCS)
    jobs = os.environ.get("MAX_JOBS") or str(min(16, os.cpu_count() or 1))
    done = subprocess.run(["make", "-C", CSRC_DIR, "-j", jobs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if done.returncode != 0:
        sys.stderr.write(done.stdout)
        raise EngineError(f"`make -C {CSRC_DIR} -j {jobs}` failed with status {done.returncode}: the compiler's output is above")
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"build did not produce {LIB_PATH}")
    return LIB_PATH


GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)   # sae_grad_ready_fn


# Every entry point of include/freud_sae.h, once: name -> (restype, argtypes).  load() declares them, EXPORTED_SYMBOLS lists them.
_vp, _i32, _i64, _dbl, _fptr = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER(C.c_float)
_SIGNATURES = {
    "sae_last_error": (C.c_char_p, []),
    "sae_version": (C.c_int, []),
    "sae_create": (C.c_int, [C.POINTER(SaeConfig), C.POINTER(_vp)]),
    "sae_destroy": (None, [_vp]),
    "sae_set_params": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "sae_get_params": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "sae_set_opt_state": (C.c_int, [_vp, _i64, C.POINTER(_vp), C.POINTER(_vp), C.c_int]),
    "sae_get_opt_state": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_vp), C.c_int]),
    "sae_forward_backward": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp]),
    "sae_grad_buffer": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "sae_optimizer_step": (C.c_int, [_vp, _dbl, _dbl, _vp]),
    "sae_batch_stats": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp]),
    "sae_stats_buffer": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "sae_set_dp_world": (C.c_int, [_vp, C.c_int]),
    "sae_dist_unique_id": (C.c_int, [_vp, _i64]),
    "sae_dist_init": (C.c_int, [_vp, _vp, _i64, C.c_int, C.c_int]),
    "sae_dist_world": (C.c_int, [_vp]),
    "sae_dist_set_payload": (C.c_int, [_vp, C.c_int]),
    "sae_p2p_blob_bytes": (C.c_int, []),
    "sae_p2p_export": (C.c_int, [_vp, _vp, _i64]),
    "sae_p2p_init": (C.c_int, [_vp, _vp, _i64, C.c_int, C.c_int]),
    "sae_p2p_leave": (C.c_int, [_vp]),
    "sae_dist_set_overlap": (C.c_int, [_vp, C.c_int]),
    "sae_dist_check": (C.c_int, [_vp]),
    "sae_dist_poll": (C.c_int, [_vp]),
    "sae_dist_audit": (C.c_int, [_vp, _vp]),
    "sae_grad_layout": (C.c_int, [_vp, C.POINTER(_i64)]),
    "sae_param_checksum": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "sae_set_grad_ready_callback": (C.c_int, [_vp, GRAD_READY_FN, _vp]),
    "sae_get_topk_state": (C.c_int, [_vp, C.POINTER(C.c_int64), _i64]),
    "sae_set_topk_state": (C.c_int, [_vp, C.POINTER(C.c_int64), _i64]),
    "sae_set_topk_options": (C.c_int, [_vp, _dbl, _i64]),
    "sae_set_decoder_constraint": (C.c_int, [_vp, C.c_int]),
    "sae_get_decoder_constraint": (C.c_int, [_vp]),
    "sae_step": (C.c_int, [_vp, _vp, _i64, C.c_int, _dbl, _vp]),
    "sae_eval": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp]),
    "sae_eval_into": (C.c_int, [_vp, _vp, _i64, C.c_int, _vp, _vp, _vp]),
    "sae_set_eval_precision": (C.c_int, [_vp, C.c_int]),
    "sae_latent_buffer": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "sae_topk_indices": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_int)]),
    "sae_decode": (C.c_int, [_vp, _vp, C.c_int, _i64, _i64, _vp, _vp]),
    "sae_multi_topk_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(C.c_int)]),
    "sae_read_metrics": (C.c_int, [_vp, _fptr, _vp]),
    "sae_latent_colmax": (C.c_int, [_vp, _fptr, _i64, _vp]),
    "sae_debug_read": (C.c_int, [_vp, C.c_int, _fptr, _i64]),
    "sae_l1_backward_plan": (C.c_int, [_vp, _i64, C.POINTER(_i32)]),
    "sae_search_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _vp, _vp]),
    "sae_search_raw_files": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "sae_search_merge": (C.c_int, [_vp, _vp, _i64, _i64, _i64, C.c_int, C.c_int, _dbl, _dbl, _vp, _vp, _vp]),
    "sae_search_file_values": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, _i64, _i64, _i64, _vp, _vp]),
    "sae_file_top_features": (C.c_int, [_vp, _i64, _i64, C.c_int, C.c_int, _vp, _vp, _vp]),
    "sae_stats_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _vp, _vp]),
    "sae_coact_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _vp, _vp]),
    "sae_coact_neighbor_keys": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, _vp]),
    "sae_label_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "sae_label_keys": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, C.c_int, _i64, _i64, _vp, _vp]),
    "sae_cross_mask_bytes": (_i64, [_i64, _i64]),
    "sae_cross_mask_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, C.POINTER(_i32), C.c_int, _vp, _i64, _vp]),
    "sae_cross_update": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "sae_cross_keys": (C.c_int, [_vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _i64, _i64, _vp, _vp]),
    "sae_hist_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int,
                                 C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "sae_timing_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, C.c_int, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sae_dict_pack_bytes": (_i64, [_i64, _i64]),
    "sae_dict_pack": (C.c_int, [_vp, _i64, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp]),
    "sae_dict_sim_keys": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, C.c_int, _vp, _vp]),
    "sae_manipulate_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, C.POINTER(_i32), C.POINTER(_i32), C.c_int, _fptr, C.c_int, C.c_int,
                                       _vp, _vp, _vp, _vp]),
    "sae_recon_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "sae_collect_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "sae_frontier_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _fptr, C.c_int, C.c_int, _vp, _vp]),
    "sae_pursuit_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _fptr, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "sae_refit_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, C.c_int, _fptr, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sae_resample_files": (C.c_int, [_vp, _vp, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp]),
    "sae_resample_workspace_bytes": (_i64, [_i64, _i64]),
    "sae_resample_select": (C.c_int, [_vp, _i64, _vp, _i64, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sae_resample_apply": (C.c_int, [_vp, _vp, _i64, _vp, _dbl, _vp, _vp]),
    "sae_input_stats_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "sae_input_moments": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, _i64, _vp]),
    "sae_input_median": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _dbl, C.c_int, _vp, _vp, _vp, _i64, _vp]),
    "sae_input_cov_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "sae_input_cov_plan": (C.c_int, [_i64, _i64, _i64, C.POINTER(_i64)]),
    "sae_input_cov": (C.c_int, [_vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, _vp, _i64, _vp]),
    "sae_findex_workspace_bytes": (_i64, [_i64, _i64]),
    "sae_findex_count": (C.c_int, [_vp, _vp, _i64, C.c_int, C.c_int, _i64, _vp, _vp, _vp]),
    "sae_findex_fill": (C.c_int, [_vp, _vp, _i64, C.c_int, C.c_int, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp,
                                  _vp]),
    "sae_findex_verify": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp]),
    "sae_store_piece_bytes": (_i64, []),
    "sae_store_convert": (C.c_int, [_vp, _vp, _i64, _vp]),
    "sae_store_gather": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "sae_store_gather_frames": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, C.c_uint64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "sae_profile": (C.c_int, [_vp, C.c_int]),
    "sae_profile_period": (C.c_int, [_vp, C.c_int]),
    "sae_kernel_times": (C.c_int, [_vp, _fptr, C.POINTER(_i32), C.c_int]),
    "sae_kernel_name": (C.c_char_p, [C.c_int]),
    "sae_dominant_kernel": (C.c_int, [_vp]),
}
EXPORTED_SYMBOLS = list(_SIGNATURES)


def load() -> C.CDLL:
    """dlopen the engine and declare every symbol of include/freud_sae.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"{LIB_PATH} is missing: the HIP engine has not been built "
            f"(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C {CSRC_DIR}`). "
            "There is no CPU fallback for the train step.")
    lib = C.CDLL(LIB_PATH)
    skipped = []
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)      # AttributeError here = header / library mismatch
        except AttributeError:
            # FREUD_SAE_ALLOW_OLD_LIB=1 (set by the A/B tools that time an OLDER build against this one, tools/ab_bench.sh): the
            # missing entry points are named once and fail when called.  A user-supplied FREUD_SAE_LIB alone does NOT switch the
            # header / library check off (a stale library would otherwise fail at an arbitrary call site mid-training).
            if os.environ.get("FREUD_SAE_ALLOW_OLD_LIB") == "1":
                skipped.append(name)
                continue
            raise EngineError(f"{LIB_PATH} does not export {name}: the library is older than include/freud_sae.h "
                              "(rebuild it, or set FREUD_SAE_ALLOW_OLD_LIB=1 for an A/B timing of an old build)") from None
        fn.restype = res
        fn.argtypes = args
    if skipped:
        print(f"freud_amd.engine: {LIB_PATH} lacks {', '.join(skipped)} (FREUD_SAE_ALLOW_OLD_LIB=1)", file=sys.stderr)
    _lib = lib
    return lib


SEARCH_ABS, SEARCH_MIN, SEARCH_MAX, SEARCH_UNFUSED = 1, 2, 4, 8     # include/freud_sae.h: SAE_SEARCH_*
SEARCH_MAX_TOP = 4096
FILE_TOP_POSITIVE = 1                                               # include/freud_sae.h: SAE_FILE_TOP_POSITIVE
FILE_TOP_MAX = 1024                                                 # include/freud_sae.h: SAE_FILE_TOP_MAX
STATS_UNFUSED = 1                                                   # include/freud_sae.h: SAE_STATS_UNFUSED
COACT_MEASURES = {"jaccard": 0, "cond": 1, "count": 2}              # include/freud_sae.h: SAE_COACT_*
LABEL_MEASURES = {"f1": 0, "precision": 1, "recall": 2, "count": 3}  # include/freud_sae.h: SAE_LABEL_*
LABEL_MAX_CLASSES = 4096                                            # include/freud_sae.h: SAE_LABEL_MAX_CLASSES
LABEL_MAX_SLOTS = 16                                                # include/freud_sae.h: SAE_LABEL_MAX_SLOTS
CROSS_MEASURES = {"jaccard": 0, "cond": 1, "lift": 2, "count": 3}   # include/freud_sae.h: SAE_CROSS_*
CROSS_SOURCE, CROSS_TARGET = 1, 2                                   # include/freud_sae.h: SAE_CROSS_SOURCE / SAE_CROSS_TARGET
CROSS_MAX_LAG, CROSS_MAX_LAGS = 32768, 8                            # include/freud_sae.h: SAE_CROSS_MAX_LAG / SAE_CROSS_MAX_LAGS
HIST_MAX_REGULAR = 128                                              # freud_amd/csrc/hist_bins.h: octaves << sub_bits at most
HIST_MAX_SEL = 64                                                   # include/freud_sae.h: SAE_HIST_MAX_SEL
TIMING_ACTIVE, TIMING_SPAN, TIMING_RUNS, TIMING_FILES, TIMING_LONGEST, TIMING_CENSORED, TIMING_NTOTALS = range(7)   # include/freud_sae.h: SAE_TIMING_*
TIMING_ONE_CHUNK = 1                                                # include/freud_sae.h: SAE_TIMING_ONE_CHUNK
TIMING_MAX_BINS, TIMING_MAX_BRIDGE, TIMING_MAX_ROWS = 111, 15, 65535  # include/freud_sae.h: SAE_TIMING_MAX_*; freud_amd/csrc/timing_bins.h: TB_MAX_ROWS
COLLECT_IDX32 = 1                                                   # include/freud_sae.h: SAE_COLLECT_IDX32
COLLECT_MAX_K = 1024                                                # include/freud_sae.h: SAE_COLLECT_MAX_K
FRONTIER_MAX_K, FRONTIER_MAX_TAU = 256, 8                           # include/freud_sae.h: SAE_FRONTIER_MAX_K / SAE_FRONTIER_MAX_TAU
PURSUIT_MAX_K, PURSUIT_MAX_TAU = 256, 8                             # include/freud_sae.h: SAE_PURSUIT_MAX_K / SAE_PURSUIT_MAX_TAU
REFIT_MAX_K, REFIT_MAX_TAU, REFIT_RATIO_BINS = 128, 8, 36           # include/freud_sae.h: SAE_REFIT_MAX_K / _MAX_TAU / _RATIO_BINS
FINDEX_IDX32 = 1                                                    # include/freud_sae.h: SAE_FINDEX_IDX32
FINDEX_NSTATS = 8                                                   # include/freud_sae.h: SAE_FINDEX_NSTATS
FINDEX_STAT_NAMES = ("slots", "zero_slots", "out_of_range", "posted")
FINDEX_ROWS, FINDEX_SEGMENT = 128, 16384                            # freud_amd/csrc/findex.h: FI_ROWS, FI_SEG (rows per block, latents per LDS segment)
DICT_LEFT, DICT_RIGHT = 0, 1                                        # include/freud_sae.h: SAE_DICT_LEFT / SAE_DICT_RIGHT
DICT_MAX_D = 8192                                                   # include/freud_sae.h: SAE_DICT_MAX_D
DICT_MAX_N = 1 << 24
MANIP_OPS = {"scale": 0, "set": 1}                                  # include/freud_sae.h: SAE_MANIP_SCALE / SAE_MANIP_SET
MANIP_MAX_EDITS = 16                                                # include/freud_sae.h: SAE_MANIP_MAX_EDITS
MANIP_MAX_VARIANTS = 16                                             # include/freud_sae.h: SAE_MANIP_MAX_VARIANTS
RECON_UNFUSED = 1                                                   # include/freud_sae.h: SAE_RECON_UNFUSED
RESAMPLE_DEAD, RESAMPLE_PAIRS, RESAMPLE_SKIPPED_DUPLICATE, RESAMPLE_TOTAL, RESAMPLE_LMAX_BITS = range(5)   # include/freud_sae.h: SAE_RESAMPLE_*
RESAMPLE_NCOUNTS = 8                                                # include/freud_sae.h: SAE_RESAMPLE_NCOUNTS
INPUT_MAX_D, INPUT_MAX_ITERATIONS = 2048, 1024                      # include/freud_sae.h: SAE_INPUT_MAX_*


_DTYPE_BYTES = {"int64": 8, "float64": 8, "float32": 4}


def _layout(fields, align: int = 1) -> dict:
    """An output block as include/freud_sae.h lays it out -- the fields (name, dtype, count) one after another from offset 0:
    name -> (offset, dtype, count), plus "bytes": the block's size, rounded up to `align`."""
    out, at = {}, 0
    for name, dtype, count in fields:
        out[name] = (at, dtype, count)
        at += _DTYPE_BYTES[dtype] * count
    out["bytes"] = -(-at // align) * align
    return out


def stats_layout(n: int) -> dict:
    """The sae_stats_files block for n latents (include/freud_sae.h: SAE_STATS_*): see _layout."""
    return _layout([("n_frames", "int64", 1), ("fire_count", "int64", n), ("act_sum", "float64", n), ("act_sq_sum", "float64", n),
                    ("l0_hist", "int64", n + 1), ("act_max", "float32", n)])


def recon_layout(n: int, d: int) -> dict:
    """The sae_recon_files block for n latents and d model dimensions (include/freud_sae.h: SAE_RECON_*): see _layout."""
    return _layout([("n_frames", "int64", 1), ("attr_sum", "float64", n), ("act_sq_sum", "float64", n), ("sum_x", "float64", d),
                    ("sum_x_sq", "float64", d), ("sum_r_sq", "float64", d), ("dec_norm_sq", "float32", n)], align=8)


def _curve_fields(n_tau: int, K: int, d: int, after_sse=()) -> list:
    """What every block of the frontier family holds after its leading counts: the curve, the denominators, the budget histograms."""
    return [("sse", "float64", K + 1), *after_sse, ("sum_x", "float64", d), ("sum_x_sq", "float64", d), ("budget", "int64", n_tau * (K + 2))]


def frontier_layout(n_tau: int, K: int, d: int) -> dict:
    """The sae_frontier_files block for n_tau thresholds, K slots and d model dimensions (include/freud_sae.h: SAE_FRONTIER_*): see
    _layout."""
    return _layout([("n_frames", "int64", 1), ("rows_cut", "int64", 1), ("active_cut", "int64", 1), *_curve_fields(n_tau, K, d)])


def pursuit_layout(n_tau: int, K: int, d: int, n: int) -> dict:
    """The sae_pursuit_files block for n_tau thresholds, K steps, d model dimensions and n latents (include/freud_sae.h:
    SAE_PURSUIT_*): see _layout."""
    return _layout([("n_frames", "int64", 1), *_curve_fields(n_tau, K, d), ("steps", "int64", K + 1), ("picks", "int64", n),
                    ("in_support", "int64", K)])


def refit_layout(n_tau: int, K: int, d: int, n: int) -> dict:
    """The sae_refit_files block for n_tau thresholds, K slots, d model dimensions and n latents (include/freud_sae.h: SAE_REFIT_*):
    see _layout."""
    return _layout([("n_frames", "int64", 1), *_curve_fields(n_tau, K, d, after_sse=[("sse_final", "float64", 1)]),
                    ("kept", "int64", K + 1), ("slots", "int64", n), ("neg", "int64", n), ("dep", "int64", n),
                    ("ratio", "int64", REFIT_RATIO_BINS), ("bad_index", "int64", 1)])


def unpack_block(block, layout: dict) -> Dict[str, np.ndarray]:
    """The arrays of a block read back from the device (uint8 bytes) by its stats_layout / recon_layout: name -> a copy."""
    b = np.ascontiguousarray(block).view(np.uint8)
    return {name: np.frombuffer(b, dtype=at[1], count=at[2], offset=at[0]).copy() for name, at in layout.items() if name != "bytes"}


def check_sub_bits(sub_bits) -> int:
    """sub_bits (2^sub_bits bins per octave: freud_amd/csrc/hist_bins.h, timing_bins.h) as an int; ValueError outside [0, 3]."""
    sub_bits = int(sub_bits)
    if sub_bits < 0 or sub_bits > 3:
        raise ValueError(f"sub_bits={sub_bits} outside [0, 3]")
    return sub_bits


def hist_nbins(spec) -> int:
    """Bins of a histogram spec (lo_exp, octaves, sub_bits) -- freud_amd/csrc/hist_bins.h; ValueError for a spec outside its limits."""
    lo_exp, octaves, sub_bits = (int(v) for v in spec)
    check_sub_bits(sub_bits)
    if lo_exp < -126 or octaves < 1 or lo_exp + octaves > 128:
        raise ValueError(f"lo_exp={lo_exp}, octaves={octaves}: -126 <= lo_exp, octaves >= 1 and lo_exp + octaves <= 128")
    if (octaves << sub_bits) > HIST_MAX_REGULAR:
        raise ValueError(f"octaves={octaves} x {1 << sub_bits} bins per octave > {HIST_MAX_REGULAR}")
    return (octaves << sub_bits) + 3


def timing_index(L: int, sub_bits: int) -> int:
    """idx of a duration or gap of L >= 1 frames (bin = idx - 1) -- freud_amd/csrc/timing_bins.h, integers only."""
    L, s = int(L), int(sub_bits)
    if L < (2 << s):
        return L
    sh = (L.bit_length() - 1) - s
    return (sh << s) + (L >> sh)


def timing_nbins(sub_bits: int, T: int) -> int:
    """Bins of the feature timing for files of T frames -- freud_amd/csrc/timing_bins.h; ValueError for a spec outside its limits."""
    sub_bits, T = check_sub_bits(sub_bits), int(T)
    if T < 1 or T > TIMING_MAX_ROWS:
        raise ValueError(f"T={T} frames per file outside [1, {TIMING_MAX_ROWS}]")
    return timing_index(T, sub_bits)


def _check(rc: int) -> None:
    if rc != 0:
        raise EngineError(f"libfreud_sae error {rc}: {load().sae_last_error().decode()}")


def _np_f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _tau_arg(fn_name: str, thresholds, max_tau: int) -> np.ndarray:
    """The thresholds of a frontier-family pass as a flat float32 host array of at most max_tau values."""
    tau = _np_f32(thresholds).reshape(-1)
    if tau.size > max_tau:
        raise EngineError(f"{fn_name}: {tau.size} thresholds > {max_tau}")
    return tau


def _shaped(name: str, a, shape) -> np.ndarray:
    """fp32 contiguous copy of `a` with exactly `shape` elements (the C side copies prod(shape) floats from the pointer:
    a short buffer would be a host heap over-read)."""
    arr = _np_f32(a)
    if arr.size != int(np.prod(shape)):
        raise EngineError(f"{name}: got {arr.shape} ({arr.size} elements), the engine expects {tuple(shape)}")
    return arr.reshape(shape)


def _quad(arrays):
    """The four pointer slots of the parameter and optimizer-state calls: the arrays' host pointers in parameter order, then nulls."""
    ptrs = [a.ctypes.data for a in arrays]
    return (C.c_void_p * 4)(*(ptrs + [None] * (4 - len(ptrs))))


class SaeEngine:
    """One engine context = one SAE on one GPU.  Thin, typed wrapper over the C ABI."""

    def __init__(self, variant: str, d_model: int, n_dict: int, max_rows: int, *, optimizer: str = "radam",
                 recon_alpha: float = 1.0, k: int = 0, auxk_alpha: float = 0.0, clip_thresh: float = 1.0,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: Optional[float] = None, device_id: int = 0,
                 force_generic: bool = False, debug_flags: int = 0, force_gemm128: bool = False,
                 topk_dense_backward: bool = False, multi_topk: bool = False, precision: str = "bf16"):
        if variant not in VARIANT:
            raise AssertionError(f"Invalid autoencoder variant: {variant}, must be 'l1' or 'topk'")
        if optimizer not in OPTIMIZER:
            raise ValueError(f"Invalid optimizer: {optimizer}, must be 'radam' or 'adam'")
        self._lib = load()
        if eps is None:  # train_sae.py:374-379: RAdam(eps=1e-5), Adam default 1e-8
            eps = 1e-5 if optimizer == "radam" else 1e-8
        cfg = SaeConfig()
        cfg.variant, cfg.d_model, cfg.n_dict, cfg.k = VARIANT[variant], d_model, n_dict, k
        cfg.optimizer, cfg.device_id, cfg.max_rows = OPTIMIZER[optimizer], device_id, max_rows
        cfg.recon_alpha, cfg.auxk_alpha, cfg.clip_thresh = recon_alpha, auxk_alpha, clip_thresh
        cfg.weight_decay, cfg.beta1, cfg.beta2, cfg.eps = weight_decay, betas[0], betas[1], eps
        cfg.debug_flags = debug_flags                 # timing experiments only (results become wrong)
        cfg.force_generic = 1 if force_generic else 0   # 1 = generic three-GEMM backward even where a fused kernel exists
        cfg.force_gemm128 = 1 if force_gemm128 else 0   # 1 = 128x128 GEMM tiles even where the 256x256 kernel applies
        cfg.topk_dense_backward = int(topk_dense_backward)   # 0 = CSC sparse backward; 1 = dense GEMM + mask; 2 = sparse dpre + dense dW GEMMs
        cfg.multi_topk = 1 if multi_topk else 0       # TopKAutoEncoderConfig.multi_topk
        if precision not in PRECISION:
            raise ValueError(f"Invalid precision: {precision}, must be one of {sorted(PRECISION)}")
        cfg.precision = PRECISION[precision]
        self.variant, self.d, self.n, self.max_rows, self.device_id = variant, d_model, n_dict, max_rows, device_id
        self.k, self.multi_topk, self.precision = k, bool(multi_topk), precision
        self._ctx = C.c_void_p()
        _check(self._lib.sae_create(C.byref(cfg), C.byref(self._ctx)))

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.sae_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters ---------------------------------------------------------------------------
    def param_shapes(self) -> Dict[str, tuple]:
        """Reference state_dict keys and shapes, in the engine's parameter order."""
        if self.variant == "l1":   # l1autoencoder.py:56-60
            return {"decoder.weight": (self.d, self.n), "encoder_bias": (self.n,)}
        return {"encoder.weight": (self.n, self.d), "encoder.bias": (self.n,),
                "W_dec": (self.n, self.d), "b_dec": (self.d,)}   # topkautoencoder.py:62-70

    def set_params(self, params: Dict[str, np.ndarray]) -> None:
        arrs = [_shaped(k, params[k], shape) for k, shape in self.param_shapes().items()]
        _check(self._lib.sae_set_params(self._ctx, *_quad(arrs), 0))

    def get_params(self) -> Dict[str, np.ndarray]:
        out = {k: np.empty(shape, dtype=np.float32) for k, shape in self.param_shapes().items()}
        _check(self._lib.sae_get_params(self._ctx, *_quad(out.values()), 0))
        return out

    def set_opt_state(self, step: int, exp_avg: Dict[str, np.ndarray], exp_avg_sq: Dict[str, np.ndarray]) -> None:
        shapes = self.param_shapes()
        a = [_shaped(f"exp_avg[{k}]", exp_avg[k], s) for k, s in shapes.items()]
        b = [_shaped(f"exp_avg_sq[{k}]", exp_avg_sq[k], s) for k, s in shapes.items()]
        _check(self._lib.sae_set_opt_state(self._ctx, int(step), _quad(a), _quad(b), 0))

    def get_opt_state(self):
        shapes = self.param_shapes()
        a = {k: np.empty(s, dtype=np.float32) for k, s in shapes.items()}
        b = {k: np.empty(s, dtype=np.float32) for k, s in shapes.items()}
        step = C.c_int64(0)
        _check(self._lib.sae_get_opt_state(self._ctx, C.byref(step), _quad(a.values()), _quad(b.values()), 0))
        return int(step.value), a, b

    def set_topk_options(self, dead_feature_threshold: float, rows_per_file: int) -> None:
        """TopK only: autoencoder_config["dead_feature_threshold"] (train_sae.py:438) and T of the [B][T][d] batch."""
        self._dead_threshold, self._rows_per_file = float(dead_feature_threshold), int(rows_per_file)
        _check(self._lib.sae_set_topk_options(self._ctx, float(dead_feature_threshold), int(rows_per_file)))

    def set_decoder_constraint(self, on: bool, keep_rows: bool = False) -> None:
        """TopK, bf16 contexts only (EngineError otherwise).  While on, every optimizer_step() / step() projects the gradient of W_dec
        off its rows before the clip norm and renormalises the rows after the update (the reference model's
        remove_gradient_parallel_to_decoder_directions / set_decoder_norm_to_unit_norm, topkautoencoder.py:153-175, which its train()
        never calls).  Switching it on, and set_params() while it is on, renormalise the rows at once: loading weights that were
        trained without the constraint changes the model.  keep_rows: switch it on without that renorm -- for rows a constrained
        run left (its own checkpoint, loaded before the switch), which a second renorm would move by an ulp."""
        _check(self._lib.sae_set_decoder_constraint(self._ctx, (2 if keep_rows else 1) if on else 0))

    @property
    def decoder_constraint(self) -> bool:
        return self._lib.sae_get_decoder_constraint(self._ctx) == 1

    def get_topk_state(self) -> np.ndarray:
        """TopK only: num_frames_since_fired[n_dict] (int64) - train_sae.py:412-415 keeps it in the live process only."""
        out = np.zeros(self.n, dtype=np.int64)
        _check(self._lib.sae_get_topk_state(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int64)), self.n))
        return out

    def set_topk_state(self, num_frames_since_fired) -> None:
        a = np.ascontiguousarray(np.asarray(num_frames_since_fired, dtype=np.int64).reshape(-1))
        _check(self._lib.sae_set_topk_state(self._ctx, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size))

    def set_dead_feature_threshold(self, v: float) -> None:
        self.set_topk_options(v, getattr(self, "_rows_per_file", 0))

    # -- the hot path -------------------------------------------------------------------------
    @staticmethod
    def _x_args(x):
        """x: a torch CUDA tensor [M, d] (or [B, T, d]) fp32/fp16/bf16, contiguous."""
        import torch
        if not x.is_cuda:
            raise EngineError("activations must live in HBM (torch CUDA tensor); there is no CPU path")
        if not x.is_contiguous():
            x = x.contiguous()
        name = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}.get(x.dtype)
        if name is None:
            raise EngineError(f"unsupported activation dtype {x.dtype}")
        rows = x.numel() // x.shape[-1]
        return x, x.data_ptr(), rows, DTYPE[name]

    def _note_shape(self, x) -> None:
        """TopK: x.mean(0) is over the files of a [B, T, d] batch -> tell the engine T when it changes."""
        if self.variant == "topk" and x.dim() == 3 and getattr(self, "_rows_per_file", None) != x.shape[1]:
            self.set_topk_options(getattr(self, "_dead_threshold", 1e300), x.shape[1])

    def _x(self, x):
        """The front of every hot-path call: _note_shape, then what _x_args returns.  (The variant is tested here and the tuple is
        passed on as it is, so that an L1 step makes the two calls it made before and nothing else.)"""
        if self.variant == "topk":
            self._note_shape(x)
        return self._x_args(x)

    def forward_backward(self, x, stream=None) -> None:
        x, ptr, rows, dt = self._x(x)
        _check(self._lib.sae_forward_backward(self._ctx, C.c_void_p(ptr), rows, dt, _stream_ptr(stream)))
        err, self._cb_error = getattr(self, "_cb_error", None), None
        if err is not None:
            raise err

    # -- data parallel (include/freud_sae.h, "data-parallel exactness") ------------------------------------
    def batch_stats(self, x, stream=None) -> None:
        """This rank's statistics of batch x (what the losses normalise by) into the statistics buffer."""
        x, ptr, rows, dt = self._x(x)
        _check(self._lib.sae_batch_stats(self._ctx, C.c_void_p(ptr), rows, dt, _stream_ptr(stream)))

    def stats_tensor(self):
        """The statistics of the last batch_stats() as a float64 torch CUDA tensor aliasing the engine's buffer:
        all-reduce (sum) it over the ranks before forward_backward()."""
        p, n = C.c_void_p(), C.c_int64()
        _check(self._lib.sae_stats_buffer(self._ctx, C.byref(p), C.byref(n)))
        return _alias(int(p.value), (int(n.value),), "<f8", f"cuda:{self.device_id}")

    def set_dp_world(self, world: int) -> None:
        _check(self._lib.sae_set_dp_world(self._ctx, int(world)))

    @staticmethod
    def dist_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load().sae_dist_unique_id(buf, 128))
        return buf.raw

    def dist_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """Give the context its own RCCL communicator: forward_backward() / step() then run the data-parallel protocol
        (statistics and gradient all-reduces on a communication stream) inside the engine."""
        buf = C.create_string_buffer(bytes(unique_id), len(unique_id))
        _check(self._lib.sae_dist_init(self._ctx, buf, len(unique_id), int(rank), int(world)))

    def dist_world(self) -> int:
        return int(self._lib.sae_dist_world(self._ctx))

    def dist_set_payload(self, dtype: str) -> None:
        """"float32" (default, exact) or "bfloat16" (fused d=384 path: half the all-reduce bytes)."""
        _check(self._lib.sae_dist_set_payload(self._ctx, DTYPE[dtype]))

    def p2p_export(self) -> bytes:
        """This rank's blob for the peer exchange (hipIpc handles of the gradient / statistics / flag buffers)."""
        nbytes = int(self._lib.sae_p2p_blob_bytes())
        buf = C.create_string_buffer(nbytes)
        _check(self._lib.sae_p2p_export(self._ctx, buf, nbytes))
        return buf.raw

    def p2p_init(self, blobs: Sequence[bytes], rank: int, world: int) -> None:
        """Map the peers from the blobs of ALL ranks (rank order) and run the self-test exchange.  Collective.  Afterwards
        forward_backward() / step() run the data-parallel protocol with the engine's own exchange kernels."""
        assert len(blobs) == world and all(len(b) == len(blobs[0]) for b in blobs)
        joined = b"".join(blobs)
        buf = C.create_string_buffer(joined, len(joined))
        _check(self._lib.sae_p2p_init(self._ctx, buf, len(blobs[0]), int(rank), int(world)))

    def p2p_leave(self) -> None:
        """Undo p2p_init (a peer's self-test failed although this rank's passed: the ranks fall back together)."""
        _check(self._lib.sae_p2p_leave(self._ctx))

    def dist_set_overlap(self, nranges: int) -> None:
        """Fused d=384 backward in `nranges` column-tile ranges, each exchanged under the next one's backward."""
        _check(self._lib.sae_dist_set_overlap(self._ctx, int(nranges)))

    def dist_check(self) -> None:
        """Synchronise and raise if an in-engine exchange failed (a peer never arrived)."""
        _check(self._lib.sae_dist_check(self._ctx))

    def dist_poll(self) -> None:
        """The same report without synchronising (host-mapped failure word): free after every step."""
        _check(self._lib.sae_dist_poll(self._ctx))

    def dist_audit(self, snapshot) -> None:
        """snapshot: a float32 CUDA tensor shaped like grad_tensor() (kept alive by the caller) -- every gradient exchange
        first copies the segments it is about to sum into it; None switches the snapshots off (freud_amd/dp.py: audit)."""
        if snapshot is None:
            _check(self._lib.sae_dist_audit(self._ctx, None))
            return
        g = self.grad_tensor()
        assert snapshot.is_cuda and snapshot.dtype == g.dtype and snapshot.numel() == g.numel() and snapshot.is_contiguous()
        _check(self._lib.sae_dist_audit(self._ctx, C.c_void_p(snapshot.data_ptr())))

    def grad_layout(self) -> tuple:
        """(parameter-gradient floats, loss scalars, did_fire flags) of grad_tensor(), in that order."""
        out = (C.c_int64 * 3)()
        _check(self._lib.sae_grad_layout(self._ctx, out))
        return tuple(int(v) for v in out)

    def param_checksum(self) -> tuple:
        """(parameters, first moments, second moments, step): order-independent 64-bit checksums of the fp32 bits.  Replicas
        of a data-parallel run must agree on all four (train() compares them over the host channel).  Synchronises."""
        out = (C.c_uint64 * 4)()
        _check(self._lib.sae_param_checksum(self._ctx, out))
        return tuple(int(v) for v in out)

    def optimizer_step(self, lr: float, grad_scale: float = 1.0, stream=None) -> None:
        _check(self._lib.sae_optimizer_step(self._ctx, float(lr), float(grad_scale), _stream_ptr(stream)))

    def step(self, x, lr: float, stream=None) -> None:
        x, ptr, rows, dt = self._x(x)
        _check(self._lib.sae_step(self._ctx, C.c_void_p(ptr), rows, dt, float(lr), _stream_ptr(stream)))

    def eval(self, x, stream=None) -> None:
        x, ptr, rows, dt = self._x(x)
        _check(self._lib.sae_eval(self._ctx, C.c_void_p(ptr), rows, dt, _stream_ptr(stream)))

    def set_eval_precision(self, precision: str) -> None:
        """"bf16" (default): eval() / eval_into() run the training kernels' arithmetic (CPU autocast's).  "fp32": fp32 end to end --
        what the reference's validate() computes on device='cpu' (train_sae.py:162-166) and selects bestval.pth by.  The fp32
        forward takes at most max_rows rows and leaves no bf16 latent: after it latent_buffer(), topk_indices_tensor(),
        multi_topk_buffers() and debug_read(0 / 1 / 3 / 8 / 9) raise EngineError until the next bf16 eval() / step(); metrics(),
        latent_colmax(), debug_read(2), get_params(), get_opt_state(), get_topk_state() and decode() stay valid."""
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"Invalid evaluation precision: {precision}, must be 'bf16' or 'fp32'")
        _check(self._lib.sae_set_eval_precision(self._ctx, 3 if precision == "fp32" else PRECISION["bf16"]))
        self.eval_precision = precision

    def eval_into(self, x, metrics_row, colmax_row=None, stream=None) -> None:
        """eval() of one file with its 8 loss scalars (and per-feature latent maxima) left in the given fp32 CUDA rows:
        no host synchronisation (validate() reads all rows once at the end)."""
        x, ptr, rows, dt = self._x(x)
        assert metrics_row.is_cuda and metrics_row.is_contiguous() and metrics_row.numel() >= NUM_METRICS
        cm = None
        if colmax_row is not None:
            assert colmax_row.is_cuda and colmax_row.is_contiguous() and colmax_row.numel() >= self.n
            cm = C.c_void_p(colmax_row.data_ptr())
        _check(self._lib.sae_eval_into(self._ctx, C.c_void_p(ptr), rows, dt, C.c_void_p(metrics_row.data_ptr()), cm, _stream_ptr(stream)))

    # -- inference ---------------------------------------------------------
    def latent_buffer(self):
        """(device pointer, row stride in elements) of the bf16 latent of the last forward (EngineError after an fp32 evaluation)."""
        ptr, ld = C.c_void_p(), C.c_int64()
        _check(self._lib.sae_latent_buffer(self._ctx, C.byref(ptr), C.byref(ld)))
        return ptr.value, ld.value

    def topk_indices_tensor(self, rows: int, device):
        """int32 [rows][k] torch view of the top-k indices of the last forward (TopK contexts; EngineError after an fp32 evaluation)."""
        ptr, k = C.c_void_p(), C.c_int()
        _check(self._lib.sae_topk_indices(self._ctx, C.byref(ptr), C.byref(k)))
        return _alias(ptr.value, (rows, k.value), "<i4", device)

    def multi_topk_buffers(self, rows: int, device):
        """TopK with multi_topk: (bf16 [rows][n_dict] dense 4k activations, int32 [rows][4k] indices) of the last forward
        (EngineError after an fp32 evaluation)."""
        import torch
        dptr, ld, iptr, k4 = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int()
        _check(self._lib.sae_multi_topk_buffers(self._ctx, C.byref(dptr), C.byref(ld), C.byref(iptr), C.byref(k4)))
        dense = _alias(dptr.value, (rows, ld.value), "<i2", device).view(torch.bfloat16)[:, : self.n]
        return dense, _alias(iptr.value, (rows, k4.value), "<i4", device)

    def decode(self, latent, out, stream=None) -> None:
        """out[rows][d_model] (fp32 CUDA tensor) = decode(latent[rows][>= n_dict]) (fp32 or bf16 CUDA tensor, row-major)."""
        import torch
        assert latent.is_cuda and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
        assert latent.dim() == 2 and latent.stride(1) == 1
        dt = {torch.float32: DTYPE["float32"], torch.bfloat16: DTYPE["bfloat16"]}.get(latent.dtype)
        if dt is None:
            raise EngineError(f"unsupported latent dtype {latent.dtype}: decode takes float32 or bfloat16")
        if latent.shape[1] < self.n:     # (the C side sees the row stride only: a narrow view of a wide tensor would pass it)
            raise EngineError(f"latent has {latent.shape[1]} columns, the dictionary {self.n}")
        _check(self._lib.sae_decode(self._ctx, C.c_void_p(latent.data_ptr()), dt, int(latent.stride(0)), int(latent.shape[0]),
                                    C.c_void_p(out.data_ptr()), _stream_ptr(stream)))

    def metrics(self, stream=None) -> np.ndarray:
        out = np.zeros(NUM_METRICS, dtype=np.float32)
        _check(self._lib.sae_read_metrics(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), _stream_ptr(stream)))
        return out

    def latent_colmax(self, stream=None) -> np.ndarray:
        """max over rows of |latent| per dictionary feature for the last forward (validate()), the fp32 evaluation included."""
        out = np.empty(self.n, dtype=np.float32)
        _check(self._lib.sae_latent_colmax(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), self.n, _stream_ptr(stream)))
        return out

    def grad_buffer(self):
        """(device pointer, number of floats) of the flat gradient + metrics buffer (for all-reduce)."""
        p, n = C.c_void_p(), C.c_int64()
        _check(self._lib.sae_grad_buffer(self._ctx, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def set_grad_ready_callback(self, fn) -> None:
        """fn(offset, count) is called from inside forward_backward() each time the range [offset, offset + count) of the
        gradient buffer is final in stream order (data-parallel overlap: start that range's all-reduce).  None removes
        it.  Exceptions raised by fn are re-raised by forward_backward()."""
        self._cb_error = None
        if fn is None:
            self._cb = None
            _check(self._lib.sae_set_grad_ready_callback(self._ctx, C.cast(None, GRAD_READY_FN), None))
            return

        def tramp(_user, offset, count, _stream):
            try:
                fn(int(offset), int(count))
            except BaseException as e:      # never unwind through the C frames
                self._cb_error = e

        self._cb = GRAD_READY_FN(tramp)     # keep the thunk alive
        _check(self._lib.sae_set_grad_ready_callback(self._ctx, self._cb, None))

    def grad_tensor(self):
        """The gradient buffer as a torch CUDA tensor aliasing the engine's HBM (no copy)."""
        ptr, n = self.grad_buffer()
        return _alias(ptr, (n,), "<f4", f"cuda:{self.device_id}")

    # -- feature search (include/freud_sae.h: sae_search_*; freud_amd/feature_search.py) ------------------
    def search_files(self, x, file_keys, lengths=None, unfused: bool = False, stream=None) -> None:
        """Per-(file, latent) keys of x [n_files, T, d] (CUDA) into file_keys (int64 CUDA tensor [n_files, n_dict]); lengths: int32
        CUDA tensor [n_files] or None.  Asynchronous.  Afterwards the last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "search_files", lengths)
        keys = _dev("file_keys", file_keys, "int64", B * self.n, at_least=True)
        _check(self._lib.sae_search_files(self._ctx, xp, B, T, dt, lp, SEARCH_UNFUSED if unfused else 0, keys, _stream_ptr(stream)))

    # -- feature statistics (include/freud_sae.h: sae_stats_files; freud_amd/feature_stats.py) -----------------------------
    def stats_files(self, x, stats_block, lengths=None, unfused: bool = False, stream=None) -> None:
        """Add the statistics of x [n_files, T, d] (CUDA) to stats_block (a zero-initialised uint8 CUDA tensor of
        stats_layout(n)["bytes"] bytes); lengths: int32 CUDA tensor [n_files] or None.  Asynchronous.  Afterwards the last-forward
        getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "stats_files", lengths)
        block = _dev("stats_block", stats_block, "uint8", stats_layout(self.n)["bytes"], at_least=True)
        _check(self._lib.sae_stats_files(self._ctx, xp, B, T, dt, lp, STATS_UNFUSED if unfused else 0, block, _stream_ptr(stream)))

    # -- feature co-activation (include/freud_sae.h: sae_coact_files; freud_amd/coactivation.py) ---------------------------
    def coact_files(self, x, counts, lengths=None, stream=None) -> None:
        """Add the co-activation counts of x [n_files, T, d] (CUDA) to counts (a zero-initialised contiguous int32 CUDA tensor
        [n_dict, n_dict]); lengths: int32 CUDA tensor [n_files] or None.  Asynchronous.  Afterwards the last-forward getters fail
        until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "coact_files", lengths)
        table = _dev("counts", counts, "int32", self.n * self.n)
        _check(self._lib.sae_coact_files(self._ctx, xp, B, T, dt, lp, 0, table, _stream_ptr(stream)))

    # -- feature labels (include/freud_sae.h: sae_label_files; freud_amd/feature_labels.py) ---------------------------------
    def label_files(self, x, labels, n_classes: int, counts, label_count, lengths=None, stream=None) -> None:
        """Add the label counts of x [n_files, T, d] (CUDA) with labels (a contiguous int32 CUDA tensor [n_files, T, n_slots]: class
        ids in [0, n_classes), -1 = empty) to counts (zero-initialised contiguous int32 CUDA [n_classes + 1, n_dict]) and label_count
        (zero-initialised int64 CUDA [n_classes + 1]); lengths: int32 CUDA tensor [n_files] or None.  Asynchronous.  Afterwards
        the last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "label_files", lengths)
        lab, n_slots = _labels_arg(labels, B, T)
        table, lc = _label_table(counts, label_count, n_classes, self.n)
        _check(self._lib.sae_label_files(self._ctx, xp, B, T, dt, lp, lab, n_slots, int(n_classes), 0, table, lc, _stream_ptr(stream)))

    # -- cross-activation (include/freud_sae.h: sae_cross_mask_files; freud_amd/cross_activation.py) ---------------------------
    def cross_mask_files(self, x, masks, sides: int, lags=(), lengths=None, stream=None) -> None:
        """One encode of x [n_files, T, d] (CUDA), then its activity masks into masks (a contiguous int8 or uint8 CUDA tensor): the
        source mask (sides & CROSS_SOURCE), then one target mask per lag (sides & CROSS_TARGET), each of
        cross_mask_bytes(n_dict, n_files * T) bytes; lengths: int32 CUDA tensor [n_files] or None.  Asynchronous.  Afterwards the
        last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "cross_mask_files", lengths)
        lags = [int(v) for v in lags]
        m = _dev("masks", masks, ("int8", "uint8"), 0, at_least=True)
        arr = (C.c_int32 * max(len(lags), 1))(*lags)
        _check(self._lib.sae_cross_mask_files(self._ctx, xp, B, T, dt, lp, int(sides), arr if lags else None, len(lags), m,
                                              int(masks.numel()), _stream_ptr(stream)))

    # -- activation histograms (include/freud_sae.h: sae_hist_files; freud_amd/activation_hist.py) ------------------------------
    def hist_files(self, x, spec, frame_hist, file_max_hist, n_frames, lengths=None, labels=None, n_classes: int = 0, sel_latents=None,
                   label_hist=None, label_count=None, stream=None) -> None:
        """Add the activation histograms of x [n_files, T, d] (CUDA) for spec = (lo_exp, octaves, sub_bits), NB = hist_nbins(spec),
        to frame_hist and file_max_hist (zero-initialised contiguous int64 CUDA [n_dict, NB]) and n_frames (int64 CUDA [1]); lengths:
        int32 CUDA tensor [n_files] or None.  With sel_latents (int32 CUDA [n_sel], n_sel <= HIST_MAX_SEL) and labels (contiguous
        int32 CUDA [n_files, T, n_slots], as label_files) also to label_hist (int64 CUDA [n_sel, n_classes + 1, NB]) and label_count
        (int64 CUDA [n_classes + 1]).  The same arrays go to every call of one pass.  Asynchronous.  Afterwards the last-forward
        getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "hist_files", lengths)
        lo_exp, octaves, sub_bits = (int(v) for v in spec)
        nb = hist_nbins(spec)
        fh, mh = _dev("frame_hist", frame_hist, "int64", self.n * nb), _dev("file_max_hist", file_max_hist, "int64", self.n * nb)
        nf = _dev("n_frames", n_frames, "int64", 1)
        n_sel = 0 if sel_latents is None else int(sel_latents.numel())
        lab = sel = lh = lc = None
        n_slots = 0
        if n_sel:
            if n_sel > HIST_MAX_SEL:
                raise EngineError(f"{n_sel} chosen latents > {HIST_MAX_SEL}")
            sel = _dev("sel_latents", sel_latents, "int32", n_sel)      # (its own size: n_sel is read off it)
            lab, n_slots = _labels_arg(labels, B, T)
            lh = _dev("label_hist", label_hist, "int64", n_sel * (int(n_classes) + 1) * nb)
            lc = _dev("label_count", label_count, "int64", int(n_classes) + 1)
        _check(self._lib.sae_hist_files(self._ctx, xp, B, T, dt, lp, lo_exp, octaves, sub_bits, 0, fh, mh, nf, lab, n_slots, int(n_classes),
                                        sel, n_sel, lh, lc, _stream_ptr(stream)))

    # -- feature timing (include/freud_sae.h: sae_timing_files; freud_amd/feature_timing.py) -----------------------------------
    def timing_files(self, x, sub_bits: int, bridge: int, threshold_bits: int, run_hist, gap_hist, totals, n_frames, lengths=None,
                     one_chunk: bool = False, stream=None) -> None:
        """Add the run-duration and gap histograms of x [n_files, T, d] (CUDA), NB = timing_nbins(sub_bits, T), to run_hist and gap_hist
        (zero-initialised contiguous int64 CUDA [n_dict, NB]), the totals to totals (int64 CUDA [n_dict, TIMING_NTOTALS]) and the
        counted frames to n_frames (int64 CUDA [1]); bridge in [0, TIMING_MAX_BRIDGE]; a frame is active iff the bf16 magnitude bits
        of its value exceed threshold_bits; lengths: int32 CUDA tensor [n_files] or None.  The same arrays go to every call of one
        pass.  one_chunk: an L1 context walks all files of the call in one chunk per column block (another launch geometry, the same
        arrays; slower).  Asynchronous.  Afterwards the last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "timing_files", lengths)
        nb = timing_nbins(sub_bits, T)
        rh, gh = _dev("run_hist", run_hist, "int64", self.n * nb), _dev("gap_hist", gap_hist, "int64", self.n * nb)
        tt, nf = _dev("totals", totals, "int64", self.n * TIMING_NTOTALS), _dev("n_frames", n_frames, "int64", 1)
        if not 0 <= int(bridge) <= TIMING_MAX_BRIDGE:
            raise EngineError(f"bridge={bridge} outside [0, {TIMING_MAX_BRIDGE}]")
        if not 0 <= int(threshold_bits) <= 0x7F80:
            raise EngineError(f"threshold_bits={threshold_bits} outside [0, 0x7F80]")
        _check(self._lib.sae_timing_files(self._ctx, xp, B, T, dt, lp, int(sub_bits), int(bridge), int(threshold_bits),
                                          TIMING_ONE_CHUNK if one_chunk else 0, rh, gh, tt, nf, _stream_ptr(stream)))

    # -- feature manipulation (include/freud_sae.h: sae_manipulate_files; freud_amd/manipulate.py) -------------------------
    def manipulate_files(self, x, latents, ops, values, standard, manipulated, series, stream=None) -> None:
        """Edit the latents `latents` [E] (ops [E]: MANIP_OPS values) of every frame of x [n_files, T, d] (CUDA) with each row of
        values [V, E] and decode both ways, into contiguous fp32 CUDA tensors: standard (n_files * T * d elements), manipulated
        (V times that) and series (E * n_files * T: the edited latents' own values per frame).  Asynchronous.  Afterwards the
        context is as after eval(x)."""
        x, xp, B, T, d, dt, _lp = _files_args(x, "manipulate_files", None)
        lat = np.ascontiguousarray(np.asarray(latents, dtype=np.int32).reshape(-1))
        op = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1))
        val = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
        E = int(lat.size)
        if E < 1 or E > MANIP_MAX_EDITS or op.size != E:
            raise EngineError(f"manipulate_files: {E} latents and {op.size} ops; the engine takes 1 to {MANIP_MAX_EDITS} edits")
        if val.ndim != 2 or val.shape[1] != E or not 1 <= val.shape[0] <= MANIP_MAX_VARIANTS:
            raise EngineError(f"manipulate_files: values must be [1..{MANIP_MAX_VARIANTS}, {E}], got {val.shape}")
        V, M = int(val.shape[0]), B * T
        std, man = _dev("standard", standard, "float32", M * d), _dev("manipulated", manipulated, "float32", V * M * d)
        ser = _dev("series", series, "float32", E * M)
        self._note_shape(x)
        _check(self._lib.sae_manipulate_files(self._ctx, xp, B, T, dt, lat.ctypes.data_as(C.POINTER(C.c_int32)),
                                              op.ctypes.data_as(C.POINTER(C.c_int32)), E, val.ctypes.data_as(C.POINTER(C.c_float)), V, 0,
                                              std, man, ser, _stream_ptr(stream)))

    # -- reconstruction report (include/freud_sae.h: sae_recon_files; freud_amd/reconstruction.py) -------------------------
    def recon_files(self, x, block, file_out, lengths=None, resid=None, unfused: bool = False, stream=None) -> None:
        """Add the reconstruction report of x [n_files, T, d] (CUDA) to block (a zero-initialised uint8 CUDA tensor of
        recon_layout(n, d)["bytes"] bytes) and write file_out (float64 CUDA [n_files, 2]: sum r^2, sum x^2 per file) and, if given,
        resid (float32 CUDA, n_files * T * d elements: r = x - x_hat, 0 on frames that do not count); lengths: int32 CUDA tensor
        [n_files] or None.  Asynchronous.  Afterwards the last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, d, dt, lp = _files_args(x, "recon_files", lengths)
        blk = _dev("block", block, "uint8", recon_layout(self.n, self.d)["bytes"], at_least=True)
        fo = _dev("file_out", file_out, "float64", 2 * B)
        res = _dev("resid", resid, "float32", B * T * d, optional=True)
        _check(self._lib.sae_recon_files(self._ctx, xp, B, T, dt, lp, RECON_UNFUSED if unfused else 0, blk, fo, res, _stream_ptr(stream)))

    # -- dead-latent resampling (include/freud_sae.h: sae_resample_*; freud_amd/resample.py) ---------------------------------------
    def resample_files(self, x, row_loss, row0: int, fire_count, lengths=None, stream=None) -> None:
        """The row losses of x [n_files, T, d] (CUDA) into row_loss[row0 : row0 + n_files * T] (a contiguous float32 CUDA tensor over
        all rows of the pass) and its firing counts added to fire_count (zero-initialised int64 CUDA [n_dict]); lengths: int32 CUDA
        tensor [n_files] or None.  L1 contexts in bf16 precision.  Asynchronous.  Afterwards the last-forward getters fail until the
        next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "resample_files", lengths)
        row0 = int(row0)
        if row0 < 0:
            raise EngineError(f"row0={row0} is negative")
        _dev("row_loss", row_loss, "float32", row0 + B * T, at_least=True)
        fc = _dev("fire_count", fire_count, "int64", self.n)
        _check(self._lib.sae_resample_files(self._ctx, xp, B, T, dt, lp, C.c_void_p(row_loss.data_ptr() + 4 * row0), fc, _stream_ptr(stream)))

    def resample_apply(self, latents, x_rows, alpha: float, out_stats, stream=None) -> None:
        """Rewrite the columns `latents` (int32 CUDA [P]) of W, b and both Adam moments from x_rows (contiguous float32 CUDA [P, d]:
        the drawn shard rows) inside the engine; out_stats: int64 CUDA [2 + P], written ([0] revived, [1] skipped_degenerate,
        [2 + i] = 1 iff pair i was applied).  Synchronises the stream (the latents are checked on the host first)."""
        P = int(latents.numel())
        lat = _dev("latents", latents, "int32", P)                      # (its own size: the call takes the count from it)
        xr = _dev("x_rows", x_rows, "float32", P * self.d)
        st = _dev("out_stats", out_stats, "int64", 2 + P)
        _check(self._lib.sae_resample_apply(self._ctx, lat, P, xr, float(alpha), st, _stream_ptr(stream)))

    def resample_dead_latents(self, data_path: str, layer_name: str, **kw):
        """freud_amd.resample.resample_dead_latents on this engine (what train() calls for a "resample" round)."""
        from .resample import resample_dead_latents
        return resample_dead_latents(self, data_path, layer_name, **kw)

    # -- feature collection (include/freud_sae.h: sae_collect_files; freud_amd/collect_features.py) ------------------------------
    def collect_files(self, x, K: int, values, indices, stats, stream=None) -> None:
        """Write the K slots of every row of x [n_files, T, d] (CUDA) -- the first K entries of the stable descending sort of the
        latent row encode() returns -- to values (contiguous float32 CUDA, n_files * T * K elements) and indices (int64 or int32
        CUDA of the same size; its dtype chooses the form), and add the batch to stats (zero-initialised contiguous int64 CUDA [8]).
        Asynchronous.  Afterwards the last-forward getters fail until the next eval() / step()."""
        import torch
        x, xp, B, T, _d, dt, _lp = _files_args(x, "collect_files", None)
        numel = B * T * int(K)
        val, idx = _dev("values", values, "float32", numel), _dev("indices", indices, ("int64", "int32"), numel)
        st = _dev("stats", stats, "int64", 8)
        _check(self._lib.sae_collect_files(self._ctx, xp, B, T, dt, int(K), COLLECT_IDX32 if indices.dtype == torch.int32 else 0,
                                           val, idx, st, _stream_ptr(stream)))

    # -- sparsity frontier (include/freud_sae.h: sae_frontier_files; freud_amd/sparsity_frontier.py) ------------------------------
    def frontier_files(self, x, K: int, thresholds, block, lengths=None, stream=None) -> None:
        """Add the sparsity frontier of x [n_files, T, d] (CUDA) -- per counted frame the squared error after its first s slots,
        s = 0 .. K, and its budget at every threshold -- to block (a zero-initialised uint8 CUDA tensor of
        frontier_layout(len(thresholds), K, d)["bytes"] bytes); thresholds: up to FRONTIER_MAX_TAU floats inside (0, 1); lengths:
        int32 CUDA tensor [n_files] or None.  Asynchronous.  Afterwards the last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "frontier_files", lengths)
        tau = _tau_arg("frontier_files", thresholds, FRONTIER_MAX_TAU)
        K = int(K)
        blk = _dev("block", block, "uint8", frontier_layout(tau.size, max(K, 0), self.d)["bytes"], at_least=True)
        _check(self._lib.sae_frontier_files(self._ctx, xp, B, T, dt, lp, K, tau.ctypes.data_as(_fptr), int(tau.size), 0, blk,
                                            _stream_ptr(stream)))

    # -- pursuit frontier (include/freud_sae.h: sae_pursuit_files; freud_amd/pursuit.py) ------------------------------------------
    def pursuit_files(self, x, K: int, thresholds, block, lengths=None, trace=None, stream=None) -> None:
        """Add the pursuit frontier of x [n_files, T, d] (CUDA) -- every counted frame coded by K steps of non-negative matching pursuit
        on the decoder directions -- to block (a zero-initialised uint8 CUDA tensor of pursuit_layout(len(thresholds), K, d, n)["bytes"]
        bytes); thresholds: up to PURSUIT_MAX_TAU floats inside (0, 1); lengths: int32 CUDA tensor [n_files] or None; trace: None or
        three contiguous CUDA tensors (idx int32 [n_files * T * K], val float32 of the same size, err float32 [n_files * T * (K + 1)])
        that receive this batch's pursuit code in pick order.  Asynchronous.  Afterwards the last-forward getters fail until the next
        eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "pursuit_files", lengths)
        tau = _tau_arg("pursuit_files", thresholds, PURSUIT_MAX_TAU)
        K = int(K)
        blk = _dev("block", block, "uint8", pursuit_layout(tau.size, max(K, 0), self.d, self.n)["bytes"], at_least=True)
        ti = tv = te = None
        if trace is not None:
            idx, val, err = trace
            rows = B * T
            ti = _dev("trace idx", idx, "int32", rows * max(K, 0))
            tv = _dev("trace val", val, "float32", rows * max(K, 0))
            te = _dev("trace err", err, "float32", rows * (max(K, 0) + 1))
        _check(self._lib.sae_pursuit_files(self._ctx, xp, B, T, dt, lp, K, tau.ctypes.data_as(_fptr), int(tau.size), 0, blk, ti, tv, te,
                                           _stream_ptr(stream)))

    # -- refit frontier (include/freud_sae.h: sae_refit_files; freud_amd/refit.py) ------------------------------------------------
    def refit_files(self, x, K: int, thresholds, block, lengths=None, support=None, trace=None, stream=None) -> None:
        """Add the refit frontier of x [n_files, T, d] (CUDA) -- every counted frame's least-squares error on every prefix of its
        support's K slots -- to block (a zero-initialised uint8 CUDA tensor of refit_layout(len(thresholds), K, d, n)["bytes"] bytes);
        thresholds: up to REFIT_MAX_TAU floats inside (0, 1); lengths: int32 CUDA tensor [n_files] or None; support: None (the slots of
        collect_files) or a contiguous int32 CUDA tensor of n_files * T * K indices (-1: an empty slot); trace: None or a dict with any
        of "coef" (float32, n_files * T * K), "err" (float32, n_files * T * (K + 1)), "dep" (uint8, n_files * T * K) and "gram"
        (float32, n_files * T * (K + 1) * K), contiguous CUDA tensors that receive this batch's rows.  Asynchronous.  Afterwards the
        last-forward getters fail until the next eval() / step()."""
        x, xp, B, T, _d, dt, lp = _files_args(x, "refit_files", lengths)
        tau = _tau_arg("refit_files", thresholds, REFIT_MAX_TAU)
        K = int(K)
        Kc, rows = max(K, 0), B * T
        blk = _dev("block", block, "uint8", refit_layout(tau.size, Kc, self.d, self.n)["bytes"], at_least=True)
        sup = None if support is None else _dev("support", support, "int32", rows * Kc)
        trace = dict(trace or {})
        unknown = set(trace) - {"coef", "err", "dep", "gram"}
        if unknown:
            raise EngineError(f"refit_files: unknown trace arrays {sorted(unknown)}")
        tc = _dev("trace coef", trace["coef"], "float32", rows * Kc) if trace.get("coef") is not None else None
        te = _dev("trace err", trace["err"], "float32", rows * (Kc + 1)) if trace.get("err") is not None else None
        td = _dev("trace dep", trace["dep"], "uint8", rows * Kc) if trace.get("dep") is not None else None
        tg = _dev("trace gram", trace["gram"], "float32", rows * (Kc + 1) * Kc) if trace.get("gram") is not None else None
        _check(self._lib.sae_refit_files(self._ctx, xp, B, T, dt, lp, K, tau.ctypes.data_as(_fptr), int(tau.size), 0, sup, blk, tc, te, td, tg,
                                         _stream_ptr(stream)))

    # -- inspection -----------------------------------------------------------------------------
    def debug_read(self, which: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=np.float32)
        _check(self._lib.sae_debug_read(self._ctx, which, out.ctypes.data_as(C.POINTER(C.c_float)), count))
        return out

    def l1_backward_plan(self, M: int) -> dict:
        """L1, bf16 contexts: how the weight gradient of a batch of M rows would be launched (nothing runs)."""
        out = (_i32 * 8)()
        _check(self._lib.sae_l1_backward_plan(self._ctx, int(M), out))
        keys = ("form", "splits", "balanced", "bal_m", "bal_q", "grid", "steps", "ntiles")
        return {k: int(v) for k, v in zip(keys, out)}

    def profile(self, level: int, period: Optional[int] = None) -> None:
        """level 1 brackets the dominant kernel with HIP events on every `period`-th step (default 8)."""
        if period is not None:
            _check(self._lib.sae_profile_period(self._ctx, int(period)))
        _check(self._lib.sae_profile(self._ctx, level))

    def kernel_times(self) -> Dict[str, tuple]:
        n = 48
        ms = (C.c_float * n)()
        cnt = (C.c_int32 * n)()
        _check(self._lib.sae_kernel_times(self._ctx, ms, cnt, n))
        out = {}
        for i in range(n):
            name = self._lib.sae_kernel_name(i)
            if name is None:
                break
            out[name.decode()] = (float(ms[i]), int(cnt[i]))
        return out

    def dominant_kernel(self) -> str:
        return self._lib.sae_kernel_name(self._lib.sae_dominant_kernel(self._ctx)).decode()


# -- the device-tensor arguments, and feature search without a context (raw mode, merge, per-file values) ------------------------------
_TORCH_DTYPES = {}      # _dev's dtype argument -> the torch dtypes it names, filled on first use (torch is not imported up here)


def _torch_dtypes(dtype) -> tuple:
    import torch
    _TORCH_DTYPES[dtype] = tuple(getattr(torch, s) for s in (dtype if isinstance(dtype, tuple) else (dtype,)))
    return _TORCH_DTYPES[dtype]


def _dev(name: str, t, dtype, numel: int, *, at_least: bool = False, optional: bool = False):
    """The one check of a device-tensor argument: t must be a contiguous CUDA tensor of `dtype` (a torch dtype's name, or a tuple of
    names) with exactly numel elements (at_least: numel or more) -> its pointer as void*.  optional: None passes, as None.  A size
    rule that lets a short tensor through is a device over-write, so every caller states here which of the two it means."""
    if t is None and optional:
        return None
    want = _TORCH_DTYPES.get(dtype) or _torch_dtypes(dtype)
    if not (t is not None and t.is_cuda and t.dtype in want and t.is_contiguous()
            and (t.numel() >= numel if at_least else t.numel() == numel)):
        names = " or ".join(dtype if isinstance(dtype, tuple) else (dtype,))
        raise EngineError(f"{name} must be a contiguous {names} CUDA tensor of {'>= ' if at_least else ''}{numel} elements")
    return C.c_void_p(t.data_ptr())


def _labels_arg(labels, B: int, T: int):
    """The labels of label_files / hist_files, a contiguous int32 CUDA tensor [B, T, n_slots] -> (its pointer, n_slots)."""
    import torch
    if not (labels is not None and labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and labels.dim() == 3
            and tuple(labels.shape[:2]) == (B, T)):
        raise EngineError(f"labels must be a contiguous int32 CUDA tensor [{B}, {T}, n_slots]")
    return C.c_void_p(labels.data_ptr()), int(labels.shape[2])


def _label_table(counts, label_count, n_classes: int, n: int):
    """The label table of label_files / label_keys -> (counts pointer, label_count pointer)."""
    rows = int(n_classes) + 1
    return _dev("counts", counts, "int32", rows * n), _dev("label_count", label_count, "int64", rows)


def _alias(ptr: int, shape: tuple, typestr: str, device):
    """A torch CUDA tensor over `shape` elements of `typestr` (as in __cuda_array_interface__) of the engine's HBM at ptr: no copy."""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}

    return torch.as_tensor(_View(), device=device)


def _stream_ptr(stream=None):
    import torch
    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def _files_args(x, who: str, lengths):
    """The shared front of search_files / stats_files / search_raw_files: x [n_files, T, d] and the files' lengths ->
    (x kept alive, its pointer, n_files, T, d, dtype code, lengths pointer or None)."""
    if x.dim() != 3:
        raise EngineError(f"{who} expects x as [n_files, T, d], got {tuple(x.shape)}")
    B, T, d = (int(v) for v in x.shape)
    lp = _dev("lengths", lengths, "int32", B, optional=True)
    x, ptr, _rows, dt = SaeEngine._x_args(x)
    return x, C.c_void_p(ptr), B, T, d, dt, lp


def search_raw_files(x, file_keys, aux=None, lengths=None, absolute: bool = False, stream=None) -> None:
    """Raw mode (no SAE): per-(file, column) keys of x [n_files, T, d] itself; with absolute, aux gets the abs-mode side words."""
    x, xp, B, T, d, dt, lp = _files_args(x, "search_raw_files", lengths)
    keys = _dev("file_keys", file_keys, "int64", B * d, at_least=True)
    side = _dev("aux", aux, "int64", B * d, at_least=True) if absolute else None
    _check(load().sae_search_raw_files(xp, B, T, d, dt, lp, int(absolute), keys, side, _stream_ptr(stream)))


def search_merge(file_keys, aux, n_files: int, ncols: int, file0: int, n_top: int, flags: int, min_val: float, max_val: float,
                 top_keys, top_frames, stream=None) -> None:
    keys = _dev("file_keys", file_keys, "int64", n_files * ncols, at_least=True)
    side = _dev("aux", aux, "int64", n_files * ncols, at_least=True, optional=True)
    tk = _dev("top_keys", top_keys, "int64", n_top * ncols, at_least=True)
    tf = _dev("top_frames", top_frames, "int32", n_top * ncols, at_least=True)
    _check(load().sae_search_merge(keys, side, int(n_files), int(ncols), int(file0), int(n_top), int(flags), float(min_val), float(max_val),
                                   tk, tf, _stream_ptr(stream)))


# -- dead-latent resampling without a context (include/freud_sae.h: sae_resample_select) ------------------------------------------------
def resample_workspace_bytes(rows: int, n: int) -> int:
    """Bytes of workspace that resample_select needs for `rows` row losses and n latents."""
    nbytes = int(load().sae_resample_workspace_bytes(int(rows), int(n)))
    if nbytes < 0:
        raise EngineError(f"resample_workspace_bytes: rows={rows} outside [1, 2^31) or n={n} outside [1, 2^24]")
    return nbytes


def resample_select(row_loss, rows: int, fire_count, n: int, seed: int, round: int, latents_out, rows_out, counts_out, workspace,
                    stream=None) -> None:
    """The applying (dead latent, row) pairs of row_loss (float32 CUDA, >= rows) and fire_count (int64 CUDA [n]) for (seed, round), in
    ascending latent order into latents_out (int32 CUDA [n]) / rows_out (int64 CUDA [n]); counts_out: int64 CUDA [RESAMPLE_NCOUNTS];
    workspace: a uint8 CUDA tensor of >= resample_workspace_bytes(rows, n).  Asynchronous."""
    rl = _dev("row_loss", row_loss, "float32", int(rows), at_least=True)
    fc = _dev("fire_count", fire_count, "int64", int(n))
    lo, ro = _dev("latents_out", latents_out, "int32", int(n)), _dev("rows_out", rows_out, "int64", int(n))
    co = _dev("counts_out", counts_out, "int64", RESAMPLE_NCOUNTS)
    ws = _dev("workspace", workspace, "uint8", resample_workspace_bytes(rows, n), at_least=True)
    _check(load().sae_resample_select(rl, int(rows), fc, int(n), int(seed) & (2 ** 64 - 1), int(round) & (2 ** 64 - 1), lo, ro, co, ws,
                                      int(workspace.numel()), _stream_ptr(stream)))


# -- input statistics without a context (include/freud_sae.h: sae_input_*; freud_amd/input_stats.py) --------------------------------
def input_stats_workspace_bytes(n_files: int, T: int, d: int) -> int:
    """Bytes of workspace that input_moments / input_median need for a sample [n_files, T, d]."""
    nbytes = int(load().sae_input_stats_workspace_bytes(int(n_files), int(T), int(d)))
    if nbytes < 0:
        raise EngineError(f"input_stats_workspace_bytes: n_files={n_files}, T={T} or d={d} (1 <= d <= {INPUT_MAX_D}) out of range")
    return nbytes


def _input_args(x, who: str, lengths, workspace):
    x, xp, B, T, d, dt, lp = _files_args(x, who, lengths)
    if d > INPUT_MAX_D:
        raise EngineError(f"{who}: d={d} > {INPUT_MAX_D}")
    ws = _dev("workspace", workspace, "uint8", input_stats_workspace_bytes(B, T, d), at_least=True)
    return x, xp, B, T, d, dt, lp, ws


def input_moments(x, out, workspace, lengths=None, stream=None) -> None:
    """The moments of the sample x [n_files, T, d]: out (float64 CUDA [4 d + 2]) = mean | centred sum of squares | min | max |
    sum |x|^2 | N.  workspace: a uint8 CUDA tensor of >= input_stats_workspace_bytes(n_files, T, d).  Asynchronous."""
    x, xp, B, T, d, dt, lp, ws = _input_args(x, "input_moments", lengths, workspace)
    o = _dev("out", out, "float64", 4 * d + 2)
    _check(load().sae_input_moments(xp, B, T, d, dt, lp, o, ws, int(workspace.numel()), _stream_ptr(stream)))


def input_median(x, start, floor: float, iterations: int, path, objective, workspace, lengths=None, stream=None) -> None:
    """Weiszfeld's iteration on the sample x [n_files, T, d] from start (float64 CUDA [d]): path (float64 CUDA [iterations + 1, d]) =
    m_0 .. m_I, objective (float64 CUDA [iterations + 1]) = J_0 .. J_I.  Asynchronous."""
    x, xp, B, T, d, dt, lp, ws = _input_args(x, "input_median", lengths, workspace)
    iterations = int(iterations)
    if iterations < 1 or iterations > INPUT_MAX_ITERATIONS:
        raise EngineError(f"input_median: iterations={iterations} outside [1, {INPUT_MAX_ITERATIONS}]")
    st = _dev("start", start, "float64", d)
    pa = _dev("path", path, "float64", (iterations + 1) * d)
    ob = _dev("objective", objective, "float64", iterations + 1)
    _check(load().sae_input_median(xp, B, T, d, dt, lp, st, float(floor), iterations, pa, ob, ws, int(workspace.numel()),
                                   _stream_ptr(stream)))


# -- input covariance without a context (include/freud_sae.h: sae_input_cov*; freud_amd/input_pca.py) --------------------------------
def input_cov_workspace_bytes(n_files: int, T: int, d: int) -> int:
    """Bytes of workspace that input_cov needs for a sample [n_files, T, d]."""
    nbytes = int(load().sae_input_cov_workspace_bytes(int(n_files), int(T), int(d)))
    if nbytes < 0:
        raise EngineError(f"input_cov_workspace_bytes: n_files={n_files}, T={T} or d={d} (1 <= d <= {INPUT_MAX_D}) out of range")
    return nbytes


def input_cov_plan(n_files: int, T: int, d: int) -> dict:
    """The decomposition input_cov uses for a sample [n_files, T, d]: {"tile", "tiles", "segments", "units_per_segment"}."""
    out = (_i64 * 4)()
    _check(load().sae_input_cov_plan(int(n_files), int(T), int(d), out))
    return dict(zip(("tile", "tiles", "segments", "units_per_segment"), (int(v) for v in out)))


def input_cov(x, out, workspace, center=None, lengths=None, stream=None) -> None:
    """The centred scatter of the sample x [n_files, T, d]: out (float64 CUDA [d, d]) = sum_k a_k a_k^T, a_k = double(x_k) - center
    over the counted frames (center: float64 CUDA [d] or None = zeros), not divided by N.  workspace: a uint8 CUDA tensor of >=
    input_cov_workspace_bytes(n_files, T, d).  Asynchronous."""
    x, xp, B, T, d, dt, lp = _files_args(x, "input_cov", lengths)
    if d > INPUT_MAX_D:
        raise EngineError(f"input_cov: d={d} > {INPUT_MAX_D}")
    ws = _dev("workspace", workspace, "uint8", input_cov_workspace_bytes(B, T, d), at_least=True)
    o = _dev("out", out, "float64", d * d)
    c = _dev("center", center, "float64", d) if center is not None else None
    _check(load().sae_input_cov(xp, B, T, d, dt, lp, c, o, ws, int(workspace.numel()), _stream_ptr(stream)))


# -- feature index (include/freud_sae.h: sae_findex_*; freud_amd/feature_index.py) ---------------------------------------------------
def _findex_batch(values, indices):
    import torch
    if not (values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.dim() == 2):
        raise EngineError("values must be a contiguous float32 CUDA tensor [rows, K]")
    if indices.dtype not in (torch.int32, torch.int64):
        raise EngineError(f"indices must be int32 or int64, got {indices.dtype}")
    if not (indices.is_cuda and indices.is_contiguous() and tuple(indices.shape) == tuple(values.shape) and indices.device == values.device):
        raise EngineError(f"indices must be a contiguous CUDA tensor of the values' shape {tuple(values.shape)}")
    rows, K = (int(v) for v in values.shape)
    return rows, K, FINDEX_IDX32 if indices.dtype == torch.int32 else 0


def findex_workspace_bytes(max_rows: int, n_range: int) -> int:
    """Bytes of workspace that findex_fill needs for batches of at most max_rows rows and a range of n_range latents."""
    nbytes = int(load().sae_findex_workspace_bytes(int(max_rows), int(n_range)))
    if nbytes < 0:
        raise EngineError(f"findex_workspace_bytes: max_rows={max_rows}, n_range={n_range} out of range")
    return nbytes


def findex_count(values, indices, n_dict: int, totals, stats, stream=None) -> None:
    """Sweep 1 of the feature index: totals int64 [n_dict] += the batch's posted slots per latent, stats int64 [FINDEX_NSTATS] += the
    tallies (FINDEX_STAT_NAMES)."""
    rows, K, flags = _findex_batch(values, indices)
    tot, st = _dev("totals", totals, "int64", int(n_dict)), _dev("stats", stats, "int64", FINDEX_NSTATS)
    _check(load().sae_findex_count(C.c_void_p(values.data_ptr()), C.c_void_p(indices.data_ptr()), rows, K, flags, int(n_dict), tot, st,
                                   _stream_ptr(stream)))


def findex_fill(values, indices, n_dict: int, j0: int, j1: int, pos0: int, cursor, out_base: int, positions_out, values_out, workspace,
                err, stream=None) -> None:
    """Sweep 2: the batch's posted slots of the latents [j0, j1) written behind each list's cursor (int64 [n_dict], absolute, advanced
    by the call) into positions_out (int32 holding uint32) / values_out (float32), whose element 0 is absolute slot out_base;
    workspace: a uint8 tensor of >= findex_workspace_bytes(rows, j1 - j0); err int64 [2]."""
    import torch
    rows, K, flags = _findex_batch(values, indices)
    cur, er = _dev("cursor", cursor, "int64", int(n_dict)), _dev("err", err, "int64", 2)
    if not (positions_out.is_cuda and positions_out.dtype == torch.int32 and positions_out.is_contiguous() and positions_out.dim() == 1):
        raise EngineError("positions_out must be a contiguous 1-D int32 CUDA tensor (it holds the uint32 position words)")
    vo = _dev("values_out", values_out, "float32", positions_out.numel())
    need = findex_workspace_bytes(rows, int(j1) - int(j0)) if 0 <= int(j0) < int(j1) else 0
    ws = _dev("workspace", workspace, "uint8", need, at_least=True)
    _check(load().sae_findex_fill(C.c_void_p(values.data_ptr()), C.c_void_p(indices.data_ptr()), rows, K, flags, int(n_dict), int(j0),
                                  int(j1), int(pos0), cur, int(out_base), C.c_void_p(positions_out.data_ptr()), vo,
                                  int(positions_out.numel()), ws, int(workspace.numel()), er, _stream_ptr(stream)))


def findex_verify(starts, j0: int, j1: int, out_base: int, positions, limit: int, err, stream=None) -> None:
    """err[0] += the slots of the finished lists [j0, j1) (starts int64 [n_dict + 1], absolute; positions as findex_fill wrote them)
    whose position is not strictly greater than its predecessor's in the list, or is >= limit."""
    import torch
    if not (starts.is_cuda and starts.dtype == torch.int64 and starts.is_contiguous() and starts.dim() == 1 and starts.numel() >= 2):
        raise EngineError("starts must be a contiguous 1-D int64 CUDA tensor [n_dict + 1]")
    er = _dev("err", err, "int64", 2)
    if not (positions.is_cuda and positions.dtype == torch.int32 and positions.is_contiguous() and positions.dim() == 1):
        raise EngineError("positions must be a contiguous 1-D int32 CUDA tensor")
    _check(load().sae_findex_verify(C.c_void_p(starts.data_ptr()), int(starts.numel()) - 1, int(j0), int(j1), int(out_base),
                                    C.c_void_p(positions.data_ptr()), int(positions.numel()), int(limit), er, _stream_ptr(stream)))


def file_top_features(file_keys, n_files: int, ncols: int, n_top: int, flags: int, top_latents, top_keys, stream=None) -> None:
    """Per file the n_top best latents of file_keys [n_files, ncols] (as search_files / search_raw_files leave them) into
    top_latents (int32, -1 = empty) and top_keys (int64 holding the uint64 file keys, 0 = empty), both [n_files, n_top]."""
    keys = _dev("file_keys", file_keys, "int64", n_files * ncols, at_least=True)
    tk = _dev("top_keys", top_keys, "int64", n_files * n_top, at_least=True)
    tl = _dev("top_latents", top_latents, "int32", n_files * n_top, at_least=True)
    _check(load().sae_file_top_features(keys, int(n_files), int(ncols), int(n_top), int(flags), tl, tk, _stream_ptr(stream)))


def coact_neighbor_keys(counts, n: int, row0: int, n_rows: int, measure: int, keys, stream=None) -> None:
    """keys [n_rows, n] (int64 holding uint64) = the neighbour keys of rows [row0, row0 + n_rows) of the count table counts [n, n]
    for file_top_features(keys, n_rows, n, n_top, FILE_TOP_POSITIVE, ...); measure: a COACT_MEASURES value."""
    table = _dev("counts", counts, "int32", n * n)
    out = _dev("keys", keys, "int64", max(int(n_rows), 0) * n, at_least=True)
    _check(load().sae_coact_neighbor_keys(table, int(n), int(row0), int(n_rows), int(measure), out, _stream_ptr(stream)))


def label_keys(counts, label_count, n_classes: int, n: int, measure: int, by_latent: int, row0: int, n_rows: int, keys, stream=None) -> None:
    """keys (int64 holding uint64) = the keys of rows [row0, row0 + n_rows) of the label table counts [n_classes + 1, n] /
    label_count [n_classes + 1]: [n_rows, n] (by_latent 0: a row is a label) or [n_rows, n_classes] (1: a row is a latent), for
    file_top_features(keys, n_rows, columns, n_top, FILE_TOP_POSITIVE, ...); measure: a LABEL_MEASURES value."""
    table, lc = _label_table(counts, label_count, n_classes, n)
    out = _dev("keys", keys, "int64", max(int(n_rows), 0) * (int(n_classes) if by_latent else n), at_least=True)
    _check(load().sae_label_keys(table, lc, int(n_classes), int(n), int(measure), int(by_latent), int(row0), int(n_rows), out,
                                 _stream_ptr(stream)))


def cross_mask_bytes(n: int, rows: int) -> int:
    """Bytes of one activity mask of a dictionary of n latents over `rows` frames (include/freud_sae.h, sae_cross_mask_bytes)."""
    b = int(load().sae_cross_mask_bytes(int(n), int(rows)))
    if b <= 0:
        raise EngineError(f"n={n} outside [1, 2^21] or rows={rows} outside [1, {65535 * 128}]")
    return b


def cross_update(mask_a, n_a: int, mask_b, n_b: int, rows: int, counts, stream=None) -> None:
    """counts (contiguous int32 CUDA [n_a + 1, n_b + 1]) += mask_a x mask_b^T: a source mask of A and a target mask of B as
    cross_mask_files wrote them for the same batch of `rows` frames (contiguous int8 / uint8 CUDA tensors of cross_mask_bytes)."""
    a = _dev("mask_a", mask_a, ("int8", "uint8"), cross_mask_bytes(n_a, rows), at_least=True)
    b = _dev("mask_b", mask_b, ("int8", "uint8"), cross_mask_bytes(n_b, rows), at_least=True)
    table = _dev("counts", counts, "int32", (int(n_a) + 1) * (int(n_b) + 1))
    _check(load().sae_cross_update(a, int(n_a), b, int(n_b), int(rows), table, _stream_ptr(stream)))


def cross_keys(counts, n_a: int, n_b: int, measure: int, by_b: int, exclude_diagonal: int, row0: int, n_rows: int, keys, stream=None) -> None:
    """keys (int64 holding uint64) = the keys of rows [row0, row0 + n_rows) of the cross-activation table counts [n_a + 1, n_b + 1]:
    [n_rows, n_b] (by_b 0: a row is a latent of A) or [n_rows, n_a] (1: a row is a latent of B), for
    file_top_features(keys, n_rows, columns, n_top, FILE_TOP_POSITIVE, ...); measure: a CROSS_MEASURES value."""
    table = _dev("counts", counts, "int32", (int(n_a) + 1) * (int(n_b) + 1))
    out = _dev("keys", keys, "int64", max(int(n_rows), 0) * int(n_a if by_b else n_b), at_least=True)
    _check(load().sae_cross_keys(table, int(n_a), int(n_b), int(measure), int(by_b), int(exclude_diagonal), int(row0), int(n_rows), out,
                                 _stream_ptr(stream)))


def dict_pack_bytes(n: int, d: int) -> int:
    """Bytes of the packed operand of a dictionary of n directions of length d (include/freud_sae.h, sae_dict_pack)."""
    b = int(load().sae_dict_pack_bytes(int(n), int(d)))
    if b <= 0:
        raise EngineError(f"n={n} outside [1, 2^24] or d={d} outside [1, {DICT_MAX_D}]")
    return b


def _packed(name: str, t, n: int, d: int):
    """A packed dictionary operand: a contiguous CUDA tensor of any dtype that holds dict_pack_bytes(n, d) bytes -> its pointer."""
    if not (t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= dict_pack_bytes(n, d)):
        raise EngineError(f"{name} must be a contiguous CUDA tensor of >= {dict_pack_bytes(n, d)} bytes")
    return C.c_void_p(t.data_ptr())


def dict_pack(w, n: int, d: int, dir_stride: int, elem_stride: int, side: int, packed, norms, stream=None) -> None:
    """The unit directions of w (fp32 CUDA; direction i, element e at w.data_ptr() + 4 (i dir_stride + e elem_stride), all inside its
    storage) as the split bf16 GEMM operand `packed` (a CUDA tensor of >= dict_pack_bytes(n, d) bytes) and norms [n] (fp32)."""
    import torch
    n, d, dir_stride, elem_stride = int(n), int(d), int(dir_stride), int(elem_stride)
    if not (w.is_cuda and w.dtype == torch.float32):
        raise EngineError("the directions must be a float32 CUDA tensor")
    if n >= 1 and d >= 1 and dir_stride >= 1 and elem_stride >= 1:
        last = w.storage_offset() + (n - 1) * dir_stride + (d - 1) * elem_stride
        if last >= w.untyped_storage().nbytes() // 4:
            raise EngineError(f"{n} directions of length {d} with strides ({dir_stride}, {elem_stride}) reach past the tensor's storage")
    pk, nr = _packed("packed", packed, n, d), _dev("norms", norms, "float32", n, at_least=True)
    _check(load().sae_dict_pack(C.c_void_p(w.data_ptr()), n, d, dir_stride, elem_stride, int(side), pk, nr, _stream_ptr(stream)))


def dict_sim_keys(packed_a, n_a: int, packed_b, n_b: int, d: int, row0: int, n_rows: int, self_mode: bool, keys, stream=None) -> None:
    """keys [n_rows, n_b] (int64 holding uint64) = the cosine keys of the directions [row0, row0 + n_rows) of A against all of B, from
    their packed operands (dict_pack with DICT_LEFT / DICT_RIGHT), for file_top_features(keys, n_rows, n_b, n_top, 0, ...)."""
    pa, pb = _packed("packed_a", packed_a, n_a, d), _packed("packed_b", packed_b, n_b, d)
    out = _dev("keys", keys, "int64", max(int(n_rows), 0) * int(n_b), at_least=True)
    _check(load().sae_dict_sim_keys(pa, int(n_a), pb, int(n_b), int(d), int(row0), int(n_rows), int(bool(self_mode)), out,
                                    _stream_ptr(stream)))


def store_piece_bytes() -> int:
    """Bytes of a row that one workgroup of store_gather copies (include/freud_sae.h, sae_store_piece_bytes)."""
    return int(load().sae_store_piece_bytes())


def store_convert(src, dst, stream=None) -> None:
    """dst (bfloat16 CUDA, contiguous) = src (float32 CUDA, contiguous, as many elements) by the loader's conversion rule
    (include/freud_sae.h, sae_store_convert)."""
    n = int(src.numel())
    _check(load().sae_store_convert(_dev("src", src, "float32", n), _dev("dst", dst, ("bfloat16", "int16"), n), n, _stream_ptr(stream)))


def store_gather(store, idx, out, err, stream=None) -> None:
    """out[j] = store[idx[j]] for j < len(idx) (include/freud_sae.h, sae_store_gather): store [n_files, row] a contiguous CUDA tensor,
    idx a contiguous int32 CUDA vector, out [>= len(idx), row] a CUDA tensor of the store's dtype whose rows are contiguous (its row
    stride may exceed the row), err one int32 on the device -- incremented per index outside the store, never cleared here."""
    import torch
    if not (store.is_cuda and store.dim() == 2 and store.is_contiguous() and store.shape[0] >= 1 and store.shape[1] >= 1):
        raise EngineError("store must be a contiguous CUDA tensor [n_files, row] with n_files, row >= 1")
    nb = int(idx.numel())
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.dim() == 1 and idx.is_contiguous()):
        raise EngineError("idx must be a contiguous int32 CUDA vector")
    row = int(store.shape[1])
    if not (out.is_cuda and out.dtype == store.dtype and out.dim() == 2 and out.shape[0] >= nb and out.shape[1] == row
            and (out.stride(1) == 1 or row == 1) and (out.stride(0) >= row or out.shape[0] <= 1)):
        raise EngineError(f"out must be a {store.dtype} CUDA tensor [>= {nb}, {row}] with contiguous rows")
    es = store.element_size()
    stride = int(out.stride(0)) if out.shape[0] > 1 else row
    _check(load().sae_store_gather(C.c_void_p(store.data_ptr()), int(store.shape[0]), row * es, C.c_void_p(idx.data_ptr()), nb,
                                   C.c_void_p(out.data_ptr()), stride * es, _dev("err", err, "int32", 1), _stream_ptr(stream)))


def store_gather_frames(store, T: int, prefix, n_frames: int, key: int, pos0: int, pos_stride: int, out, err, ordinals=None,
                        stream=None) -> None:
    """out[j] = the frame that position pos0 + j * pos_stride of the epoch `key` holds, for j < out.shape[0] (include/freud_sae.h,
    sae_store_gather_frames): store [n_files, T * d] a contiguous CUDA tensor, prefix None (untrimmed) or a contiguous int64 CUDA
    vector [n_files + 1] (the exclusive prefix sum of the trimmed lengths), n_frames the counted frames, key any integer (taken mod
    2^64), out [rows, d] a CUDA tensor of the store's dtype whose rows are contiguous (its row stride may exceed d), err one int32 on
    the device -- incremented per frame a malformed prefix placed outside the store, never cleared here --, ordinals None or a
    contiguous int64 CUDA vector [rows] that receives every row's index into store.view(n_files * T, d)."""
    T = int(T)
    if not (store.is_cuda and store.dim() == 2 and store.is_contiguous() and store.shape[0] >= 1 and T >= 1 and store.shape[1] >= T
            and store.shape[1] % T == 0):
        raise EngineError("store must be a contiguous CUDA tensor [n_files, T * d] with n_files, T, d >= 1")
    n_files, d = int(store.shape[0]), int(store.shape[1]) // T
    if not (out.is_cuda and out.dtype == store.dtype and out.dim() == 2 and out.shape[1] == d and (out.stride(1) == 1 or d == 1)
            and (out.stride(0) >= d or out.shape[0] <= 1)):
        raise EngineError(f"out must be a {store.dtype} CUDA tensor [rows, {d}] with contiguous rows")
    rows = int(out.shape[0])
    es = store.element_size()
    stride = int(out.stride(0)) if rows > 1 else d
    _check(load().sae_store_gather_frames(C.c_void_p(store.data_ptr()), n_files, T, d * es, _dev("prefix", prefix, "int64", n_files + 1, optional=True),
                                          int(n_frames), int(key) & (2 ** 64 - 1), int(pos0), int(pos_stride), rows, C.c_void_p(out.data_ptr()),
                                          stride * es, _dev("ordinals", ordinals, "int64", rows, optional=True), _dev("err", err, "int32", 1),
                                          _stream_ptr(stream)))


def search_file_values(file_keys, aux, n_files: int, ncols: int, flags: int, latents, file0: int, out, stream=None) -> None:
    import torch
    keys = _dev("file_keys", file_keys, "int64", n_files * ncols, at_least=True)
    side = _dev("aux", aux, "int64", n_files * ncols, at_least=True, optional=True)
    lat = _dev("latents", latents, "int32", int(latents.numel()))       # (its own size: the call takes the count from it)
    if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.is_contiguous() and out.shape[0] >= latents.numel()):
        raise EngineError(f"out must be a contiguous float32 CUDA tensor [>= {latents.numel()}, files]")
    _check(load().sae_search_file_values(keys, side, int(n_files), int(ncols), int(flags), lat, int(latents.numel()), int(file0),
                                         int(out.shape[1]), C.c_void_p(out.data_ptr()), _stream_ptr(stream)))
