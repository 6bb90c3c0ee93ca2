"""ctypes binding of libnwhip.so (include/nw_hip.h) -- the MI355X NW fill.

This is the Python-side mirror of the reference's fill plugin interface
(`needlemanWunsch(dnaArray s1, dnaArray s2, int* t)`, src/serial/serial.cpp:4):
`fill(s1, s2)` returns the full (n2+1) x (n1+1) int32 table in the reference
layout, `score(s1, s2)` only t[n2][n1] (what src/common/driver.cpp:35 prints).
Device-resident variants take torch tensors and never leave HBM.

There is no CPU fallback: if build/libnwhip.so is missing or no gfx950 device is
visible, every call raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# NWHIP_LIB selects an alternative in-tree build (tuning variants from `make variant`)
LIB_PATH = os.environ.get("NWHIP_LIB") or os.path.join(HERE, "build", "libnwhip.so")

NW_OK, NW_ERR_ARG, NW_ERR_HIP, NW_ERR_OOM, NW_ERR_TIMEOUT, NW_ERR_NODEVICE, NW_ERR_UNSUPPORTED = range(7)
NW_ERR_TABLE = 7  # traceback: a cell no move reproduces (not a table of these parameters)
MODE_NW, MODE_SW = 0, 1  # nw_params.mode: global (the reference fills) / Smith-Waterman local
# nw_params.kernel: auto / anti-diagonal strips (nw_fill.hip) / row-scan panels (nw_rows.hip)
KERNEL_AUTO, KERNEL_STRIPS, KERNEL_PANELS = 0, 1, 2
# the `ends` of the semi-global batch entries (NW_ENDS_*): which end gaps are free
ENDS_S1_BEGIN, ENDS_S1_END, ENDS_S2_BEGIN, ENDS_S2_END = 1, 2, 4, 8
ENDS_GLOBAL, ENDS_S2_IN_S1, ENDS_S1_IN_S2, ENDS_OVERLAP = 0, 3, 12, 15

# every symbol include/nw_hip.h declares (checked by tests/test_host.py)
EXPORTS = ["nw_params_default", "nw_strerror", "nw_version", "nw_fill", "nw_table_pitch",
           "nw_table_bytes", "nw_table_offset", "nw_strip_lds_bytes", "nw_panel_lds_bytes", "nw_ctx_create", "nw_ctx_destroy", "nw_ctx_workspace_bytes",
           "nw_fill_device", "nw_fill_device_async", "nw_ctx_status", "nw_read_bdna", "nw_free",
           "nw_synth_bdna", "nw_band_layout", "nw_halo_bytes", "nw_fill_band_async",
           "nw_ipc_get_handle", "nw_ipc_open_handle", "nw_ipc_close_handle", "nw_halo_alloc",
           "nw_halo_free", "nw_fill_emb", "nw_sw_align", "nw_sw_traceback", "nw_tuned_shape", "nw_auto_shape", "nw_debug_ctrl", "nw_debug_set_trace",
           "nw_debug_trace_words", "nw_colband_layout", "nw_feed_bytes", "nw_feed_alloc",
           "nw_fill_colband_async", "nw_link_alloc", "nw_link_wait_async", "nw_link_signal_async",
           "nw_link_status", "nw_host_warmup", "nw_host_release", "nw_halo_alloc_regions",
           "nw_fill_band_cycle_async", "nw_fill_tband_async", "nw_link_wait_ctx_async", "nw_debug_failure",
           "nw_traceback", "nw_align", "nw_ops_expand", "nw_ops_score", "nw_ckpt_plan", "nw_ckpt_bytes", "nw_ckpt_peak_bytes",
           "nw_ckpt_sweep_async", "nw_score", "nw_traceback_block", "nw_align_ckpt", "nw_debug_tb_shift",
           "nw_batch_dir_bytes", "nw_score_batch_async", "nw_score_batch", "nw_align_batch",
           "nw_batch_affine_dir_bytes", "nw_score_batch_affine_async", "nw_score_batch_affine",
           "nw_align_batch_affine", "nw_ops_score_affine",
           "nw_score_batch_matrix_async", "nw_score_batch_matrix", "nw_align_batch_matrix", "nw_ops_score_matrix",
           "nw_score_batch_local_async", "nw_score_batch_local", "nw_align_batch_local",
           "nw_score_batch_semi_async", "nw_score_batch_semi", "nw_align_batch_semi",
           "nw_batch_banded_dir_bytes", "nw_score_batch_banded_async", "nw_score_batch_banded",
           "nw_align_batch_banded",
           "nw_batch_dual_dir_bytes", "nw_score_batch_dual_async", "nw_score_batch_dual", "nw_align_batch_dual",
           "nw_ops_score_dual",
           "nw_batch_dual_banded_dir_bytes", "nw_score_batch_dual_banded_async", "nw_score_batch_dual_banded",
           "nw_align_batch_dual_banded"]
IPC_HANDLE_BYTES = 64


class NwParams(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("mismatch", ctypes.c_int32), ("gap", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("waves", ctypes.c_int32), ("device", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("substrips", ctypes.c_int32),
                ("strip_waves", ctypes.c_int32), ("timeout_ms", ctypes.c_int32),
                ("kernel", ctypes.c_int32)]


class NwResult(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("cells", ctypes.c_int64),
                ("kernel_ms", ctypes.c_double), ("table_bytes", ctypes.c_double),
                ("strips", ctypes.c_int32), ("waves", ctypes.c_int32),
                ("substrips", ctypes.c_int32), ("strip_waves", ctypes.c_int32),
                ("end_i", ctypes.c_int64), ("end_j", ctypes.c_int64),
                ("kernel", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class NwAlignment(ctypes.Structure):
    """nw_alignment (include/nw_hip.h): a Smith-Waterman alignment."""
    _fields_ = [("score", ctypes.c_int32), ("status", ctypes.c_int32), ("begin_i", ctypes.c_int64),
                ("begin_j", ctypes.c_int64), ("end_i", ctypes.c_int64), ("end_j", ctypes.c_int64),
                ("n_ops", ctypes.c_int64), ("fill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double)]


class NwTbOpts(ctypes.Structure):
    """nw_tb_opts (include/nw_hip.h): window geometry of the global traceback (0 = default)."""
    _fields_ = [("band", ctypes.c_int32), ("max_windows", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class NwTbStats(ctypes.Structure):
    """nw_tb_stats (include/nw_hip.h): what a global traceback ran."""
    _fields_ = [("rounds", ctypes.c_int32), ("windows", ctypes.c_int32), ("band", ctypes.c_int32),
                ("max_windows", ctypes.c_int32), ("tail_ops", ctypes.c_int64)]


class NwCkptOpts(ctypes.Structure):
    """nw_ckpt_opts (include/nw_hip.h): block height and device budget of nw_align_ckpt (0 = planned)."""
    _fields_ = [("block_rows", ctypes.c_int64), ("mem_bytes", ctypes.c_int64), ("reserved", ctypes.c_int32 * 4)]


class NwCkptStats(ctypes.Structure):
    """nw_ckpt_stats (include/nw_hip.h): the plan of a checkpointed alignment and what it ran."""
    _fields_ = [("block_rows", ctypes.c_int64), ("blocks", ctypes.c_int64), ("ckpt_bytes", ctypes.c_int64),
                ("block_bytes", ctypes.c_int64), ("peak_bytes", ctypes.c_int64), ("refill_cells", ctypes.c_int64),
                ("rounds", ctypes.c_int32), ("windows", ctypes.c_int32), ("sweep_ms", ctypes.c_double),
                ("refill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double)]


class NwBatchOpts(ctypes.Structure):
    """nw_batch_opts (include/nw_hip.h): device budget of nw_align_batch (0 = 80 % of the free HBM)."""
    _fields_ = [("mem_bytes", ctypes.c_int64), ("reserved", ctypes.c_int32 * 6)]


class NwBatchStats(ctypes.Structure):
    """nw_batch_stats (include/nw_hip.h): what a batched call ran."""
    _fields_ = [("pairs", ctypes.c_int64), ("cells", ctypes.c_int64), ("chunks", ctypes.c_int64),
                ("dir_bytes", ctypes.c_int64), ("peak_bytes", ctypes.c_int64), ("waves", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("fill_ms", ctypes.c_double), ("walk_ms", ctypes.c_double)]


SUBMAT_MAX = 32  # NW_SUBMAT_MAX: letters of a substitution matrix


class NwSubmat(ctypes.Structure):
    """nw_submat (include/nw_hip.h): a substitution matrix over at most 32 letters."""
    _fields_ = [("n", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3), ("index", ctypes.c_uint8 * 256),
                ("score", ctypes.c_int8 * (SUBMAT_MAX * SUBMAT_MAX))]


CKPT_TAG = 1   # NW_CKPT_TAG: the tag of every checkpoint granule (nw_band.tag of a re-fill)
TB_NO_AIM = 1  # nw_tb_opts.flags NW_TB_NO_AIM: diagonal rounds instead of rounds aimed at (0, 0)


class NwLocalHit(ctypes.Structure):
    """nw_local_hit (include/nw_hip.h): the best local alignment of one pair of a batch."""
    _fields_ = [("score", ctypes.c_int32), ("end_i", ctypes.c_int32), ("end_j", ctypes.c_int32),
                ("begin_i", ctypes.c_int32), ("begin_j", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


# the same 32 bytes as a numpy record (score_batch_local, align_batch_local)
LOCAL_HIT_DTYPE = np.dtype([("score", np.int32), ("end_i", np.int32), ("end_j", np.int32), ("begin_i", np.int32),
                            ("begin_j", np.int32), ("reserved", np.int32, (3,))])


class NwBand(ctypes.Structure):
    """nw_band (include/nw_hip.h): halo granule buffers of one row band."""
    _fields_ = [("halo_in", ctypes.c_void_p), ("halo_out", ctypes.c_void_p),
                ("tag", ctypes.c_uint32), ("row0", ctypes.c_uint32)]


class NwBandCycle(ctypes.Structure):
    """nw_band_cycle (include/nw_hip.h): one rank's blocks of block-cyclic row bands."""
    _fields_ = [("halo_in", ctypes.c_void_p), ("halo_out", ctypes.c_void_p), ("nblk", ctypes.c_int32),
                ("hin_first", ctypes.c_int32), ("hout_shift", ctypes.c_int32), ("tag", ctypes.c_uint32),
                ("row0_max", ctypes.c_int64), ("t_stride", ctypes.c_int64)]


class NwColBand(ctypes.Structure):
    """nw_colband (include/nw_hip.h): feed granule buffers of one column band."""
    _fields_ = [("feed_in", ctypes.c_void_p), ("feed_out", ctypes.c_void_p), ("tag", ctypes.c_uint32),
                ("nbands", ctypes.c_int32), ("r", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class NwTBand(ctypes.Structure):
    """nw_tband (include/nw_hip.h): feed granule buffers of one row band in horizontal strips."""
    _fields_ = [("feed_in", ctypes.c_void_p), ("feed_out", ctypes.c_void_p), ("tag", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("row0", ctypes.c_int64)]


TBAND_DENSE_POLLS = 1  # nw_tband.flags NW_TBAND_DENSE_POLLS


class NwError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"libnwhip {what}: {strerror(status)} ({status})")


_lib = None
_i8p = ctypes.POINTER(ctypes.c_int8)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)


def lib() -> ctypes.CDLL:
    """Load build/libnwhip.so (raises if it has not been built).

    torch (when installed) is imported first: torch and libnwhip share one HIP
    runtime (libamdhip64.so.7, deduplicated by SONAME), and torch must be the one
    that loads it or its own device initialisation fails."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} missing: run `make -C fast-needleman-wunsch_amd` "
                                "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    L.nw_params_default.argtypes = [ctypes.POINTER(NwParams)]
    L.nw_params_default.restype = None
    L.nw_strerror.argtypes = [ctypes.c_int]
    L.nw_strerror.restype = ctypes.c_char_p
    L.nw_version.restype = ctypes.c_char_p
    L.nw_fill.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.POINTER(NwParams),
                          _i32p, ctypes.POINTER(NwResult)]
    L.nw_fill_emb.argtypes = L.nw_fill.argtypes
    L.nw_sw_align.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.POINTER(NwParams), _u8p,
                              ctypes.c_int64, ctypes.POINTER(NwAlignment)]
    L.nw_sw_traceback.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                  ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_void_p, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_int64, _u8p, ctypes.c_int64,
                                  ctypes.POINTER(NwAlignment)]
    L.nw_traceback.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                               ctypes.POINTER(NwParams), ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(NwTbOpts),
                               ctypes.c_void_p, _u8p, ctypes.c_int64, ctypes.POINTER(NwAlignment),
                               ctypes.POINTER(NwTbStats)]
    L.nw_align.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.POINTER(NwParams),
                           ctypes.POINTER(NwTbOpts), _u8p, ctypes.c_int64, ctypes.POINTER(NwAlignment),
                           ctypes.POINTER(NwTbStats)]
    L.nw_ckpt_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(NwCkptStats)]
    L.nw_ckpt_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.nw_ckpt_bytes.restype = ctypes.c_int64
    L.nw_ckpt_peak_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.nw_ckpt_peak_bytes.restype = ctypes.c_int64
    L.nw_ckpt_sweep_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.POINTER(NwParams),
                           ctypes.POINTER(NwResult)]
    L.nw_traceback_block.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.POINTER(NwTbOpts), ctypes.c_void_p, _u8p, ctypes.c_int64,
                                     ctypes.POINTER(NwAlignment), ctypes.POINTER(NwTbStats)]
    L.nw_align_ckpt.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.POINTER(NwParams),
                                ctypes.POINTER(NwCkptOpts), ctypes.POINTER(NwTbOpts), _u8p, ctypes.c_int64,
                                ctypes.POINTER(NwAlignment), ctypes.POINTER(NwCkptStats)]
    _i64p_ = ctypes.POINTER(ctypes.c_int64)
    L.nw_batch_dir_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.nw_batch_dir_bytes.restype = ctypes.c_int64
    L.nw_score_batch_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _i32p,
                                 ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams),
                                 ctypes.POINTER(NwBatchOpts), _i32p, _u8p, _i64p_, _i64p_,
                                 ctypes.POINTER(NwBatchStats)]
    L.nw_batch_affine_dir_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.nw_batch_affine_dir_bytes.restype = ctypes.c_int64
    L.nw_score_batch_affine_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch_affine.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams),
                                        ctypes.c_int32, _i32p, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_affine.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams),
                                        ctypes.c_int32, ctypes.POINTER(NwBatchOpts), _i32p, _u8p, _i64p_, _i64p_,
                                        ctypes.POINTER(NwBatchStats)]
    L.nw_ops_score_affine.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      _u8p, ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int64)]
    _smp = ctypes.POINTER(NwSubmat)
    L.nw_score_batch_matrix_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch_matrix.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                        ctypes.c_int32, _i32p, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_matrix.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                        ctypes.c_int32, ctypes.POINTER(NwBatchOpts), _i32p, _u8p, _i64p_, _i64p_,
                                        ctypes.POINTER(NwBatchStats)]
    L.nw_ops_score_matrix.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      _u8p, ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int64)]
    _lhp = ctypes.POINTER(NwLocalHit)
    L.nw_score_batch_local_async.argtypes = L.nw_score_batch_matrix_async.argtypes
    L.nw_score_batch_local.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                       ctypes.c_int32, _lhp, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_local.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                       ctypes.c_int32, ctypes.POINTER(NwBatchOpts), _lhp, _u8p, _i64p_, _i64p_,
                                       ctypes.POINTER(NwBatchStats)]
    L.nw_score_batch_semi_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch_semi.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                      ctypes.c_int32, ctypes.c_int32, _lhp, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_semi.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(NwBatchOpts), _lhp, _u8p,
                                      _i64p_, _i64p_, ctypes.POINTER(NwBatchStats)]
    L.nw_batch_banded_dir_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    L.nw_batch_banded_dir_bytes.restype = ctypes.c_int64
    L.nw_score_batch_banded_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch_banded.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                        ctypes.c_int32, ctypes.c_int32, _i32p, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_banded.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                        ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(NwBatchOpts), _i32p, _u8p,
                                        _i64p_, _i64p_, ctypes.POINTER(NwBatchStats)]
    L.nw_batch_dual_dir_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.nw_batch_dual_dir_bytes.restype = ctypes.c_int64
    L.nw_score_batch_dual_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.nw_score_batch_dual.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p,
                                      ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_dual.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams), _smp,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(NwBatchOpts),
                                      _i32p, _u8p, _i64p_, _i64p_, ctypes.POINTER(NwBatchStats)]
    L.nw_batch_dual_banded_dir_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    L.nw_batch_dual_banded_dir_bytes.restype = ctypes.c_int64
    L.nw_score_batch_dual_banded_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                                   ctypes.c_void_p]
    L.nw_score_batch_dual_banded.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams),
                                             _smp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             _i32p, ctypes.POINTER(NwBatchStats)]
    L.nw_align_batch_dual_banded.argtypes = [_i8p, _i64p_, _i8p, _i64p_, ctypes.c_int64, ctypes.POINTER(NwParams),
                                             _smp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(NwBatchOpts), _i32p, _u8p, _i64p_, _i64p_,
                                             ctypes.POINTER(NwBatchStats)]
    L.nw_ops_score_dual.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                    _u8p, ctypes.c_int64, ctypes.POINTER(NwParams), _smp, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
    L.nw_debug_tb_shift.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.c_int64]
    L.nw_debug_tb_shift.restype = ctypes.c_int64
    L.nw_ops_expand.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _u8p,
                                ctypes.c_int64, _i8p, _i8p]
    L.nw_ops_score.argtypes = [_i8p, ctypes.c_int64, _i8p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _u8p,
                               ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.POINTER(ctypes.c_int64)]
    L.nw_table_pitch.argtypes = [ctypes.c_int64]
    L.nw_table_pitch.restype = ctypes.c_int64
    L.nw_table_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.nw_table_bytes.restype = ctypes.c_int64
    L.nw_table_offset.argtypes = []
    L.nw_table_offset.restype = ctypes.c_int64
    L.nw_strip_lds_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.nw_strip_lds_bytes.restype = ctypes.c_int64
    L.nw_panel_lds_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.nw_panel_lds_bytes.restype = ctypes.c_int64
    L.nw_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_ctx_destroy.argtypes = [ctypes.c_void_p]
    L.nw_ctx_destroy.restype = None
    L.nw_ctx_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    L.nw_ctx_workspace_bytes.restype = ctypes.c_int64
    dev_args = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                ctypes.POINTER(NwParams), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.nw_fill_device.argtypes = dev_args + [ctypes.POINTER(NwResult)]
    L.nw_fill_device_async.argtypes = dev_args
    L.nw_ctx_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.nw_read_bdna.argtypes = [ctypes.c_char_p, ctypes.POINTER(_i8p), ctypes.POINTER(ctypes.c_int64)]
    L.nw_free.argtypes = [ctypes.c_void_p]
    L.nw_free.restype = None
    L.nw_synth_bdna.argtypes = [ctypes.c_uint64, ctypes.c_int64, _i8p]
    L.nw_synth_bdna.restype = None
    L.nw_band_layout.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.nw_band_layout.restype = None
    L.nw_halo_bytes.argtypes = [ctypes.c_int64]
    L.nw_halo_bytes.restype = ctypes.c_int64
    L.nw_fill_band_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(NwParams),
                                     ctypes.POINTER(NwBand), ctypes.c_void_p, ctypes.c_int64,
                                     ctypes.c_void_p]
    L.nw_ipc_get_handle.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.nw_ipc_open_handle.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_ipc_close_handle.argtypes = [ctypes.c_void_p]
    L.nw_halo_alloc.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_halo_free.argtypes = [ctypes.c_void_p]
    L.nw_halo_alloc_regions.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_fill_band_cycle_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.POINTER(NwBandCycle),
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.nw_tuned_shape.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                                 ctypes.POINTER(ctypes.c_int32)]
    L.nw_tuned_shape.restype = None
    L.nw_auto_shape.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.nw_auto_shape.restype = None
    L.nw_colband_layout.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.POINTER(NwParams), _i64p, _i64p, _i64p, _i64p]
    L.nw_feed_bytes.argtypes = [ctypes.c_int64]
    L.nw_feed_bytes.restype = ctypes.c_int64
    L.nw_feed_alloc.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_fill_colband_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.POINTER(NwColBand),
                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.nw_fill_tband_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.POINTER(NwParams), ctypes.POINTER(NwTBand),
                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.nw_link_alloc.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.nw_link_wait_async.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p]
    L.nw_link_wait_ctx_async.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32,
                                         ctypes.c_void_p]
    L.nw_debug_failure.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    L.nw_link_signal_async.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.nw_link_status.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    L.nw_host_warmup.argtypes = [ctypes.c_int]
    L.nw_host_release.argtypes = [ctypes.c_int]
    L.nw_host_release.restype = None
    L.nw_debug_ctrl.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    L.nw_debug_set_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.nw_debug_trace_words.argtypes = []
    L.nw_debug_trace_words.restype = ctypes.c_int32
    _lib = L
    return L


def strerror(status: int) -> str:
    try:
        return lib().nw_strerror(status).decode()
    except FileNotFoundError:
        return str(status)


def version() -> str:
    return lib().nw_version().decode()


@dataclass
class Scheme:
    """Runtime replacement of needleman-wunsch.hpp:11-13 (MATCH, MISMATCH, GAP)."""
    match: int = 1
    mismatch: int = 0
    gap: int = -1


def params(scheme=(1, 0, -1), waves: int = 0, device: int = -1, flags: int = 0,
           substrips: int = 0, strip_waves: int = 0, timeout_ms: int = 0, mode: int = MODE_NW,
           kernel: int = KERNEL_AUTO) -> NwParams:
    if isinstance(scheme, Scheme):
        scheme = (scheme.match, scheme.mismatch, scheme.gap)
    p = NwParams()
    lib().nw_params_default(ctypes.byref(p))
    p.match, p.mismatch, p.gap = (int(x) for x in scheme)
    p.waves = int(waves)
    p.device = int(device)
    p.flags = int(flags)
    p.substrips = int(substrips)
    p.strip_waves = int(strip_waves)
    p.timeout_ms = int(timeout_ms)
    p.mode = int(mode)
    p.kernel = int(kernel)
    return p


def sw_align(s1, s2, scheme=(1, -1, -1), device: int = -1, substrips: int = 0, strip_waves: int = 0,
             kernel: int = KERNEL_AUTO):
    """Smith-Waterman local alignment on the device (nw_sw_align): returns
    (NwAlignment, ops) with ops a uint8 array in path order (0 diag, 1 up, 2 left)."""
    a, b = _seq(s1), _seq(s2)
    ops = np.empty(a.size + b.size + 1, dtype=np.uint8)
    out = NwAlignment()
    p = params(scheme, device=device, substrips=substrips, strip_waves=strip_waves, mode=MODE_SW, kernel=kernel)
    st = lib().nw_sw_align(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, ctypes.byref(p),
                           ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ops.size, ctypes.byref(out))
    if st != NW_OK:
        raise NwError(st, "nw_sw_align")
    return out, ops[:out.n_ops].copy()


def tb_opts(band: int = 0, max_windows: int = 0, no_aim: bool = False) -> NwTbOpts:
    return NwTbOpts(int(band), int(max_windows), TB_NO_AIM if no_aim else 0, 0)


def align(s1, s2, scheme=(1, 0, -1), band: int = 0, max_windows: int = 0, no_aim: bool = False,
          device: int = -1, substrips: int = 0, strip_waves: int = 0, kernel: int = KERNEL_AUTO):
    """Global alignment on the device (nw_align): returns (NwAlignment, ops, NwTbStats),
    ops a uint8 array in path order from (0, 0) to (n2, n1) (0 diag, 1 up, 2 left).
    band / max_windows / no_aim: nw_tb_opts (0 = the defaults)."""
    a, b = _seq(s1), _seq(s2)
    ops = np.empty(max(a.size + b.size, 1), dtype=np.uint8)
    out, stats = NwAlignment(), NwTbStats()
    p = params(scheme, device=device, substrips=substrips, strip_waves=strip_waves, kernel=kernel)
    o = tb_opts(band, max_windows, no_aim)
    st = lib().nw_align(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, ctypes.byref(p),
                        ctypes.byref(o), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), a.size + b.size,
                        ctypes.byref(out), ctypes.byref(stats))
    if st != NW_OK:
        raise NwError(st, "nw_align")
    return out, ops[:out.n_ops].copy(), stats


def ckpt_plan(n1: int, n2: int, mem_bytes: int) -> NwCkptStats:
    """The block height a checkpointed alignment of an n1 x n2 pair gets within mem_bytes
    of device memory (nw_ckpt_plan; host only): block_rows, blocks, ckpt_bytes,
    block_bytes, peak_bytes.  Raises NwError(NW_ERR_OOM) when 64-row blocks do not fit."""
    plan = NwCkptStats()
    st = lib().nw_ckpt_plan(int(n1), int(n2), int(mem_bytes), ctypes.byref(plan))
    if st != NW_OK:
        raise NwError(st, "nw_ckpt_plan")
    return plan


def ckpt_peak_bytes(n1: int, n2: int, block_rows: int) -> int:
    """Device memory of an alignment in blocks of block_rows rows (nw_ckpt_peak_bytes)."""
    return int(lib().nw_ckpt_peak_bytes(int(n1), int(n2), int(block_rows)))


def ckpt_bytes(n1: int, n2: int, block_rows: int) -> int:
    return int(lib().nw_ckpt_bytes(int(n1), int(n2), int(block_rows)))


def score_sweep(s1, s2, scheme=(1, 0, -1), waves: int = 0, device: int = -1, flags: int = 0,
                timeout_ms: int = 0) -> NwResult:
    """Score of the global alignment without a table (nw_score: the checkpoint sweep
    with no checkpoints): NwResult with score, cells, kernel_ms; table_bytes = 0."""
    a, b = _seq(s1), _seq(s2)
    r = NwResult()
    p = params(scheme, waves, device, flags=flags, timeout_ms=timeout_ms)
    st = lib().nw_score(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, ctypes.byref(p),
                        ctypes.byref(r))
    if st != NW_OK:
        raise NwError(st, "nw_score")
    return r


def align_ckpt(s1, s2, scheme=(1, 0, -1), block_rows: int = 0, mem_bytes: int = 0, band: int = 0,
               max_windows: int = 0, no_aim: bool = False, device: int = -1, flags: int = 0):
    """Global alignment in linear memory (nw_align_ckpt): (NwAlignment, ops, NwCkptStats),
    the ops byte-identical to align's.  block_rows: K, a multiple of 64 (0: planned
    within mem_bytes; mem_bytes = 0: 80 % of the free device memory)."""
    a, b = _seq(s1), _seq(s2)
    ops = np.empty(max(a.size + b.size, 1), dtype=np.uint8)
    out, stats = NwAlignment(), NwCkptStats()
    p = params(scheme, device=device, flags=flags)
    o = tb_opts(band, max_windows, no_aim)
    co = NwCkptOpts(int(block_rows), int(mem_bytes))
    st = lib().nw_align_ckpt(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, ctypes.byref(p),
                             ctypes.byref(co), ctypes.byref(o), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                             a.size + b.size, ctypes.byref(out), ctypes.byref(stats))
    if st != NW_OK:
        raise NwError(st, "nw_align_ckpt")
    return out, ops[:out.n_ops].copy(), stats


def batch_dir_bytes(n1: int, n2: int) -> int:
    """Direction bytes of one pair in align_batch, with padding (nw_batch_dir_bytes):
    0 for an empty side, -1 for a negative size."""
    return int(lib().nw_batch_dir_bytes(int(n1), int(n2)))


def batch_csr(pairs):
    """(s1cat, off1, s2cat, off2) of a list of (s1, s2) pairs: the concatenations as int8
    arrays and the int64 offsets (npairs + 1 each) the batched calls take."""
    a = [_seq(p[0]) for p in pairs]
    b = [_seq(p[1]) for p in pairs]
    off1 = np.zeros(len(pairs) + 1, np.int64)
    off2 = np.zeros(len(pairs) + 1, np.int64)
    off1[1:] = np.cumsum([x.size for x in a])
    off2[1:] = np.cumsum([x.size for x in b])
    cat1 = np.concatenate(a) if a else np.zeros(0, np.int8)
    cat2 = np.concatenate(b) if b else np.zeros(0, np.int8)
    return (np.ascontiguousarray(cat1, dtype=np.int8), off1, np.ascontiguousarray(cat2, dtype=np.int8), off2)


def _batch_result(n: int, hits: bool):
    """The result array of a batched call, int32 scores or LOCAL_HIT_DTYPE hits, and its pointer."""
    res = np.zeros(max(n, 1), LOCAL_HIT_DTYPE if hits else np.int32)
    return res, res.ctypes.data_as(ctypes.POINTER(NwLocalHit) if hits else _i32p)


def _score_batch_call(entry: str, pairs, p: NwParams, extra=(), mat=None, hits: bool = False,
                      return_stats: bool = False):
    """One synchronous score call: the C entry `entry` on `pairs` under `p`, with `extra` (after
    the matrix, when `mat` is given: the sequences are checked against it) between the params and
    the results; `hits`: nw_local_hit records, not int32 scores."""
    s1, off1, s2, off2 = batch_csr(pairs)
    if mat is not None:
        mat.check(s1, s2)
        extra = (ctypes.byref(mat.c), *extra)
    n = len(pairs)
    res, resp = _batch_result(n, hits)
    stats = NwBatchStats()
    st = getattr(lib(), entry)(s1.ctypes.data_as(_i8p), off1.ctypes.data_as(_i64p), s2.ctypes.data_as(_i8p),
                               off2.ctypes.data_as(_i64p), n, ctypes.byref(p), *extra, resp, ctypes.byref(stats))
    if st != NW_OK:
        raise NwError(st, entry)
    return (res[:n], stats) if return_stats else res[:n]


def _align_batch_call(entry: str, pairs, p: NwParams, mem_bytes: int, extra=(), mat=None, hits: bool = False):
    """One synchronous align call, as _score_batch_call: (results, [ops of pair 0, ..], NwBatchStats)."""
    s1, off1, s2, off2 = batch_csr(pairs)
    if mat is not None:
        mat.check(s1, s2)
        extra = (ctypes.byref(mat.c), *extra)
    n = len(pairs)
    ops_off = off1 + off2
    ops = np.zeros(max(int(ops_off[-1]), 1), np.uint8)
    res, resp = _batch_result(n, hits)
    n_ops = np.zeros(max(n, 1), np.int64)
    stats = NwBatchStats()
    o = NwBatchOpts(int(mem_bytes))
    st = getattr(lib(), entry)(s1.ctypes.data_as(_i8p), off1.ctypes.data_as(_i64p), s2.ctypes.data_as(_i8p),
                               off2.ctypes.data_as(_i64p), n, ctypes.byref(p), *extra, ctypes.byref(o), resp,
                               ops.ctypes.data_as(_u8p), ops_off.ctypes.data_as(_i64p), n_ops.ctypes.data_as(_i64p),
                               ctypes.byref(stats))
    if st != NW_OK:
        raise NwError(st, entry)
    out = [ops[int(ops_off[i]):int(ops_off[i]) + int(n_ops[i])].copy() for i in range(n)]
    return res[:n], out, stats


def score_batch(pairs, scheme=(1, 0, -1), waves: int = 0, device: int = -1, flags: int = 0,
                return_stats: bool = False):
    """Scores of many (s1, s2) pairs in one call (nw_score_batch): an int32 array, the
    score of pair i at index i (and the NwBatchStats with return_stats)."""
    return _score_batch_call("nw_score_batch", pairs, params(scheme, waves, device, flags=flags),
                             return_stats=return_stats)


def align_batch(pairs, scheme=(1, 0, -1), mem_bytes: int = 0, waves: int = 0, device: int = -1, flags: int = 0):
    """Scores and alignments of many pairs in one call (nw_align_batch): (scores, [ops of
    pair 0, ops of pair 1, ..], NwBatchStats), each ops a uint8 array in path order (0, 0)
    -> (n2, n1) (0 diag, 1 up, 2 left), byte-identical to align's.  mem_bytes: the device
    budget the chunks fit (0 = 80 % of the free device memory)."""
    return _align_batch_call("nw_align_batch", pairs, params(scheme, waves, device, flags=flags), mem_bytes)


def batch_affine_dir_bytes(n1: int, n2: int) -> int:
    """Direction bytes of one pair in align_batch_affine (nw_batch_affine_dir_bytes): 4 bits
    per cell, twice batch_dir_bytes; 0 for an empty side, -1 for a negative size."""
    return int(lib().nw_batch_affine_dir_bytes(int(n1), int(n2)))


def score_batch_affine(pairs, scheme=(1, 0, -1), gap_open: int = 0, waves: int = 0, device: int = -1,
                       flags: int = 0, return_stats: bool = False):
    """score_batch under affine gap cost (nw_score_batch_affine): a run of L ups or of L
    lefts costs gap_open + L * scheme[2]."""
    return _score_batch_call("nw_score_batch_affine", pairs, params(scheme, waves, device, flags=flags),
                             (int(gap_open),), return_stats=return_stats)


def align_batch_affine(pairs, scheme=(1, 0, -1), gap_open: int = 0, mem_bytes: int = 0, waves: int = 0,
                       device: int = -1, flags: int = 0):
    """align_batch under affine gap cost (nw_align_batch_affine): (scores, [ops of pair 0,
    ..], NwBatchStats), the ops the three-state walk include/nw_hip.h defines."""
    return _align_batch_call("nw_align_batch_affine", pairs, params(scheme, waves, device, flags=flags), mem_bytes,
                             (int(gap_open),))


def ops_score_affine(s1, s2, ops, scheme=(1, 0, -1), gap_open: int = 0, begin=(0, 0)) -> int:
    """Score of an alignment's ops under affine gap cost (nw_ops_score_affine): ops_score
    plus gap_open for every run of ups or of lefts."""
    a, b = _seq(s1), _seq(s2)
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    p = params(scheme)
    sc = ctypes.c_int64()
    st = lib().nw_ops_score_affine(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, int(begin[0]),
                                   int(begin[1]), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), o.size,
                                   ctypes.byref(p), int(gap_open), ctypes.byref(sc))
    if st != NW_OK:
        raise NwError(st, "nw_ops_score_affine")
    return int(sc.value)


def _letter_byte(tok) -> int:
    """A letter of a matrix: an int byte value, a one-character str / bytes, or "0xHH"."""
    if isinstance(tok, (int, np.integer)):
        v = int(tok)
    elif isinstance(tok, bytes) and len(tok) == 1:
        v = tok[0]
    elif isinstance(tok, str) and len(tok) == 1:
        v = ord(tok)
    elif isinstance(tok, str) and len(tok) == 4 and tok[:2] in ("0x", "0X"):
        v = int(tok[2:], 16)
    else:
        raise ValueError(f"matrix letter {tok!r}: one character or 0xHH expected")
    if not 0 <= v <= 255:
        raise ValueError(f"matrix letter {tok!r} is not a byte")
    return v


class SubMatrix:
    """A substitution matrix for the *_matrix calls (nw_submat, include/nw_hip.h).

    letters: n <= 32 distinct letters -- a str or bytes (one letter per character) or a
             sequence of byte values / one-character strings / "0xHH" strings.
    scores:  n x n integers that fit int8; scores[x][y] = s(s1 letter x, s2 letter y), so
             the matrix may be asymmetric.
    other:   the letter every unlisted byte maps to (a wildcard: X, N, *).  Without it an
             unlisted byte in a sequence raises ValueError in the host-side calls, and
             the device-side call (Context.score_batch_matrix), which cannot look at the
             sequences, refuses the matrix.
    A lower-case ASCII byte maps like its upper-case letter unless it is listed itself."""

    def __init__(self, letters, scores, other=None):
        if isinstance(letters, (str, bytes, bytearray)):
            letters = list(letters)
        self.letters = [_letter_byte(t) for t in letters]
        n = len(self.letters)
        if not 1 <= n <= SUBMAT_MAX:
            raise ValueError(f"a matrix has 1..{SUBMAT_MAX} letters, not {n}")
        if len(set(self.letters)) != n:
            raise ValueError("matrix letters must be distinct")
        sc = np.asarray(scores)
        if sc.shape != (n, n) or not np.issubdtype(sc.dtype, np.integer):
            raise ValueError(f"scores must be {n} x {n} integers")
        if sc.min() < -128 or sc.max() > 127:
            raise ValueError("matrix scores must fit int8 (-128..127)")
        self.scores = sc.astype(np.int64)
        self.other = None if other is None else _letter_byte(other)
        if self.other is not None and self.other not in self.letters:
            raise ValueError("other must be one of the letters")
        pos = {b: k for k, b in enumerate(self.letters)}
        fill = pos[self.other] if self.other is not None else 0
        self.index = np.full(256, fill, np.uint8)
        self.listed = np.zeros(256, bool)
        for b, k in pos.items():
            self.index[b], self.listed[b] = k, True
        for b in range(ord("a"), ord("z") + 1):
            if not self.listed[b] and self.listed[b - 32]:
                self.index[b], self.listed[b] = self.index[b - 32], True
        self.c = NwSubmat()
        self.c.n = n
        self.c.index[:] = self.index.tolist()
        full = np.zeros((SUBMAT_MAX, SUBMAT_MAX), np.int8)
        full[:n, :n] = sc
        self.c.score[:] = full.ravel().tolist()

    @property
    def n(self) -> int:
        return len(self.letters)

    def check(self, *seqs) -> None:
        """Without `other`: ValueError for a sequence byte that is no letter."""
        if self.other is not None:
            return
        for s in seqs:
            s = _seq(s).view(np.uint8)
            bad = ~self.listed[s]
            if bad.any():
                raise ValueError(f"byte {int(s[bad][0])} is not a letter of the matrix (pass other=)")

    @classmethod
    def uniform(cls, letters, match: int, mismatch: int, other=None):
        """The match / mismatch matrix over `letters`: `match` on the diagonal, `mismatch`
        elsewhere.  other: one more letter, added to them, that every unlisted byte maps
        to and that scores `mismatch` against everything, itself included (N against N is
        no match)."""
        if isinstance(letters, (str, bytes, bytearray)):
            letters = list(letters)
        letters = [_letter_byte(t) for t in letters]
        if other is not None:
            letters = letters + [_letter_byte(other)]
        n = len(letters)
        sc = np.full((n, n), int(mismatch), np.int64)
        sc[np.arange(n), np.arange(n)] = int(match)
        if other is not None:
            sc[n - 1, n - 1] = int(mismatch)
        return cls(letters, sc, None if other is None else letters[-1])

    @classmethod
    def from_text(cls, path_or_str, other=None):
        """The usual NCBI text layout: '#' comment lines, a header row of letters, then one
        row per letter (its letter, then n integers): the entry of row r, column c is
        s(s1 letter r, s2 letter c).  A letter is one character or 0xHH (a byte value).
        Text with a newline is parsed as it is, anything else is a path.  other=None and
        a '*' among the letters: '*' is the wildcard, as in NCBI's files."""
        text = path_or_str
        if isinstance(text, bytes):
            text = text.decode("ascii")
        if "\n" not in text:
            with open(text) as f:
                text = f.read()
        letters, rows = None, {}
        for line in text.splitlines():
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if letters is None:
                letters = [_letter_byte(t) for t in tok]
                continue
            r = _letter_byte(tok[0])
            if r not in letters or r in rows or len(tok) != len(letters) + 1:
                raise ValueError(f"matrix row {line!r}: a letter of the header and {len(letters)} numbers expected")
            try:
                rows[r] = [int(t) for t in tok[1:]]
            except ValueError:
                raise ValueError(f"matrix row {line!r}: integers expected") from None
        if letters is None or len(rows) != len(letters):
            raise ValueError("matrix text: a header row and one row per letter expected")
        if other is None and ord("*") in letters:
            other = "*"
        return cls(letters, np.array([rows[b] for b in letters], np.int64), other)


def _needs_other(mat: SubMatrix, who: str) -> None:
    """The calls on device tensors do not look at the sequences: the matrix must cover every byte."""
    if mat.other is None and not mat.listed.all():
        raise ValueError(who + " needs a matrix with other= (it cannot check the sequences)")


def score_batch_matrix(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, waves: int = 0, device: int = -1,
                       return_stats: bool = False):
    """score_batch_affine with substitution by matrix (nw_score_batch_matrix): s(s1 letter,
    s2 letter) from `mat`, a run of L ups or of L lefts costs gap_open + L * gap."""
    return _score_batch_call("nw_score_batch_matrix", pairs, params((1, 0, int(gap)), waves, device),
                             (int(gap_open),), mat, return_stats=return_stats)


def align_batch_matrix(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, mem_bytes: int = 0, waves: int = 0,
                       device: int = -1):
    """align_batch_affine with substitution by matrix (nw_align_batch_matrix): (scores, [ops
    of pair 0, ..], NwBatchStats)."""
    return _align_batch_call("nw_align_batch_matrix", pairs, params((1, 0, int(gap)), waves, device), mem_bytes,
                             (int(gap_open),), mat)


def score_batch_local(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, waves: int = 0, device: int = -1,
                      return_stats: bool = False):
    """Batched local alignment scores (nw_score_batch_local): Smith-Waterman under affine
    gap cost with substitution by `mat`.  Returns a LOCAL_HIT_DTYPE array, one record per
    pair: score, end_i, end_j (the first row-major maximum; (0, 0) when the score is 0)
    and begin_i = begin_j = -1 (the score entry finds no begin cell)."""
    return _score_batch_call("nw_score_batch_local", pairs, params((1, 0, int(gap)), waves, device, mode=MODE_SW),
                             (int(gap_open),), mat, hits=True, return_stats=return_stats)


def align_batch_local(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, mem_bytes: int = 0, waves: int = 0,
                      device: int = -1):
    """Batched local alignments (nw_align_batch_local): (hits, [ops of pair 0, ..],
    NwBatchStats).  hits as score_batch_local with the begin cells filled in; a pair's ops
    (0 diag, 1 up, 2 left) lead from its begin cell to its end cell."""
    return _align_batch_call("nw_align_batch_local", pairs, params((1, 0, int(gap)), waves, device, mode=MODE_SW),
                             mem_bytes, (int(gap_open),), mat, hits=True)


def score_batch_semi(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, ends: int = ENDS_S2_IN_S1,
                     waves: int = 0, device: int = -1, return_stats: bool = False):
    """Batched semi-global alignment scores (nw_score_batch_semi): Gotoh with substitution
    by `mat` and the end gaps of `ends` (ENDS_* bits) free.  Returns a LOCAL_HIT_DTYPE array
    as score_batch_local does: score (it may be negative), end_i, end_j (the first row-major
    maximum among the admissible end cells) and begin_i = begin_j = -1."""
    return _score_batch_call("nw_score_batch_semi", pairs, params((1, 0, int(gap)), waves, device),
                             (int(gap_open), int(ends)), mat, hits=True, return_stats=return_stats)


def align_batch_semi(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, ends: int = ENDS_S2_IN_S1,
                     mem_bytes: int = 0, waves: int = 0, device: int = -1):
    """Batched semi-global alignments (nw_align_batch_semi): (hits, [ops of pair 0, ..],
    NwBatchStats), as align_batch_local returns them.  A pair's ops (0 diag, 1 up, 2 left)
    lead from its begin cell to its end cell; the skipped ends emit nothing."""
    return _align_batch_call("nw_align_batch_semi", pairs, params((1, 0, int(gap)), waves, device), mem_bytes,
                             (int(gap_open), int(ends)), mat, hits=True)


def _band32(band) -> int:
    """The band width as the int32 the C entries take: any width of 2^31 - 1 or more covers
    every table they admit."""
    return min(int(band), 2**31 - 1)


def batch_banded_dir_bytes(n1: int, n2: int, band: int) -> int:
    """Direction bytes of one pair in align_batch_banded (nw_batch_banded_dir_bytes): the
    iterations of each strip that can touch the band; batch_affine_dir_bytes(n1, n2) when
    the band covers the table; 0 for an empty side, -1 for a negative size or band."""
    return int(lib().nw_batch_banded_dir_bytes(int(n1), int(n2), _band32(band)))


def score_batch_banded(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, band: int = 0, waves: int = 0,
                       device: int = -1, return_stats: bool = False):
    """score_batch_matrix inside a band (nw_score_batch_banded): with n1 = len(s1) columns
    and n2 = len(s2) rows, cell (i, j) counts iff min(0, n2 - n1) - band <= i - j <= max(0,
    n2 - n1) + band; the score is the best over the paths that stay inside.  A band of
    max(n1, n2) or more gives score_batch_matrix's scores."""
    return _score_batch_call("nw_score_batch_banded", pairs, params((1, 0, int(gap)), waves, device),
                             (int(gap_open), _band32(band)), mat, return_stats=return_stats)


def align_batch_banded(pairs, mat: SubMatrix, gap: int = -1, gap_open: int = 0, band: int = 0, mem_bytes: int = 0,
                       waves: int = 0, device: int = -1):
    """align_batch_matrix inside a band (nw_align_batch_banded): (scores, [ops of pair 0,
    ..], NwBatchStats).  Every vertex of a pair's path is in its band; direction bits are
    kept for the band's neighbourhood only (batch_banded_dir_bytes)."""
    return _align_batch_call("nw_align_batch_banded", pairs, params((1, 0, int(gap)), waves, device), mem_bytes,
                             (int(gap_open), _band32(band)), mat)


def batch_dual_dir_bytes(n1: int, n2: int) -> int:
    """Direction bytes of one pair in align_batch_dual (nw_batch_dual_dir_bytes): a byte per
    cell, 2 * batch_affine_dir_bytes(n1, n2); 0 for an empty side, -1 for a negative size."""
    return int(lib().nw_batch_dual_dir_bytes(int(n1), int(n2)))


def score_batch_dual(pairs, mat: SubMatrix, gap: int = -2, gap_open: int = -4, gap2: int = -1, gap_open2: int = -24,
                     waves: int = 0, device: int = -1, return_stats: bool = False):
    """score_batch_matrix under a two-piece gap cost (nw_score_batch_dual): a run of L ups
    or of L lefts costs max(gap_open + L * gap, gap_open2 + L * gap2) -- short indels by the
    steep piece, long ones by the flat piece.  Equal pieces give score_batch_matrix's scores."""
    return _score_batch_call("nw_score_batch_dual", pairs, params((1, 0, int(gap)), waves, device),
                             (int(gap_open), int(gap_open2), int(gap2)), mat, return_stats=return_stats)


def align_batch_dual(pairs, mat: SubMatrix, gap: int = -2, gap_open: int = -4, gap2: int = -1, gap_open2: int = -24,
                     mem_bytes: int = 0, waves: int = 0, device: int = -1):
    """align_batch_matrix under a two-piece gap cost (nw_align_batch_dual): (scores, [ops of
    pair 0, ..], NwBatchStats).  The ops are 0 / 1 / 2 as everywhere: they do not say which
    piece priced a run (ops_score_dual takes the better one per run)."""
    return _align_batch_call("nw_align_batch_dual", pairs, params((1, 0, int(gap)), waves, device), mem_bytes,
                             (int(gap_open), int(gap_open2), int(gap2)), mat)


def batch_dual_banded_dir_bytes(n1: int, n2: int, band: int) -> int:
    """Direction bytes of one pair in align_batch_dual_banded (nw_batch_dual_banded_dir_bytes): a
    byte per cell for the iterations of each strip that can touch the band, 2 *
    batch_banded_dir_bytes(n1, n2, band); batch_dual_dir_bytes(n1, n2) when the band covers the
    table; 0 for an empty side, -1 for a negative size or band."""
    return int(lib().nw_batch_dual_banded_dir_bytes(int(n1), int(n2), _band32(band)))


def score_batch_dual_banded(pairs, mat: SubMatrix, gap: int = -2, gap_open: int = -4, gap2: int = -1,
                            gap_open2: int = -24, band: int = 0, waves: int = 0, device: int = -1,
                            return_stats: bool = False):
    """score_batch_dual inside a band (nw_score_batch_dual_banded): only paths that stay within
    `band` diagonals of the pair's own (of 0 .. n2 - n1) count.  A covering band gives
    score_batch_dual's scores, equal pieces give score_batch_banded's."""
    return _score_batch_call("nw_score_batch_dual_banded", pairs, params((1, 0, int(gap)), waves, device),
                             (int(gap_open), int(gap_open2), int(gap2), _band32(band)), mat,
                             return_stats=return_stats)


def align_batch_dual_banded(pairs, mat: SubMatrix, gap: int = -2, gap_open: int = -4, gap2: int = -1,
                            gap_open2: int = -24, band: int = 0, mem_bytes: int = 0, waves: int = 0,
                            device: int = -1):
    """align_batch_dual inside a band (nw_align_batch_dual_banded): (scores, [ops of pair 0, ..],
    NwBatchStats); every vertex of a path lies in the band.  stats.dir_bytes counts the
    iterations of each strip's range alone (batch_dual_banded_dir_bytes)."""
    return _align_batch_call("nw_align_batch_dual_banded", pairs, params((1, 0, int(gap)), waves, device), mem_bytes,
                             (int(gap_open), int(gap_open2), int(gap2), _band32(band)), mat)


def ops_score_dual(s1, s2, ops, mat: SubMatrix, gap: int = -2, gap_open: int = -4, gap2: int = -1,
                   gap_open2: int = -24, begin=(0, 0)) -> int:
    """Score of an alignment's ops under a matrix and the two-piece gap cost (nw_ops_score_dual):
    every maximal run of L ups or of L lefts adds max(gap_open + L * gap, gap_open2 + L * gap2)."""
    a, b = _seq(s1), _seq(s2)
    mat.check(a, b)
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    p = params((1, 0, int(gap)))
    sc = ctypes.c_int64()
    st = lib().nw_ops_score_dual(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, int(begin[0]),
                                 int(begin[1]), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), o.size,
                                 ctypes.byref(p), ctypes.byref(mat.c), int(gap_open), int(gap_open2), int(gap2),
                                 ctypes.byref(sc))
    if st != NW_OK:
        raise NwError(st, "nw_ops_score_dual")
    return int(sc.value)


def ops_score_matrix(s1, s2, ops, mat: SubMatrix, gap: int = -1, gap_open: int = 0, begin=(0, 0)) -> int:
    """Score of an alignment's ops under a matrix and affine gap cost (nw_ops_score_matrix)."""
    a, b = _seq(s1), _seq(s2)
    mat.check(a, b)
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    p = params((1, 0, int(gap)))
    sc = ctypes.c_int64()
    st = lib().nw_ops_score_matrix(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, int(begin[0]),
                                   int(begin[1]), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), o.size,
                                   ctypes.byref(p), ctypes.byref(mat.c), int(gap_open), ctypes.byref(sc))
    if st != NW_OK:
        raise NwError(st, "nw_ops_score_matrix")
    return int(sc.value)


def ops_expand(s1, s2, ops, begin=(0, 0)):
    """The two gapped rows of an alignment (nw_ops_expand): (row1 from s1, row2 from s2),
    int8 arrays of len(ops) with 0 = gap; `begin` = (begin_i, begin_j), (0, 0) for a
    global alignment."""
    a, b = _seq(s1), _seq(s2)
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    r1, r2 = np.zeros(max(o.size, 1), np.int8), np.zeros(max(o.size, 1), np.int8)
    st = lib().nw_ops_expand(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, int(begin[0]),
                             int(begin[1]), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), o.size,
                             r1.ctypes.data_as(_i8p), r2.ctypes.data_as(_i8p))
    if st != NW_OK:
        raise NwError(st, "nw_ops_expand")
    return r1[:o.size], r2[:o.size]


def ops_score(s1, s2, ops, scheme=(1, 0, -1), begin=(0, 0)) -> int:
    """Sum of match / mismatch / gap along an alignment's ops (nw_ops_score)."""
    a, b = _seq(s1), _seq(s2)
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    p = params(scheme)
    sc = ctypes.c_int64()
    st = lib().nw_ops_score(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size, int(begin[0]),
                            int(begin[1]), o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), o.size,
                            ctypes.byref(p), ctypes.byref(sc))
    if st != NW_OK:
        raise NwError(st, "nw_ops_score")
    return int(sc.value)


def _seq(s) -> np.ndarray:
    if isinstance(s, (bytes, bytearray)):
        return np.frombuffer(bytes(s), dtype=np.int8).copy()
    return np.ascontiguousarray(np.asarray(s, dtype=np.int8))


FLAG_TIMING_ONLY, FLAG_NO_PROFILE, FLAG_NO_FINISH = 1, 2, 4  # nw_params.flags (include/nw_hip.h)
FLAG_DEBUG_DRAIN, FLAG_DEBUG_NO_STORE = 0x100, 0x200  # compute-pace probes, with FLAG_TIMING_ONLY only
FLAG_DEBUG_NO_CHAIN = 0x400  # store-pattern probe: strips unchained, HBM stores kept, no fill
FLAG_DEBUG_STAGGER = 0x800   # with NO_CHAIN: strip p starts p * 11.5 us after its claim


def fill(s1, s2, scheme=(1, 0, -1), waves: int = 0, device: int = -1, substrips: int = 0,
         flags: int = 0, strip_waves: int = 0, kernel: int = KERNEL_AUTO):
    """Full table in the reference layout ((n2+1) x (n1+1) int32) + NwResult."""
    a, b = _seq(s1), _seq(s2)
    t = np.empty((b.size + 1, a.size + 1), dtype=np.int32)
    r = NwResult()
    p = params(scheme, waves, device, flags=flags, substrips=substrips, strip_waves=strip_waves, kernel=kernel)
    st = lib().nw_fill(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size,
                       ctypes.byref(p), t.ctypes.data_as(_i32p), ctypes.byref(r))
    if st != NW_OK:
        raise NwError(st, "nw_fill")
    return t, r


def score(s1, s2, scheme=(1, 0, -1), waves: int = 0, device: int = -1, substrips: int = 0,
          strip_waves: int = 0, kernel: int = KERNEL_AUTO) -> int:
    a, b = _seq(s1), _seq(s2)
    r = NwResult()
    p = params(scheme, waves, device, substrips=substrips, strip_waves=strip_waves, kernel=kernel)
    st = lib().nw_fill(a.ctypes.data_as(_i8p), a.size, b.ctypes.data_as(_i8p), b.size,
                       ctypes.byref(p), None, ctypes.byref(r))
    if st != NW_OK:
        raise NwError(st, "nw_fill")
    return int(r.score)


def host_release(device: int = -1) -> None:
    """Free the per-device state of the host-buffer calls (nw_host_release)."""
    lib().nw_host_release(device)


def trace_words() -> int:
    """uint64 words per strip of the debug trace (nw_debug_trace_words)."""
    return int(lib().nw_debug_trace_words())


def table_pitch(n1: int) -> int:
    return int(lib().nw_table_pitch(n1))


def table_rows(n2: int) -> int:
    return (n2 + 1 + 63) // 64 * 64


def table_offset() -> int:
    """Element offset of the table base from a 256-byte aligned allocation that
    puts column 1 on a 256-byte line (nw_table_offset)."""
    return int(lib().nw_table_offset())


def tuned_shape(n1: int, n2: int) -> tuple[int, int]:
    """(C, NC) an auto-shaped fill of an n1 x n2 table uses (nw_tuned_shape)."""
    c, nc = ctypes.c_int32(), ctypes.c_int32()
    lib().nw_tuned_shape(n1, n2, ctypes.byref(c), ctypes.byref(nc))
    return int(c.value), int(nc.value)


def auto_shape(n1: int, n2: int, cus: int = 256) -> tuple[int, int, int]:
    """(kernel, C, NC) a global fill with kernel = substrips = strip_waves = 0 uses
    for an n1 x n2 table on a device of `cus` CUs (nw_auto_shape)."""
    k, c, nc = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib().nw_auto_shape(n1, n2, cus, ctypes.byref(k), ctypes.byref(c), ctypes.byref(nc))
    return int(k.value), int(c.value), int(nc.value)


def strip_shape(substrips: int = 0, strip_waves: int = 0, n1: int = -1, n2: int = -1) -> tuple[int, int]:
    """(C, NC) the library uses for these nw_params values (0 = auto), as
    make_shape in nw_capi.cpp: auto = the tuned shape for the table size (n1, n2;
    (2, 2) when no size is given); C alone implies 256-column strips."""
    if substrips <= 0 and strip_waves <= 0:
        return tuned_shape(n1, n2) if n1 >= 0 and n2 >= 0 else (2, 2)
    c = substrips if substrips > 0 else 2
    if strip_waves > 0:
        return c, strip_waves
    return c, {1: 4, 2: 2, 4: 1}[c]


def strip_lds_bytes(substrips: int, strip_waves: int) -> int:
    """LDS bytes of one strip workgroup of this shape (-1: unsupported shape)."""
    return int(lib().nw_strip_lds_bytes(substrips, strip_waves))


def panel_lds_bytes(substrips: int, strip_waves: int) -> int:
    """LDS bytes of one panel workgroup of this shape (-1: unsupported shape)."""
    return int(lib().nw_panel_lds_bytes(substrips, strip_waves))


def read_bdna(path: str) -> np.ndarray:
    """readSequence semantics (src/common/helper.cpp:3-25)."""
    buf = _i8p()
    n = ctypes.c_int64()
    st = lib().nw_read_bdna(path.encode(), ctypes.byref(buf), ctypes.byref(n))
    if st != NW_OK:
        raise FileNotFoundError(path)
    out = np.ctypeslib.as_array(buf, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int8)
    lib().nw_free(buf)
    return out


def band_layout(n2: int, nbands: int, r: int):
    """(rows incl. the halo row, global index of row 0) of band r -- the row
    partition of src/mpi/mpi-horz-driver.cpp:31-32 / mpi-horz.cpp:16."""
    rows, start = ctypes.c_int64(), ctypes.c_int64()
    lib().nw_band_layout(n2, nbands, r, ctypes.byref(rows), ctypes.byref(start))
    return int(rows.value), int(start.value)


def colband_layout(n1: int, n2: int, nbands: int, r: int, substrips: int = 0, strip_waves: int = 0,
                   kernel: int = KERNEL_AUTO):
    """(strip_first, strip_count, start, n_cols) of column band r: its strips of the
    whole table's sweep and the global columns [start, start + n_cols) of its local
    table, local column 0 = band r-1's last column (src/mpi/mpi-vert.cpp:17,
    mpi-vert-driver.cpp:35-36, at strip granularity)."""
    p = params(substrips=substrips, strip_waves=strip_waves, kernel=kernel)
    out = [ctypes.c_int64() for _ in range(4)]
    st = lib().nw_colband_layout(n1, n2, nbands, r, ctypes.byref(p), *[ctypes.byref(x) for x in out])
    if st != NW_OK:
        raise NwError(st, "nw_colband_layout")
    return tuple(int(x.value) for x in out)


def feed_bytes(n2: int) -> int:
    return int(lib().nw_feed_bytes(n2))


def halo_bytes(n1: int) -> int:
    return int(lib().nw_halo_bytes(n1))


class Halo:
    """A zeroed halo granule buffer (regions x (n1+1) {tag, value}) in its own
    allocation (one region per row block for block-cyclic bands)."""

    def __init__(self, n1: int, device: int = -1, regions: int = 1):
        ptr = ctypes.c_void_p()
        st = lib().nw_halo_alloc_regions(device, n1, regions, ctypes.byref(ptr))
        if st != NW_OK:
            raise NwError(st, "nw_halo_alloc_regions")
        self.ptr, self.n1, self.regions = int(ptr.value), n1, regions

    def free(self):
        if self.ptr:
            lib().nw_halo_free(ctypes.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Feed(Halo):
    """A zeroed column-band feed granule buffer (n2+1 rows, padded to 64, x {tag, value})."""

    def __init__(self, n2: int, device: int = -1):
        ptr = ctypes.c_void_p()
        st = lib().nw_feed_alloc(device, n2, ctypes.byref(ptr))
        if st != NW_OK:
            raise NwError(st, "nw_feed_alloc")
        self.ptr, self.n2 = int(ptr.value), n2


class Link(Halo):
    """A zeroed launch-to-launch flow-control word pair (nw_link_alloc): the
    consumer band signals into it (peer store), the producer's stream waits on it."""

    def __init__(self, device: int = -1):
        ptr = ctypes.c_void_p()
        st = lib().nw_link_alloc(device, ctypes.byref(ptr))
        if st != NW_OK:
            raise NwError(st, "nw_link_alloc")
        self.ptr = int(ptr.value)

    def status(self) -> int:
        out = ctypes.c_uint32()
        st = lib().nw_link_status(ctypes.c_void_p(self.ptr), ctypes.byref(out))
        if st != NW_OK:
            raise NwError(st, "nw_link_status")
        return int(out.value)


def link_wait(ptr: int, value: int, stream, timeout_ms: int = 0, ctx: "Context | None" = None) -> None:
    """Stream-ordered wait until the link word at `ptr` is >= value (nw_link_wait_async).
    With `ctx` (nw_link_wait_ctx_async) a wait that gives up also fails that context:
    its next fill gives up at once instead of rewriting a buffer still being read."""
    st = lib().nw_link_wait_ctx_async(ctx._h if ctx is not None else None, ctypes.c_void_p(ptr),
                                      int(value) & 0xFFFFFFFF, int(timeout_ms), ctypes.c_void_p(stream.cuda_stream))
    if st != NW_OK:
        raise NwError(st, "nw_link_wait_ctx_async")


def link_status_at(ptr: int) -> int:
    """Word [1] of the word pair at `ptr` (nw_link_status): what a nw_link_wait on
    `ptr` records when it gives up, 0 otherwise."""
    out = ctypes.c_uint32()
    st = lib().nw_link_status(ctypes.c_void_p(ptr), ctypes.byref(out))
    if st != NW_OK:
        raise NwError(st, "nw_link_status")
    return int(out.value)


def link_signal(ptr: int, value: int, stream) -> None:
    """Stream-ordered store of `value` into the link word at `ptr` (may be peer memory)."""
    st = lib().nw_link_signal_async(ctypes.c_void_p(ptr), int(value) & 0xFFFFFFFF,
                                    ctypes.c_void_p(stream.cuda_stream))
    if st != NW_OK:
        raise NwError(st, "nw_link_signal_async")


def ipc_get_handle(ptr: int) -> bytes:
    """Export a device allocation (e.g. a halo buffer) to another process."""
    buf = ctypes.create_string_buffer(IPC_HANDLE_BYTES)
    st = lib().nw_ipc_get_handle(ctypes.c_void_p(ptr), buf)
    if st != NW_OK:
        raise NwError(st, "nw_ipc_get_handle")
    return buf.raw


def ipc_open_handle(handle: bytes) -> int:
    """Map a peer process's exported allocation into this device's address space."""
    ptr = ctypes.c_void_p()
    st = lib().nw_ipc_open_handle(handle, ctypes.byref(ptr))
    if st != NW_OK:
        raise NwError(st, "nw_ipc_open_handle")
    return int(ptr.value)


def ipc_close_handle(ptr: int) -> None:
    st = lib().nw_ipc_close_handle(ctypes.c_void_p(ptr))
    if st != NW_OK:
        raise NwError(st, "nw_ipc_close_handle")


def synth(seed: int, n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.int8)
    lib().nw_synth_bdna(seed, n, out.ctypes.data_as(_i8p))
    return out


class Context:
    """Device-resident fills on torch tensors (table stays in HBM)."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        st = lib().nw_ctx_create(device, ctypes.byref(self._h))
        if st != NW_OK:
            raise NwError(st, "nw_ctx_create")
        self.device = device

    def close(self):
        if self._h:
            lib().nw_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def alloc_table(n1: int, n2: int, device="cuda", pitch: int = 0):
        """(table_rows(n2), table_pitch(n1)) int32 view whose base sits
        table_offset() elements into a 256-byte aligned allocation, so that column
        1 of every row starts a 256-byte line (the fill then sweeps columns 1..n1
        in whole strips; include/nw_hip.h, nw_table_offset).  `pitch` (a
        multiple of 64 >= table_pitch(n1)) overrides the row pitch."""
        import torch
        rows = table_rows(n2)
        pitch = pitch or table_pitch(n1)
        assert pitch % 64 == 0 and pitch >= table_pitch(n1)
        off = table_offset() if n1 >= 1 else 0  # (no column 1 when n1 = 0)
        flat = torch.empty(rows * pitch + 64, dtype=torch.int32, device=device)
        shift = (-(flat.data_ptr() // 4) + off) % 64  # torch allocations are 512-B aligned
        return flat[shift:shift + rows * pitch].view(rows, pitch)

    @staticmethod
    def alloc_cycle_tables(n1: int, n2_blk: int, nblk: int, device="cuda"):
        """(nblk, table_rows(n2_blk), table_pitch(n1)) int32 view: nblk block tables
        laid out like alloc_table's, back to back (t_stride = rows * pitch)."""
        import torch
        rows, pitch = table_rows(n2_blk), table_pitch(n1)
        off = table_offset() if n1 >= 1 else 0
        flat = torch.empty(nblk * rows * pitch + 64, dtype=torch.int32, device=device)
        shift = (-(flat.data_ptr() // 4) + off) % 64
        return flat[shift:shift + nblk * rows * pitch].view(nblk, rows, pitch)

    def fill(self, d_s1, d_s2, table, scheme=(1, 0, -1), waves: int = 0, stream=None,
             sync: bool = True, flags: int = 0, substrips: int = 0, strip_waves: int = 0,
             timeout_ms: int = 0, mode: int = MODE_NW, kernel: int = KERNEL_AUTO):
        """d_s1/d_s2: int8/uint8 CUDA tensors; table: from alloc_table.  Returns NwResult
        when sync, else None (launch only)."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2.numel())
        assert table.dtype == torch.int32 and table.is_contiguous()
        assert table.shape[0] >= table_rows(n2) and table.shape[1] >= n1 + 1 and table.shape[1] % 64 == 0
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        sp = ctypes.c_void_p(stream.cuda_stream)
        p = params(scheme, waves, self.device, flags, substrips, strip_waves, timeout_ms, mode, kernel)
        args = (self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                ctypes.c_void_p(d_s2.data_ptr() if n2 else 0), n2, ctypes.byref(p),
                ctypes.c_void_p(table.data_ptr()), table.shape[1], sp)
        if sync:
            r = NwResult()
            st = lib().nw_fill_device(*args, ctypes.byref(r))
            if st != NW_OK:
                raise NwError(st, "nw_fill_device")
            return r
        st = lib().nw_fill_device_async(*args)
        if st != NW_OK:
            raise NwError(st, "nw_fill_device_async")
        return None

    def fill_band_cycle(self, d_s1, d_s2_blocks, n2_blk: int, tables, halo_in=None, halo_out=None,
                        hin_first: bool = False, hout_shift: int = 0, tag: int = 1, row0_max: int = 0,
                        scheme=(1, 0, -1), waves: int = 0, stream=None, flags: int = 0, substrips: int = 0,
                        strip_waves: int = 0, timeout_ms: int = 0, kernel: int = KERNEL_AUTO) -> None:
        """Launch one rank's blocks of block-cyclic row bands (asynchronous,
        nw_fill_band_cycle_async).  d_s2_blocks: the blocks' side characters, block
        k at [k * n2_blk, (k+1) * n2_blk); tables: alloc_cycle_tables(n1, n2_blk,
        nblk) (block k = tables[k]); halo_in / halo_out: raw device addresses of
        nblk-region halo buffers (Halo(..., regions=nblk).ptr or peer memory)."""
        import torch
        n1 = int(d_s1.numel())
        nblk = int(tables.shape[0])
        assert tables.dtype == torch.int32 and tables.is_contiguous() and tables.dim() == 3
        assert int(d_s2_blocks.numel()) == nblk * n2_blk
        assert tables.shape[1] >= table_rows(n2_blk) and tables.shape[2] >= n1 + 1 and tables.shape[2] % 64 == 0
        if stream is None:
            stream = torch.cuda.current_stream(tables.device)
        cy = NwBandCycle(halo_in, halo_out, nblk, int(bool(hin_first)), int(hout_shift), int(tag), int(row0_max),
                         int(tables.stride(0)))
        p = params(scheme, waves, self.device, flags, substrips, strip_waves, timeout_ms, kernel=kernel)
        st = lib().nw_fill_band_cycle_async(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                            ctypes.c_void_p(d_s2_blocks.data_ptr() if n2_blk else 0), n2_blk,
                                            ctypes.byref(p), ctypes.byref(cy), ctypes.c_void_p(tables.data_ptr()),
                                            tables.shape[2], ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, "nw_fill_band_cycle_async")

    def fill_band(self, d_s1, d_s2_band, table, halo_in=None, halo_out=None, tag: int = 1,
                  scheme=(1, 0, -1), waves: int = 0, stream=None, flags: int = 0,
                  substrips: int = 0, strip_waves: int = 0, row0: int = 0,
                  timeout_ms: int = 0, kernel: int = KERNEL_AUTO) -> None:
        """Launch one row band (asynchronous).  d_s2_band: the band's side
        characters (len = band rows - 1); table: alloc_table(n1, len(d_s2_band)),
        row 0 = the halo row, global row `row0` (nw_band_layout start).  halo_in /
        halo_out: int64 CUDA tensors of n1+1 granules or raw device addresses (peer
        memory from ipc_open_handle)."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2_band.numel())
        assert table.dtype == torch.int32 and table.is_contiguous()
        assert table.shape[0] >= table_rows(n2) and table.shape[1] >= n1 + 1 and table.shape[1] % 64 == 0

        def addr(x):
            if x is None:
                return None
            if isinstance(x, int):
                return x
            assert x.dtype == torch.int64 and x.numel() >= n1 + 1
            return x.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        b = NwBand(addr(halo_in), addr(halo_out), int(tag), int(row0))
        p = params(scheme, waves, self.device, flags, substrips, strip_waves, timeout_ms, kernel=kernel)
        st = lib().nw_fill_band_async(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                      ctypes.c_void_p(d_s2_band.data_ptr() if n2 else 0), n2,
                                      ctypes.byref(p), ctypes.byref(b),
                                      ctypes.c_void_p(table.data_ptr()), table.shape[1],
                                      ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, "nw_fill_band_async")

    def fill_colband(self, d_s1, d_s2, table, nbands: int, r: int, feed_in=None, feed_out=None,
                     tag: int = 1, scheme=(1, 0, -1), waves: int = 0, stream=None, flags: int = 0,
                     substrips: int = 0, strip_waves: int = 0, timeout_ms: int = 0,
                     kernel: int = KERNEL_AUTO) -> None:
        """Launch column band r of nbands (asynchronous).  d_s1 / d_s2: the WHOLE
        sequences; table: alloc_table(n_cols - 1, n2) for the band's colband_layout
        n_cols; feed_in / feed_out: Feed buffers' addresses (raw ints, e.g. peer
        memory from ipc_open_handle) or None at the ends."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2.numel())
        assert table.dtype == torch.int32 and table.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        b = NwColBand(feed_in, feed_out, int(tag), int(nbands), int(r), 0)
        p = params(scheme, waves, self.device, flags, substrips, strip_waves, timeout_ms, kernel=kernel)
        st = lib().nw_fill_colband_async(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                         ctypes.c_void_p(d_s2.data_ptr() if n2 else 0), n2, ctypes.byref(p),
                                         ctypes.byref(b), ctypes.c_void_p(table.data_ptr()), table.shape[1],
                                         ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, "nw_fill_colband_async")

    def fill_tband(self, d_s1, d_s2_band, table, row0: int = 0, feed_in=None, feed_out=None, tag: int = 1,
                   scheme=(1, 0, -1), waves: int = 0, stream=None, flags: int = 0,
                   timeout_ms: int = 0, substrips: int = 0, strip_waves: int = 0,
                   dense_polls: bool = False) -> None:
        """Launch one row band in horizontal strips (asynchronous, nw_fill_tband_async):
        the nw_fill_band contract (table: alloc_table(n1, len(d_s2_band)), row 0 =
        global row `row0` = the previous band's last row) with the band's rows swept
        as 256-row strips along the columns.  feed_in / feed_out: Feed(n1) buffers'
        addresses (raw ints, e.g. peer memory from ipc_open_handle), int64 CUDA tensors
        of feed_bytes(n1) / 8 granules, or None at the ends.  (substrips, strip_waves):
        the strip shape, (4, 1) (default) or (2, 2).  dense_polls: NW_TBAND_DENSE_POLLS
        (waiting strips poll with s_sleep 1: for chains of 1000+ strips)."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2_band.numel())
        assert table.dtype == torch.int32 and table.is_contiguous()
        assert table.shape[0] >= table_rows(n2) and table.shape[1] >= n1 + 1 and table.shape[1] % 64 == 0

        def addr(x):
            if x is None or isinstance(x, int):
                return x
            assert x.dtype == torch.int64 and x.numel() * 8 >= feed_bytes(n1)
            return x.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        b = NwTBand(addr(feed_in), addr(feed_out), int(tag), TBAND_DENSE_POLLS if dense_polls else 0, int(row0))
        p = params(scheme, waves, self.device, flags, substrips, strip_waves, timeout_ms)
        st = lib().nw_fill_tband_async(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                       ctypes.c_void_p(d_s2_band.data_ptr() if n2 else 0), n2, ctypes.byref(p),
                                       ctypes.byref(b), ctypes.c_void_p(table.data_ptr()), table.shape[1],
                                       ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, "nw_fill_tband_async")

    def sw_traceback(self, d_s1, d_s2, table, end, scheme=(1, -1, -1)):
        """Traceback of a device SW table (filled with mode=MODE_SW) from end = (i, j):
        (NwAlignment, ops) as sw_align."""
        n1, n2 = int(d_s1.numel()), int(d_s2.numel())
        ops = np.empty(end[0] + end[1] + 1, dtype=np.uint8)
        out = NwAlignment()
        p = params(scheme, device=self.device, mode=MODE_SW)
        st = lib().nw_sw_traceback(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                   ctypes.c_void_p(d_s2.data_ptr() if n2 else 0), n2, ctypes.byref(p),
                                   ctypes.c_void_p(table.data_ptr()), table.shape[1], int(end[0]), int(end[1]),
                                   ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ops.size,
                                   ctypes.byref(out))
        if st != NW_OK:
            raise NwError(st, "nw_sw_traceback")
        return out, ops[:out.n_ops].copy()

    def traceback(self, d_s1, d_s2, table, scheme=(1, 0, -1), stream=None, band: int = 0, max_windows: int = 0,
                  no_aim: bool = False):
        """Global traceback of a device table filled with mode=MODE_NW, from (n2, n1) to
        (0, 0) (nw_traceback): (NwAlignment, ops, NwTbStats) as align.  Ordered after the
        fill on `stream` (default: torch's current stream), which alone is synchronised."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2.numel())
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        ops = np.empty(max(n1 + n2, 1), dtype=np.uint8)
        out, stats = NwAlignment(), NwTbStats()
        p = params(scheme, device=self.device)
        o = tb_opts(band, max_windows, no_aim)
        st = lib().nw_traceback(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                ctypes.c_void_p(d_s2.data_ptr() if n2 else 0), n2, ctypes.byref(p),
                                ctypes.c_void_p(table.data_ptr()), table.shape[1], ctypes.byref(o),
                                ctypes.c_void_p(stream.cuda_stream), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                n1 + n2, ctypes.byref(out), ctypes.byref(stats))
        if st != NW_OK:
            raise NwError(st, "nw_traceback")
        return out, ops[:out.n_ops].copy(), stats

    def ckpt_sweep(self, d_s1, d_s2, K: int, scheme=(1, 0, -1), stream=None, waves: int = 0, flags: int = 0,
                   timeout_ms: int = 0, granules: bool = False):
        """The checkpoint sweep (nw_ckpt_sweep_async) of the table of (d_s1, d_s2), which
        is not stored: (score, rows) with rows the table's rows K, 2K, .. as an int32
        tensor of shape (nck, n1 + 1), nck = ceil(n2 / K) - 1.  granules=True returns the
        raw int64 granules {CKPT_TAG | t} instead -- row r is what fill_band takes as
        halo_in with tag=CKPT_TAG.  Synchronises `stream` and raises on a timeout."""
        import torch
        n1, n2 = int(d_s1.numel()), int(d_s2.numel())
        if stream is None:
            stream = torch.cuda.current_stream(d_s1.device)
        nck = ckpt_bytes(n1, n2, K) // (8 * (n1 + 1))
        with torch.cuda.stream(stream):
            gran = torch.zeros((nck, n1 + 1), dtype=torch.int64, device=d_s1.device)
            sc = torch.zeros(1, dtype=torch.int32, device=d_s1.device)
        p = params(scheme, waves, self.device, flags, timeout_ms=timeout_ms)
        st = lib().nw_ckpt_sweep_async(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                       ctypes.c_void_p(d_s2.data_ptr() if n2 else 0), n2, ctypes.byref(p), int(K),
                                       ctypes.c_void_p(gran.data_ptr() if nck else 0), ctypes.c_void_p(sc.data_ptr()),
                                       ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, "nw_ckpt_sweep_async")
        st = self.status(stream)
        if st != NW_OK:
            raise NwError(st, "nw_ckpt_sweep_async")
        if granules:
            return int(sc.item()), gran
        assert bool(((gran >> 32) == CKPT_TAG).all()), "checkpoint granule without its tag"
        return int(sc.item()), (gran & 0xFFFFFFFF).to(torch.int32)

    def score_batch(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, scheme=(1, 0, -1), stream=None,
                    waves: int = 0, flags: int = 0, gap_open=None, mat=None, band=None, piece2=None):
        """Scores of a batch on device tensors (nw_score_batch_async): d_s1cat / d_s2cat
        int8/uint8 CUDA tensors (the concatenations), d_off1 / d_off2 int64 CUDA tensors of
        npairs + 1 offsets, max_n2 >= every pair's n2.  Returns an int32 CUDA tensor of
        npairs scores, ordered on `stream` (default: torch's current stream); nothing is
        synchronised.  Pairs are claimed in index order: submit them longest first.
        gap_open (an int): affine gap cost, see score_batch_affine (Context.score_batch_affine).
        mat (a SubMatrix): substitution by matrix, see Context.score_batch_matrix.
        band (an int, with mat): inside a band, see Context.score_batch_banded.
        piece2 ((gap_open2, gap2), with mat): two-piece gap cost, see Context.score_batch_dual;
        with band as well: inside a band, see Context.score_batch_dual_banded."""
        m = () if mat is None else (ctypes.byref(mat.c), int(gap_open or 0))
        if mat is not None and piece2 is not None and band is not None:
            what, extra = "nw_score_batch_dual_banded_async", (*m, int(piece2[0]), int(piece2[1]), _band32(band))
        elif mat is not None and piece2 is not None:
            what, extra = "nw_score_batch_dual_async", (*m, int(piece2[0]), int(piece2[1]))
        elif mat is not None and band is not None:
            what, extra = "nw_score_batch_banded_async", (*m, _band32(band))
        elif mat is not None:
            what, extra = "nw_score_batch_matrix_async", m
        elif gap_open is None:
            what, extra = "nw_score_batch_async", ()
        else:
            what, extra = "nw_score_batch_affine_async", (int(gap_open),)
        return self._score_batch_async(what, d_s1cat, d_off1, d_s2cat, d_off2, max_n2,
                                       params(scheme, waves, self.device, flags), extra, stream)

    def _score_batch_async(self, entry: str, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, p: NwParams, extra,
                           stream, hits: bool = False):
        """One asynchronous score call: the C entry `entry` on the device tensors under `p`, with
        `extra` between the params and the results.  Returns the int32 CUDA tensor of npairs
        scores, or with `hits` of (npairs, 8) words in nw_local_hit's layout."""
        import torch
        npairs = int(d_off1.numel()) - 1
        assert d_off1.dtype == torch.int64 and d_off2.dtype == torch.int64 and int(d_off2.numel()) == npairs + 1
        assert d_off1.is_contiguous() and d_off2.is_contiguous()
        t1, t2 = int(d_s1cat.numel()), int(d_s2cat.numel())
        if stream is None:
            stream = torch.cuda.current_stream(d_off1.device)
        with torch.cuda.stream(stream):
            res = torch.zeros((max(npairs, 1), 8) if hits else max(npairs, 1), dtype=torch.int32,
                              device=d_off1.device)
        st = getattr(lib(), entry)(
            self._h, ctypes.c_void_p(d_s1cat.data_ptr() if t1 else 0), ctypes.c_void_p(d_off1.data_ptr()),
            ctypes.c_void_p(d_s2cat.data_ptr() if t2 else 0), ctypes.c_void_p(d_off2.data_ptr()), npairs, t1, t2,
            int(max_n2), ctypes.byref(p), *extra, ctypes.c_void_p(res.data_ptr()),
            ctypes.c_void_p(stream.cuda_stream))
        if st != NW_OK:
            raise NwError(st, entry)
        return res[:npairs]

    def score_batch_affine(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, scheme=(1, 0, -1), gap_open: int = 0,
                           stream=None, waves: int = 0, flags: int = 0):
        """score_batch under affine gap cost (nw_score_batch_affine_async): a run of L ups
        or of L lefts costs gap_open + L * scheme[2]."""
        return self.score_batch(d_s1cat, d_off1, d_s2cat, d_off2, max_n2, scheme, stream, waves, flags,
                                gap_open=int(gap_open))

    def score_batch_matrix(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -1,
                           gap_open: int = 0, stream=None, waves: int = 0):
        """score_batch_affine with substitution by matrix (nw_score_batch_matrix_async).  The
        sequences stay on the device and are not looked at: the matrix must name the
        letter unlisted bytes map to (SubMatrix(.., other=))."""
        _needs_other(mat, "Context.score_batch_matrix")
        return self.score_batch(d_s1cat, d_off1, d_s2cat, d_off2, max_n2, (1, 0, int(gap)), stream, waves, 0,
                                gap_open=int(gap_open), mat=mat)

    def score_batch_banded(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -1,
                           gap_open: int = 0, band: int = 0, stream=None, waves: int = 0):
        """Context.score_batch_matrix inside a band of `band` diagonals round each pair's own
        (nw_score_batch_banded_async, score_batch_banded)."""
        _needs_other(mat, "Context.score_batch_banded")
        return self.score_batch(d_s1cat, d_off1, d_s2cat, d_off2, max_n2, (1, 0, int(gap)), stream, waves, 0,
                                gap_open=int(gap_open), mat=mat, band=int(band))

    def score_batch_dual(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -2,
                         gap_open: int = -4, gap2: int = -1, gap_open2: int = -24, stream=None, waves: int = 0):
        """Context.score_batch_matrix under the two-piece gap cost max(gap_open + L * gap,
        gap_open2 + L * gap2) per run of L (nw_score_batch_dual_async, score_batch_dual)."""
        _needs_other(mat, "Context.score_batch_dual")
        return self.score_batch(d_s1cat, d_off1, d_s2cat, d_off2, max_n2, (1, 0, int(gap)), stream, waves, 0,
                                gap_open=int(gap_open), mat=mat, piece2=(int(gap_open2), int(gap2)))

    def score_batch_dual_banded(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -2,
                                gap_open: int = -4, gap2: int = -1, gap_open2: int = -24, band: int = 0,
                                stream=None, waves: int = 0):
        """Context.score_batch_dual inside a band of `band` diagonals round each pair's own
        (nw_score_batch_dual_banded_async, score_batch_dual_banded)."""
        _needs_other(mat, "Context.score_batch_dual_banded")
        return self.score_batch(d_s1cat, d_off1, d_s2cat, d_off2, max_n2, (1, 0, int(gap)), stream, waves, 0,
                                gap_open=int(gap_open), mat=mat, band=int(band),
                                piece2=(int(gap_open2), int(gap2)))

    def score_batch_local(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -1,
                          gap_open: int = 0, stream=None, waves: int = 0):
        """Local alignment hits of a batch on device tensors (nw_score_batch_local_async):
        the arguments of Context.score_batch_matrix.  Returns an int32 CUDA tensor (npairs,
        8), a row in nw_local_hit's layout: score, end_i, end_j, begin_i = begin_j = -1,
        three zeros; a pair longer than max_n2: INT32_MIN and -1 in the four coordinates.
        Ordered on `stream`; nothing is synchronised."""
        _needs_other(mat, "Context.score_batch_local")
        return self._score_batch_async("nw_score_batch_local_async", d_s1cat, d_off1, d_s2cat, d_off2, max_n2,
                                       params((1, 0, int(gap)), waves, self.device, mode=MODE_SW),
                                       (ctypes.byref(mat.c), int(gap_open)), stream, hits=True)

    def score_batch_semi(self, d_s1cat, d_off1, d_s2cat, d_off2, max_n2: int, mat: SubMatrix, gap: int = -1,
                         gap_open: int = 0, ends: int = ENDS_S2_IN_S1, stream=None, waves: int = 0):
        """Semi-global alignment hits of a batch on device tensors (nw_score_batch_semi_async):
        the arguments of Context.score_batch_local and `ends` (ENDS_* bits).  Returns an int32
        CUDA tensor (npairs, 8) in nw_local_hit's layout: score, end_i, end_j, begin_i =
        begin_j = -1, three zeros; a pair longer than max_n2: INT32_MIN and -1 in the four
        coordinates.  Ordered on `stream`; nothing is synchronised."""
        _needs_other(mat, "Context.score_batch_semi")
        return self._score_batch_async("nw_score_batch_semi_async", d_s1cat, d_off1, d_s2cat, d_off2, max_n2,
                                       params((1, 0, int(gap)), waves, self.device),
                                       (ctypes.byref(mat.c), int(gap_open), int(ends)), stream, hits=True)

    def traceback_block(self, d_s1, d_s2_block, table, row0: int, scheme=(1, 0, -1), stream=None, band: int = 0,
                        max_windows: int = 0, no_aim: bool = False):
        """Traceback of one row block (nw_traceback_block): table rows 0..len(d_s2_block)
        hold global rows row0 .. of the table over columns 0..len(d_s1) (as fill_band
        leaves them).  (NwAlignment, ops, NwTbStats): the walk from the block's last row
        at column n1 to its row 0 -- begin_j is where it arrived."""
        import torch
        n1, rows = int(d_s1.numel()), int(d_s2_block.numel())
        if stream is None:
            stream = torch.cuda.current_stream(table.device)
        ops = np.empty(max(n1 + rows, 1), dtype=np.uint8)
        out, stats = NwAlignment(), NwTbStats()
        p = params(scheme, device=self.device)
        o = tb_opts(band, max_windows, no_aim)
        st = lib().nw_traceback_block(self._h, ctypes.c_void_p(d_s1.data_ptr() if n1 else 0), n1,
                                      ctypes.c_void_p(d_s2_block.data_ptr() if rows else 0), rows, int(row0),
                                      ctypes.byref(p), ctypes.c_void_p(table.data_ptr()), table.shape[1],
                                      ctypes.byref(o), ctypes.c_void_p(stream.cuda_stream),
                                      ops.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n1 + rows,
                                      ctypes.byref(out), ctypes.byref(stats))
        if st != NW_OK:
            raise NwError(st, "nw_traceback_block")
        return out, ops[:out.n_ops].copy(), stats

    def set_trace(self, trace_tensor) -> None:
        """Debug: per-strip timeline (start, end, waits, ...: tools/trace_strips.py) into
        a uint64/int64 CUDA tensor of at least strips * trace_words() elements (None = off)."""
        if trace_tensor is not None:
            assert trace_tensor.element_size() == 8
        lib().nw_debug_set_trace(self._h, ctypes.c_void_p(trace_tensor.data_ptr() if trace_tensor is not None else 0))

    def debug_ctrl(self) -> list[int]:
        """The 8 control words of the last launch (include/nw_hip.h nw_debug_ctrl)."""
        out = (ctypes.c_uint32 * 8)()
        st = lib().nw_debug_ctrl(self._h, out)
        if st != NW_OK:
            raise NwError(st, "nw_debug_ctrl")
        return list(out)

    def debug_failure(self) -> list[int]:
        """The first failure recorded on this context (include/nw_hip.h nw_debug_failure):
        [code, site word, need, seen, failed launches], pending or as the last status() cleared it."""
        out = (ctypes.c_uint32 * 5)()
        st = lib().nw_debug_failure(self._h, out)
        if st != NW_OK:
            raise NwError(st, "nw_debug_failure")
        return list(out)

    def status(self, stream=None) -> int:
        """NW_ERR_TIMEOUT if any launch on this context since the last call gave up
        (nw_ctx_status: read and cleared), else NW_OK."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream()
        return int(lib().nw_ctx_status(self._h, ctypes.c_void_p(stream.cuda_stream)))
