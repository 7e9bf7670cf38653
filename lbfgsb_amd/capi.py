"""ctypes bindings of include/lbfgsb_hip.h and include/lbfgsb_hip_debug.h (one prototype per declared symbol)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/lbfgsb_hip.h declares: name -> (restype, argtypes)
_vp, _i32p, _dp, _cp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_char_p
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
FG_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p, C.c_void_p)
PROTOTYPES = {
    "lbfgsb_hip_create": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    _vp, C.POINTER(_vp)]),
    "lbfgsb_hip_destroy": (None, [_vp]),
    "lbfgsb_hip_last_error": (C.c_char_p, []),
    "lbfgsb_hip_rccl_unique_id": (C.c_int, [_vp]),
    "lbfgsb_hip_comm_init_rccl": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "lbfgsb_hip_comm_init_host": (C.c_int, [_vp, ALLREDUCE_FN, ALLGATHER_FN, _vp, C.c_int, C.c_int]),
    "lbfgsb_hip_setulb_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double,
                                        _vp, C.c_int, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_setulb_dev_pp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double,
                                           C.c_double, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_setulb_host": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp,
                                         C.c_double, C.c_double, _vp, _vp, _vp, C.c_int32, _vp,
                                         _vp, _vp, _vp, _cp, C.c_int32, C.c_int32]),
    "lbfgsb_hip_setulb_host_ik": (C.c_int, [C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp,
                                            C.c_double, C.c_double, _vp, _vp, _vp, C.c_int64, _vp,
                                            _vp, _vp, _vp, _cp, C.c_int32, C.c_int32, C.c_int32]),
    "lbfgsb_hip_release_host_ik": (C.c_int, [_vp, C.c_int32]),
    "lbfgsb_hip_pass_clock": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "lbfgsb_hip_get_stream": (C.c_void_p, [_vp]),
    "lbfgsb_hip_wait_stream": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_release_host": (C.c_int, [_vp]),
    "lbfgsb_hip_host_pinning": (C.c_int, [C.c_int]),
    "lbfgsb_hip_return_event": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "lbfgsb_hip_f_device": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "lbfgsb_hip_tie_splits": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_defer_stats": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_host_gap": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_collective_time": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "lbfgsb_hip_compact_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_dense_launches": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_ub_launches": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_host_segments": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_comm_info": (C.c_int, [_vp, _vp, _vp, _vp]),
    "lbfgsb_hip_path_counts": (C.c_int, [_vp, _vp, _vp, _vp]),
    "lbfgsb_hip_minimize": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_int,
                                      C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_export_state": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_qn_apply": (C.c_int, [_vp, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "lbfgsb_hip_qn_diag": (C.c_int, [_vp, C.c_int, _vp]),
    "lbfgsb_hip_qn_logdet": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_draw": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_uint64, C.c_int64, _vp, C.c_double, _vp,
                                     C.c_int64]),
    "lbfgsb_hip_qn_quad": (C.c_int, [_vp, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_gram": (C.c_int, [_vp, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_double),
                                     C.c_int64]),
    "lbfgsb_hip_qn_logpdf": (C.c_int, [_vp, C.c_int, C.c_int64, _vp, C.c_int64, _vp, C.c_double,
                                       C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_draw_logpdf": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_uint64, C.c_int64, _vp, C.c_double, _vp,
                                            C.c_int64, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_eig": (C.c_int, [_vp, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_eigvec": (C.c_int, [_vp, C.c_int, C.c_int64, C.POINTER(C.c_int32), _vp, C.c_int64]),
    "lbfgsb_hip_qn_shift_set": (C.c_int, [_vp, _vp, C.c_double, C.POINTER(C.c_int64)]),
    "lbfgsb_hip_qn_shift_solve": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "lbfgsb_hip_qn_shift_logdet": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_shift_diag": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_qn_rows": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int64]),
    "lbfgsb_hip_qn_block": (C.c_int, [_vp, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int64,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int64]),
    "lbfgsb_hip_qn_cols": (C.c_int, [_vp, C.c_int, C.c_int64, C.POINTER(C.c_int64), _vp, C.c_int64]),
    "lbfgsb_hip_qn_shift_block": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_double), C.c_int64]),
    "lbfgsb_hip_qn_shift_cols": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_int64), _vp, C.c_int64]),
    "lbfgsb_hip_qn_pairs_get": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), _vp, C.c_int64,
                                          _vp, C.c_int64]),
    "lbfgsb_hip_qn_pairs_set": (C.c_int, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64, C.c_double]),
    "lbfgsb_hip_qn_pairs_push": (C.c_int, [_vp, _vp, _vp, C.c_double, C.POINTER(C.c_int32)]),
    "lbfgsb_hip_qn_shift_sqrt": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "lbfgsb_hip_qn_shift_draw": (C.c_int, [_vp, C.c_int64, C.c_uint64, C.c_int64, _vp, C.c_double, _vp, C.c_int64]),
    "lbfgsb_hip_qn_shift_draw_logpdf": (C.c_int, [_vp, C.c_int64, C.c_uint64, C.c_int64, _vp, C.c_double, _vp,
                                                  C.c_int64, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_shift_quad": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_shift_logpdf": (C.c_int, [_vp, C.c_int64, _vp, C.c_int64, _vp, C.c_double,
                                             C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_path_set": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_int64)]),
    "lbfgsb_hip_qn_path_logdet": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_int32)]),
    "lbfgsb_hip_qn_path_solve": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_double), _vp, C.c_int64,
                                           C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lbfgsb_hip_qn_path_trust": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_int, _vp, C.POINTER(C.c_double),
                                           C.POINTER(C.c_int32)]),
    "lbfgsb_hip_kkt": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_kkt_list": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int64, _vp]),
    "lbfgsb_hip_import_state": (C.c_int, [_vp, _vp, _vp, _vp]),
    "lbfgsb_hip_projgr": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_wtv": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    "lbfgsb_hip_set_w": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_set_iwhere": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_formk_gram": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "lbfgsb_hip_wtv_launch_only": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "lbfgsb_hip_wtv_time": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "lbfgsb_hip_kernel_time": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "lbfgsb_hip_sync": (C.c_int, [_vp]),
    "lbfgsb_hip_objective": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "lbfgsb_hip_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_set_option": (C.c_int, [_vp, _cp, C.c_double]),
    "lbfgsb_hip_comm_stats": (C.c_int, [_vp, _vp, _vp]),
    "lbfgsb_hip_uniform_bounds": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_bounds_changed": (C.c_int, [_vp]),
    "lbfgsb_hip_bounds_stats": (C.c_int, [_vp, _vp, _vp, _vp]),
    "lbfgsb_hip_freev_skipped": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_skip_stats": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_refresh_count": (C.c_int, [_vp, _vp]),
    "lbfgsb_hip_vec_sub": (C.c_int, [_vp, _vp, _vp, _vp]),
    "lbfgsb_hip_vec_scale": (C.c_int, [_vp, C.c_double, _vp]),
    "lbfgsb_hip_dot": (C.c_int, [_vp, _vp, _vp, _vp]),
    # routine doors
    "lbfgsb_hip_active": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_errclb": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "lbfgsb_hip_cauchy": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, C.c_double,
                                    _vp, _vp, _vp]),
    "lbfgsb_hip_freev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_formk": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp]),
    "lbfgsb_hip_cmprlb": (C.c_int, [_vp, _vp, _vp, C.c_double, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "lbfgsb_hip_subsm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _vp, _vp,
                                   _vp]),
    "lbfgsb_hip_lnsrlb": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lbfgsb_hip_matupd": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp]),
}

E_NOGPU, E_ARG, E_ALLOC, E_COMM, E_STATE = -100, -101, -102, -103, -104   # status codes of include/lbfgsb_hip.h
QN_B, QN_H = 0, 1  # lbfgsb_hip_qn_apply / lbfgsb_hip_qn_diag: the model B, its inverse H = B^-1
QN_B_SQRT, QN_H_SQRT = 4, 5  # lbfgsb_hip_qn_apply only: the symmetric square roots B^(1/2), H^(1/2)
QN_ROOT_MAXCOL = 64
QN_PATH_MAXK = 64  # lbfgsb_hip_qn_path_solve: the most shifts of a call
QN_IDX_MAXK = 4096  # lbfgsb_hip_qn_rows / qn_block / qn_shift_block: the longest index list of a call
QN_EIG_CUT = 1e-8  # lbfgsb_hip_qn_eig: directions with |lambda - bulk| <= QN_EIG_CUT * bulk count as bulk
# lbfgsb_hip_kkt: the slots of h_cnt and h_val (LBFGSB_KKT_* without the prefix, in index order) -- the field names
# of solver.KktReport
KKT_CNT = ("n_unbounded", "n_free", "n_lower", "n_upper", "n_fixed", "n_binding", "n_weak", "n_leaving", "n_outside")
KKT_VAL = ("pg_max", "mult_max", "out_max", "gfree_max")
F_REAL32 = 1
F_MIRROR_INDEX = 2
F_NO_RETURN_SYNC = 4
F_PARALLEL_GCP = 8
F_EXACT_TIES = 16      # accepted and ignored: the default since round 3
F_INDEX_TIES = 32      # opt-out: equal breakpoints in variable order, no heap-order replay
F_DEFER_LNSRCH = 64    # the line-search set-up's sums travel with the next call's fetch (same-stream objective)
F_FOLLOW_BOUNDS = 128  # every entry compares l, u, nbd with the snapshot and follows an edit, as the reference does


class LbfgsbError(RuntimeError):
    pass


def lib_path() -> str:
    # LBFGSB_HIP_LIBRARY: another build of the same ABI (A/B timing of two builds on one box)
    return os.environ.get("LBFGSB_HIP_LIBRARY") or os.path.join(HERE, "liblbfgsb_hip.so")


def build_library() -> str:
    """hipcc --offload-arch=gfx950 ... (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "csrc")])
    return lib_path()


def load_library():
    """Load the HIP library.  torch is imported first so that both share one HIP runtime."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise LbfgsbError("%s is missing: run lbfgsb_amd.build_library() (hipcc, gfx950). "
                          "There is no CPU fallback." % path)
    try:
        import torch  # noqa: F401  (loads libamdhip64 that this library then binds to)
    except Exception:
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load_library().lbfgsb_hip_last_error()
        raise LbfgsbError("lbfgsb_hip error %d: %s" % (rc, (msg or b"").decode()))
