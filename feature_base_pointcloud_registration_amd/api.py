"""Python front-end of libfbr_hip.so (the extern "C" boundary of include/fbr.h).

The classes mirror the reference's per-scan operator interface so that tests read like the
reference's own call sites:

  ImageProjection.projectPointCloud/cloudExtraction  -> Context.project()      imageProjection.cpp:583-670
  FeatureExtraction.featureExtra                     -> Context.extract_features() featureExtraction.h:79
  mapOptimization.registration                       -> Context.register()     mapOptmization.h:263
  cloudHandler (projection -> features -> registration) -> Context.process_scan()  imageProjection.cpp:182

There is no CPU fallback: if the HIP library or a GPU is missing every call raises.
"""
import ctypes
import os

import numpy as np

from .fbr_types import (DESKEW_TABLE, GUESS_STATE, IMU_SAMPLE, MOTION, ODOM_INFO, ODOM_SAMPLE, KEYPOSE, PF_FLOAT32, POINT_XYZI, POINT_XYZIRT, REG_STATS, FbrIcpResult,
                        FbrGmapResult, FbrLoopPair, FbrLoopResult, FbrParams, FbrPgMarginalResult, FbrPgResult, FbrRegStats, FbrScMatch,
                        POSE_SCORE, REG_INFO, PointCloud2, default_params, gmap_params, icp_params, info_params, loop_params,
                        pg_marginal_params, pg_params, pose_lattice, ptr, sc_params, score_params)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_VP = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32

EXPORTED_SYMBOLS = [
    "fbr_params_default", "fbr_strerror", "fbr_abi_version", "fbr_device_count", "fbr_create",
    "fbr_destroy", "fbr_set_map", "fbr_get_map", "fbr_project", "fbr_extract_features",
    "fbr_register", "fbr_register_trace", "fbr_process_scan", "fbr_reset_stream",
    "fbr_process_batch", "fbr_ingest_bytes", "fbr_debug_counters", "fbr_map_grid_info", "fbr_batch_stage", "fbr_batch_launch", "fbr_batch_wait",
    "fbr_batch_flush", "fbr_batch_export_ready", "fbr_batch_results", "fbr_batch_set_full_masks", "fbr_batch_labels", "fbr_diag_batch_cloud", "fbr_diag_knn_last", "fbr_diag_gn_last", "fbr_batch_export", "fbr_batch_bytes", "fbr_set_profiling", "fbr_set_profiling_kernels", "fbr_kernel_time", "fbr_stream",
    "fbr_voxel_grid", "fbr_affine_from_pose", "fbr_pose_from_affine", "fbr_selftest_math", "fbr_selftest_eigen6", "fbr_selftest_gn_rows", "fbr_selftest_gn_reduce", "fbr_selftest_solve6", "fbr_selftest_eig_certified", "fbr_selftest_voxel_order", "fbr_selftest_radix_sort",
    "fbr_load_map", "fbr_pcd_read", "fbr_pcd_write_ascii", "fbr_pcd_write_binary",
    "fbr_msg_to_points", "fbr_points_to_msg_data", "fbr_project_msg", "fbr_process_msg",
    "fbr_imu_convert", "fbr_imu_deskew_info", "fbr_set_deskew", "fbr_odom_deskew_info", "fbr_motion_from_poses", "fbr_update_initial_guess", "fbr_set_motion",
    "fbr_stream_copy_bandwidth", "fbr_valu_peak",
    "fbr_keyframe_params_default", "fbr_keyframes_add", "fbr_keyframes_set_pose", "fbr_keyframes_count",
    "fbr_keyframes_reset", "fbr_extract_surrounding_keyframes",
    "fbr_loop_params_default", "fbr_detect_loop_closure", "fbr_perform_loop_closure", "fbr_icp_align", "fbr_selftest_nn1",
    "fbr_loop_candidates", "fbr_perform_loop_closures", "fbr_icp_align_batch",
    "fbr_sc_params_default", "fbr_sc_describe", "fbr_sc_update", "fbr_sc_descriptor", "fbr_sc_query",
    "fbr_sc_detect_loop_closure", "fbr_perform_loop_closure_sc",
    "fbr_pg_params_default", "fbr_pg_reset", "fbr_pg_add_prior", "fbr_pg_add_between", "fbr_pg_add_between_poses",
    "fbr_pg_add_gps", "fbr_pg_add_loop", "fbr_pg_factor_count", "fbr_pg_optimize", "fbr_pg_poses", "fbr_pg_apply",
    "fbr_pg_loop_weights",
    "fbr_pg_marginal_params_default", "fbr_pg_marginals", "fbr_pg_gps_gate",
    "fbr_gmap_params_default", "fbr_global_map_build", "fbr_global_map_get", "fbr_global_map_install",
    "fbr_global_map_save", "fbr_pcd_write_poses_ascii", "fbr_selftest_voxel_wide",
    "fbr_score_params_default", "fbr_score_poses", "fbr_pose_search",
    "fbr_info_params_default", "fbr_reg_info_poses", "fbr_batch_info", "fbr_reg_info_variances",
    "fbr_comm_unique_id", "fbr_comm_create", "fbr_comm_create_local", "fbr_comm_destroy", "fbr_batch_allgather",
]


class FbrError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        super().__init__(f"{where}: {strerror(status)} ({status})")


def lib_path():
    # FBR_LIB selects a diagnostic build (tools/); the default is the shipped library
    return os.environ.get("FBR_LIB") or os.path.join(_HERE, "libfbr_hip.so")


def lib():
    """Load the HIP library (raises if it was not built: no silent fallback)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is not built "
                               "(run __graft_entry__.build())")
        L = ctypes.CDLL(path)
        sig = {
            "fbr_params_default": (None, [_VP]),
            "fbr_strerror": (ctypes.c_char_p, [ctypes.c_int]),
            "fbr_abi_version": (ctypes.c_int, []),
            "fbr_device_count": (ctypes.c_int, [_VP]),
            "fbr_create": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
            "fbr_destroy": (ctypes.c_int, [_VP]),
            "fbr_set_map": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64]),
            "fbr_get_map": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
            "fbr_project": (ctypes.c_int, [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP]),
            "fbr_extract_features": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP]),
            "fbr_register": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64, _VP, _VP]),
            "fbr_register_trace": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64, _VP, _VP, _VP]),
            "fbr_process_scan": (ctypes.c_int, [_VP, _VP, _I64, ctypes.c_double, _VP, _VP]),
            "fbr_reset_stream": (ctypes.c_int, [_VP]),
            "fbr_process_batch": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP, _VP]),
            "fbr_ingest_bytes": (ctypes.c_int, [_VP, _VP]),
            "fbr_map_grid_info": (ctypes.c_int, [_VP, _VP]),
            "fbr_debug_counters": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int]),
            "fbr_batch_stage": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, _VP]),
            "fbr_batch_launch": (ctypes.c_int, [_VP]),
            "fbr_batch_wait": (ctypes.c_int, [_VP]),
            "fbr_batch_results": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_batch_export": (ctypes.c_int, [_VP, _VP]),
            "fbr_batch_set_full_masks": (ctypes.c_int, [_VP, ctypes.c_int]),
            "fbr_batch_labels": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _I64, _VP]),
            "fbr_batch_flush": (ctypes.c_int, [_VP]),
            "fbr_batch_export_ready": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
            "fbr_batch_bytes": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_set_profiling": (ctypes.c_int, [_VP, ctypes.c_int]),
            "fbr_set_profiling_kernels": (ctypes.c_int, [_VP, ctypes.c_char_p]),
            "fbr_kernel_time": (ctypes.c_int, [_VP, ctypes.c_char_p, _VP, _VP]),
            "fbr_stream": (_VP, [_VP]),
            "fbr_voxel_grid": (ctypes.c_int, [_VP, _VP, _I64, ctypes.c_float, _VP, _VP]),
            "fbr_affine_from_pose": (None, [_VP, _VP]),
            "fbr_pose_from_affine": (None, [_VP, _VP]),
            "fbr_selftest_math": (ctypes.c_int, [ctypes.c_int, _VP, _VP, _VP]),
            "fbr_selftest_eigen6": (ctypes.c_int, [ctypes.c_int, _VP, _VP]),
            "fbr_selftest_eig_certified": (ctypes.c_int, [ctypes.c_int, _VP, ctypes.c_float, _VP]),
            "fbr_selftest_gn_rows": (ctypes.c_int, [ctypes.c_int, _VP, _VP]),
            "fbr_selftest_gn_reduce": (ctypes.c_int, [ctypes.c_int, _VP, _VP, _VP]),
            "fbr_selftest_solve6": (ctypes.c_int, [ctypes.c_int, _VP, _VP, _VP, _VP, _VP]),
            "fbr_selftest_voxel_order": (ctypes.c_int, [_I64, _VP, ctypes.c_int, _VP]),
            "fbr_selftest_radix_sort": (ctypes.c_int, [_I64, ctypes.c_int, ctypes.c_int, _VP, _VP]),
            "fbr_load_map": (ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_char_p]),
            "fbr_pcd_read": (ctypes.c_int, [ctypes.c_char_p, _VP, _I64, _VP]),
            "fbr_pcd_write_ascii": (ctypes.c_int, [ctypes.c_char_p, _VP, _I64]),
            "fbr_pcd_write_binary": (ctypes.c_int, [ctypes.c_char_p, _VP, _I64]),
            "fbr_msg_to_points": (ctypes.c_int, [_VP, _VP, _I64, _VP, _VP]),
            "fbr_points_to_msg_data": (ctypes.c_int, [_VP, _I64, _VP]),
            "fbr_project_msg": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
            "fbr_process_msg": (ctypes.c_int, [_VP, _VP, ctypes.c_double, _VP, _VP, _VP]),
            "fbr_imu_convert": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_imu_deskew_info": (ctypes.c_int, [_VP, _I64, ctypes.c_double, ctypes.c_double, _VP, _VP]),
            "fbr_set_deskew": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
            "fbr_odom_deskew_info": (ctypes.c_int, [_VP, _I64, ctypes.c_double, ctypes.c_double, _VP, _VP]),
            "fbr_motion_from_poses": (ctypes.c_int, [_VP, _VP, ctypes.c_double, ctypes.c_double, ctypes.c_double, _VP, _VP]),
            "fbr_update_initial_guess": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, _VP]),
            "fbr_set_motion": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
            "fbr_stream_copy_bandwidth": (ctypes.c_int, [ctypes.c_int, _I64, ctypes.c_int, _VP]),
            "fbr_valu_peak": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _VP, _VP]),
            "fbr_keyframe_params_default": (None, [_VP]),
            "fbr_keyframes_add": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64]),
            "fbr_keyframes_set_pose": (ctypes.c_int, [_VP, _I64, _VP]),
            "fbr_keyframes_count": (ctypes.c_int, [_VP, _VP]),
            "fbr_keyframes_reset": (ctypes.c_int, [_VP]),
            "fbr_extract_surrounding_keyframes": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP, _VP, _VP]),
            "fbr_loop_params_default": (None, [_VP]),
            "fbr_detect_loop_closure": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP, _VP]),
            "fbr_perform_loop_closure": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP]),
            "fbr_icp_align": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64, _VP, _VP]),
            "fbr_loop_candidates": (ctypes.c_int, [_VP, _VP, _I32, _VP, _I64, _VP]),
            "fbr_perform_loop_closures": (ctypes.c_int, [_VP, _VP, _VP, _I64, _I32, _VP]),
            "fbr_icp_align_batch": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _I64, _VP, _I32, _VP]),
            "fbr_selftest_nn1": (ctypes.c_int, [_VP, _VP, _I64, _VP, _I64, ctypes.c_float, _VP, _VP]),
            "fbr_sc_params_default": (None, [_VP]),
            "fbr_sc_describe": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, _VP]),
            "fbr_sc_update": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_sc_descriptor": (ctypes.c_int, [_VP, _I64, _VP]),
            "fbr_sc_query": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, ctypes.c_int, _VP, _VP]),
            "fbr_sc_detect_loop_closure": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP, _VP, _VP, _VP]),
            "fbr_perform_loop_closure_sc": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP, _VP, _VP]),
            "fbr_pg_params_default": (None, [_VP]),
            "fbr_pg_reset": (ctypes.c_int, [_VP]),
            "fbr_pg_add_prior": (ctypes.c_int, [_VP, _I64, _VP, _VP]),
            "fbr_pg_add_between": (ctypes.c_int, [_VP, _I64, _I64, _VP, _VP]),
            "fbr_pg_add_between_poses": (ctypes.c_int, [_VP, _I64, _I64, _VP, _VP, _VP]),
            "fbr_pg_add_gps": (ctypes.c_int, [_VP, _I64, _VP, _VP]),
            "fbr_pg_add_loop": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_pg_factor_count": (ctypes.c_int, [_VP, _VP]),
            "fbr_pg_optimize": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_pg_poses": (ctypes.c_int, [_VP, _VP, _I64, _VP]),
            "fbr_pg_apply": (ctypes.c_int, [_VP]),
            "fbr_pg_loop_weights": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I64, _VP]),
            "fbr_pg_marginal_params_default": (None, [_VP]),
            "fbr_pg_marginals": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, _VP]),
            "fbr_pg_gps_gate": (ctypes.c_int, [_VP, ctypes.c_double, _VP, _VP]),
            "fbr_gmap_params_default": (None, [_VP]),
            "fbr_global_map_build": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_global_map_get": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
            "fbr_global_map_install": (ctypes.c_int, [_VP]),
            "fbr_global_map_save": (ctypes.c_int, [_VP, ctypes.c_char_p, _I32]),
            "fbr_pcd_write_poses_ascii": (ctypes.c_int, [ctypes.c_char_p, _VP, _I64]),
            "fbr_selftest_voxel_wide": (ctypes.c_int, [_VP, _VP, _I64, ctypes.c_float, _VP, _VP]),
            "fbr_score_params_default": (None, [_VP]),
            "fbr_score_poses": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _VP]),
            "fbr_info_params_default": (None, [_VP]),
            "fbr_reg_info_poses": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, _VP, _I64, _VP]),
            "fbr_batch_info": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_reg_info_variances": (ctypes.c_int, [_VP, _VP, _VP]),
            "fbr_pose_search": (ctypes.c_int, [_VP, _VP, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _VP, _VP, _VP]),
            "fbr_comm_unique_id": (ctypes.c_int, [_VP]),
            "fbr_comm_create": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
            "fbr_comm_create_local": (ctypes.c_int, [_VP, _VP, ctypes.c_int, ctypes.c_int]),
            "fbr_comm_destroy": (ctypes.c_int, [_VP]),
            "fbr_batch_allgather": (ctypes.c_int, [_VP, _VP, _I64, _VP, _VP, _VP]),
        }
        diag = bool(os.environ.get("FBR_LIB"))  # an A/B build of another round may lack newer entry points
        for name, (res, args) in sig.items():
            if diag and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def strerror(status):
    return lib().fbr_strerror(status).decode()


def _check(status, where):
    if status != 0:
        raise FbrError(status, where)


def device_count():
    n = ctypes.c_int(0)
    _check(lib().fbr_device_count(ctypes.byref(n)), "fbr_device_count")
    return n.value


def debug_counters(reset=False):
    """(kernel launches, blocking host syncs, GN flag polls) since the last reset (process-wide)."""
    v = [ctypes.c_longlong() for _ in range(3)]
    _check(lib().fbr_debug_counters(*[ctypes.byref(x) for x in v], int(reset)), "fbr_debug_counters")
    return tuple(x.value for x in v)


def host_times(reset=False):
    """Host wall time (s) of the single-scan calls since the last reset: (upload, stage enqueue,
    result wait, whole call) -- diagnostic (fbr_diag_host_times)."""
    f = lib().fbr_diag_host_times
    f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
    v = (ctypes.c_longlong * 4)()
    _check(f(v, int(reset)), "fbr_diag_host_times")
    return tuple(x * 1e-9 for x in v)


def wait_stats(reset=False):
    """Host waits on device results since the last reset -- diagnostic (fbr_diag_wait_stats):
    (fallbacks: a flag or direct result not visible although its stream drained, waits longer than
    1 ms, the longest wait in s, stream queries)."""
    if not hasattr(lib(), "fbr_diag_wait_stats"):  # an A/B build of an earlier round (FBR_LIB)
        return -1, -1, -1.0, -1
    f = lib().fbr_diag_wait_stats
    f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
    v = (ctypes.c_longlong * 4)()
    _check(f(v, int(reset)), "fbr_diag_wait_stats")
    return int(v[0]), int(v[1]), v[2] * 1e-9, int(v[3])


def live_resources():
    """What the process's contexts and communicators hold now: (device blocks, pinned blocks,
    streams, events) -- diagnostic (fbr_diag_live_resources).  Back at its earlier value once they
    are closed."""
    if not hasattr(lib(), "fbr_diag_live_resources"):  # an A/B build of an earlier round (FBR_LIB)
        return -1, -1, -1, -1
    f = lib().fbr_diag_live_resources
    f.restype, f.argtypes = ctypes.c_int, [_VP]
    v = (ctypes.c_longlong * 4)()
    _check(f(v), "fbr_diag_live_resources")
    return tuple(int(x) for x in v)


def batch_times(reset=False):
    """Host wall time (s) of fbr_batch_launch calls since the last reset, and the part of it spent
    waiting for the Gauss-Newton iteration flags -- diagnostic (fbr_diag_batch_times)."""
    f = lib().fbr_diag_batch_times
    f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
    v = (ctypes.c_longlong * 2)()
    _check(f(v, int(reset)), "fbr_diag_batch_times")
    return tuple(x * 1e-9 for x in v)


def knn_tile_stats(reset=False):
    """Block-tile kNN counters since the last reset: (queries, binned queries, tiles built, points
    in tiles, points scanned by the tile loads, tiles over capacity, 0, 0), or None unless
    FBR_KNN_TILE_STATS=1 -- diagnostic (fbr_diag_knn_tile_stats, k_knn_tile.hip)."""
    f = lib().fbr_diag_knn_tile_stats
    f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
    v = (ctypes.c_ulonglong * 8)()
    if f(v, int(reset)) != 0:
        return None
    return tuple(int(x) for x in v)


def selftest_math(a, b):
    """Device sqrt(|a|), a/b, atan2f(a,b), a*b+b*a-a, sinf(a), cosf(a) (see fbr_selftest_math)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    out = np.zeros((len(a), 6), np.float32)
    _check(lib().fbr_selftest_math(len(a), ptr(a), ptr(b), ptr(out)), "fbr_selftest_math")
    return out


def selftest_eigen6(mats):
    """cv::eigen of symmetric 6x6 float matrices on the device (see fbr_selftest_eigen6): returns
    (single-lane (W, V), wave-parallel (W, V)), W (n, 6) descending, V (n, 6, 6) rows = vectors."""
    a = np.ascontiguousarray(mats, np.float32).reshape(-1, 36)
    out = np.zeros((len(a), 84), np.float32)
    _check(lib().fbr_selftest_eigen6(len(a), ptr(a), ptr(out)), "fbr_selftest_eigen6")
    n = len(a)
    return ((out[:, :6], out[:, 6:42].reshape(n, 6, 6)), (out[:, 42:48], out[:, 48:].reshape(n, 6, 6)))


def selftest_gn_rows(cases):
    """The residual pass's per-query functions on the device (fbr_selftest_gn_rows): cases (n, 28)
    float32 = kind, 5 neighbours xyz, query xyz, scan point xyz, trig[6]; returns a dict of fit_ok
    (n,) bool, fit (n, 6), ok (n,) bool, coeff (n, 4), row (n, 6), b (n,)."""
    a = np.ascontiguousarray(cases, np.float32).reshape(-1, 28)
    out = np.zeros((len(a), 20), np.float32)
    _check(lib().fbr_selftest_gn_rows(len(a), ptr(a), ptr(out)), "fbr_selftest_gn_rows")
    return dict(fit_ok=out[:, 0] != 0, fit=out[:, 1:7].copy(), ok=out[:, 7] != 0, coeff=out[:, 8:12].copy(),
                row=out[:, 12:18].copy(), b=out[:, 18].copy())


def selftest_gn_reduce(rows, b, ok):
    """res_reduce on the device (fbr_selftest_gn_reduce): rows (s, 256, 6), b (s, 256), ok (s, 256)
    -> (s, 28) float64 sums (21 upper AtA products, 6 AtB, the count)."""
    rows = np.asarray(rows, np.float32).reshape(-1, 256, 6)
    packed = np.ascontiguousarray(np.concatenate([rows, np.asarray(b, np.float32).reshape(-1, 256, 1)], axis=2))
    okf = np.ascontiguousarray(np.asarray(ok).reshape(-1, 256) != 0, np.int8)
    assert len(okf) == len(packed)
    out = np.zeros((len(packed), 32), np.float64)
    _check(lib().fbr_selftest_gn_reduce(len(packed), ptr(packed), ptr(okf), ptr(out)), "fbr_selftest_gn_reduce")
    assert not out[:, 28:].any()
    return out[:, :28].copy()


def selftest_solve6(mats, rhs):
    """qr_solve6 and lu_inv6 on the device (fbr_selftest_solve6): mats (n, 6, 6), rhs (n, 6) ->
    (qr return codes (n,), x (n, 6), lu return codes (n,), inverses (n, 6, 6))."""
    a = np.ascontiguousarray(mats, np.float32).reshape(-1, 36)
    b = np.ascontiguousarray(rhs, np.float32).reshape(-1, 6)
    assert len(a) == len(b)
    x = np.zeros((len(a), 6), np.float32)
    inv = np.zeros((len(a), 36), np.float32)
    ret = np.zeros((len(a), 2), np.int32)
    _check(lib().fbr_selftest_solve6(len(a), ptr(a), ptr(b), ptr(x), ptr(inv), ptr(ret)), "fbr_selftest_solve6")
    return ret[:, 0].copy(), x, ret[:, 1].copy(), inv.reshape(-1, 6, 6)


def selftest_eig_certified(mats, thr=100.0):
    """1 where the device certifies every eigenvalue of a symmetric 6x6 float matrix above thr
    without the Jacobi (fbr_selftest_eig_certified: the iteration-0 degeneracy fast path)."""
    a = np.ascontiguousarray(mats, np.float32).reshape(-1, 36)
    out = np.zeros(len(a), np.int32)
    _check(lib().fbr_selftest_eig_certified(len(a), ptr(a), ctypes.c_float(thr), ptr(out)), "fbr_selftest_eig_certified")
    return out


def selftest_voxel_order(keys, lds=False):
    """Device emulation of the VoxelGrid index sort (fbr_selftest_voxel_order): the point order
    std::sort leaves (keys[i], i) in, i.e. the stable key sort of the partitioned sequence."""
    k = np.ascontiguousarray(keys, np.uint32)
    perm = np.zeros(len(k), np.uint32)
    _check(lib().fbr_selftest_voxel_order(len(k), ptr(k), int(lds), ptr(perm)), "fbr_selftest_voxel_order")
    return perm[np.argsort(k[perm], kind="stable")].astype(np.int64)


def selftest_radix_sort(keys, nbits, variant):
    """One of the VoxelGrid kernels' radix sorts on the device (fbr_selftest_radix_sort): (sorted
    keys, source index of every sorted position)."""
    k = np.ascontiguousarray(keys, np.uint32).copy()
    perm = np.zeros(len(k), np.uint32)
    _check(lib().fbr_selftest_radix_sort(len(k), int(nbits), int(variant), ptr(k), ptr(perm)), "fbr_selftest_radix_sort")
    return k, perm.astype(np.int64)


def stream_copy_bandwidth(device=0, nbytes=2 << 30, iters=20):
    """Achievable HBM GB/s of a device float4 copy (read + write), fbr_stream_copy_bandwidth."""
    g = ctypes.c_double()
    _check(lib().fbr_stream_copy_bandwidth(device, nbytes, iters, ctypes.byref(g)), "fbr_stream_copy_bandwidth")
    return g.value


def valu_peak(device=0, waves_per_simd=4, kind=0, iters=4096, reps=5):
    """(wave-level VALU G instr/s, ms per launch) of the fbr_valu_peak probe: kind 0 v_fma_f32,
    1 v_add_u32, 2 v_pk_fma_f32, 3 v_cmp_lt_u64, 4 v_cmp_lt_u32, waves_per_simd waves on every SIMD."""
    g, ms = ctypes.c_double(), ctypes.c_double()
    _check(lib().fbr_valu_peak(device, waves_per_simd, kind, iters, reps, ctypes.byref(g), ctypes.byref(ms)),
           "fbr_valu_peak")
    return g.value, ms.value


def affine_from_pose(pose):
    m = np.zeros(16, np.float32)
    lib().fbr_affine_from_pose(ptr(np.ascontiguousarray(pose, np.float32)), ptr(m))
    return m.reshape(4, 4)


def reg_info_variances(info, floor=None):
    """The between-factor variances of one REG_INFO record: max(var_tangent[k], floor[k]) in the order
    Context.pg_add_between_poses takes (fbr_reg_info_variances; floor None: no floor)."""
    rec = np.ascontiguousarray(np.asarray(info, REG_INFO).reshape(-1)[:1])
    fl = None if floor is None else np.ascontiguousarray(floor, np.float64).reshape(6)
    out = np.zeros(6, np.float64)
    _check(lib().fbr_reg_info_variances(ptr(rec), None if fl is None else ptr(fl), ptr(out)), "fbr_reg_info_variances")
    return out


def pose_from_affine(m):
    p = np.zeros(6, np.float32)
    lib().fbr_pose_from_affine(ptr(np.ascontiguousarray(m, np.float32).reshape(16)), ptr(p))
    return p


def pcd_read(path):
    """pcl::io::loadPCDFile<PointXYZI> (mapOptmization.h:247-248) -> POINT_XYZI array (host only)."""
    p = os.fsencode(path)
    n = _I64()
    _check(lib().fbr_pcd_read(p, None, 0, ctypes.byref(n)), f"fbr_pcd_read({path})")
    out = np.zeros(max(n.value, 1), POINT_XYZI)
    _check(lib().fbr_pcd_read(p, ptr(out), len(out), ctypes.byref(n)), f"fbr_pcd_read({path})")
    return out[:n.value].copy()


def pcd_write(path, points, binary=False):
    """pcl::io::savePCDFileASCII (mapOptmization.h:511-515), or DATA binary when `binary`."""
    pts = _as_points(points, POINT_XYZI)
    f = lib().fbr_pcd_write_binary if binary else lib().fbr_pcd_write_ascii
    _check(f(os.fsencode(path), ptr(pts) if len(pts) else None, len(pts)), f"fbr_pcd_write({path})")


def pcd_write_poses(path, keyposes):
    """savePCDFileASCII of cloudKeyPoses6D (transformations.pcd, mapOptmization.h:499): KEYPOSE records
    as x y z intensity roll pitch yaw time (host only)."""
    kp = _as_points(np.atleast_1d(keyposes), KEYPOSE)
    _check(lib().fbr_pcd_write_poses_ascii(os.fsencode(path), ptr(kp) if len(kp) else None, len(kp)),
           f"fbr_pcd_write_poses_ascii({path})")


def msg_to_points(msg):
    """cachePointCloud's fromROSMsg + checks (imageProjection.cpp:253-298) on the host.
    Returns (POINT_XYZIRT array, msg_flags)."""
    n, fl = _I64(), _I32()
    _check(lib().fbr_msg_to_points(ctypes.byref(msg.c), None, 0, ctypes.byref(n), ctypes.byref(fl)),
           "fbr_msg_to_points")
    out = np.zeros(max(n.value, 1), POINT_XYZIRT)
    _check(lib().fbr_msg_to_points(ctypes.byref(msg.c), ptr(out), len(out), ctypes.byref(n), ctypes.byref(fl)),
           "fbr_msg_to_points")
    return out[:n.value].copy(), fl.value


def points_to_msg(points):
    """pcl::toROSMsg of a PointXYZI cloud (publishCloud, utility.h:255-264) -> PointCloud2."""
    pts = _as_points(points, POINT_XYZI)
    data = np.zeros(32 * len(pts), np.uint8)
    _check(lib().fbr_points_to_msg_data(ptr(pts) if len(pts) else None, len(pts), ptr(data) if len(pts) else None),
           "fbr_points_to_msg_data")
    fields = [("x", 0, PF_FLOAT32, 1), ("y", 4, PF_FLOAT32, 1), ("z", 8, PF_FLOAT32, 1),
              ("intensity", 16, PF_FLOAT32, 1)]
    return PointCloud2(data.tobytes(), fields, width=len(pts), point_step=32)


def imu_convert(ext, samples):
    """imuConverter (utility.h:219-253) on each sample (IMU_SAMPLE array) with IMU_EXTRINSICS `ext`."""
    samples = _as_points(np.atleast_1d(samples), IMU_SAMPLE)
    ext = np.ascontiguousarray(ext)
    out = np.zeros_like(samples)
    for i in range(len(samples)):
        _check(lib().fbr_imu_convert(ptr(ext), ctypes.c_void_p(samples.ctypes.data + i * IMU_SAMPLE.itemsize),
                                     ctypes.c_void_p(out.ctypes.data + i * IMU_SAMPLE.itemsize)), "fbr_imu_convert")
    return out


def imu_deskew_info(queue, time_scan_cur, time_scan_next, previous=None):
    """deskewInfo + imuDeskewInfo (imageProjection.cpp:303-393) on a queue of converted samples.
    Returns (DESKEW_TABLE record, number of leading samples popped).  `previous` carries the
    imu*Init fields forward as the reference's cloudInfo member does."""
    queue = _as_points(np.atleast_1d(queue), IMU_SAMPLE)
    tab = np.zeros(1, DESKEW_TABLE) if previous is None else np.array(previous, DESKEW_TABLE).reshape(1).copy()
    n_pop = _I64()
    _check(lib().fbr_imu_deskew_info(ptr(queue) if len(queue) else None, len(queue), ctypes.c_double(time_scan_cur),
                                     ctypes.c_double(time_scan_next), ptr(tab), ctypes.byref(n_pop)),
           "fbr_imu_deskew_info")
    return tab[0], n_pop.value


def odom_deskew_info(queue, time_scan_cur, time_scan_next):
    """odomDeskewInfo (imageProjection.cpp:395-491) on a queue of ODOM_SAMPLE records in arrival
    order.  Returns (ODOM_INFO record, number of leading samples popped).  The record's motion has
    flags 0: set FBR_MOTION_* (and the time source) before Context.set_motion."""
    queue = _as_points(np.atleast_1d(queue), ODOM_SAMPLE)
    info = np.zeros(1, ODOM_INFO)
    n_pop = _I64()
    _check(lib().fbr_odom_deskew_info(ptr(queue) if len(queue) else None, len(queue), ctypes.c_double(time_scan_cur),
                                      ctypes.c_double(time_scan_next), ptr(info), ctypes.byref(n_pop)),
           "fbr_odom_deskew_info")
    return info[0], n_pop.value


def motion_from_poses(prev, cur, dt, scan_period, dt_next):
    """Constant velocity from two registered poses {roll, pitch, yaw, x, y, z} taken dt apart.
    Returns (MOTION record for a scan of scan_period, the guess dt_next after `cur`)."""
    prev = np.ascontiguousarray(prev, np.float32).reshape(6)
    cur = np.ascontiguousarray(cur, np.float32).reshape(6)
    m = np.zeros(1, MOTION)
    guess = np.zeros(6, np.float32)
    _check(lib().fbr_motion_from_poses(ptr(prev), ptr(cur), ctypes.c_double(dt), ctypes.c_double(scan_period),
                                       ctypes.c_double(dt_next), ptr(m), ptr(guess)), "fbr_motion_from_poses")
    return m[0], guess


def update_initial_guess(state, odom, table, have_keyframes, use_imu_heading, pose):
    """updateInitialGuess (mapOptmization.h:799-855).  state: a GUESS_STATE array of one record,
    updated in place (None starts one); odom: ODOM_INFO record or None; table: DESKEW_TABLE record
    or None.  Returns (pose, state)."""
    st = np.zeros(1, GUESS_STATE) if state is None else state
    if st.dtype != GUESS_STATE or st.shape != (1,):
        raise TypeError("state: a GUESS_STATE array of one record")
    od = None if odom is None else np.array(odom, ODOM_INFO).reshape(1)
    tb = None if table is None else np.array(table, DESKEW_TABLE).reshape(1)
    p = np.array(pose, np.float32).reshape(6).copy()
    _check(lib().fbr_update_initial_guess(ptr(st), None if od is None else ptr(od), None if tb is None else ptr(tb),
                                          int(bool(have_keyframes)), int(bool(use_imu_heading)), ptr(p)),
           "fbr_update_initial_guess")
    return p, st


def _as_points(a, dtype):
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        raise TypeError(f"expected dtype {dtype}, got {a.dtype}")
    return a


class Context:
    """One fbr_ctx: a HIP device, a stream, HBM buffers for `max_batch` scans."""

    def __init__(self, params=None, device=0, **kw):
        self.params = params if params is not None else default_params(**kw)
        self._h = ctypes.c_void_p()
        _check(lib().fbr_create(ctypes.byref(self._h), ctypes.byref(self.params), device), "fbr_create")

    def close(self):
        if self._h:
            lib().fbr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- map (mapOptmization.h:245-260) ----
    def set_map(self, corner, surf):
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        _check(lib().fbr_set_map(self._h, ptr(corner), len(corner), ptr(surf), len(surf)), "fbr_set_map")

    def load_map(self, corner_pcd, surf_pcd):
        """loadPCDFile(cloudCorner.pcd / cloudSurf.pcd) + the start-up DS (mapOptmization.h:245-260)."""
        _check(lib().fbr_load_map(self._h, os.fsencode(corner_pcd), os.fsencode(surf_pcd)), "fbr_load_map")

    def get_map(self):
        nc, ns = _I64(), _I64()
        _check(lib().fbr_get_map(self._h, ctypes.byref(nc), ctypes.byref(ns), None, None), "fbr_get_map")
        c = np.zeros(max(nc.value, 1), POINT_XYZI)
        s = np.zeros(max(ns.value, 1), POINT_XYZI)
        _check(lib().fbr_get_map(self._h, None, None, ptr(c), ptr(s)), "fbr_get_map")
        return c[:nc.value].copy(), s[:ns.value].copy()

    # ---- A2+A4 ----
    def project(self, pts):
        pts = _as_points(pts, POINT_XYZIRT)
        n_in, H = len(pts), self.params.n_scan
        start = np.zeros(H, np.int32)
        end = np.zeros(H, np.int32)
        cap = max(n_in, 1)
        col = np.zeros(cap, np.int32)
        rng = np.zeros(cap, np.float32)
        cloud = np.zeros(cap, POINT_XYZI)
        n = _I64()
        _check(lib().fbr_project(self._h, ptr(pts), n_in, ptr(start), ptr(end), ptr(col), ptr(rng),
                                 ptr(cloud), ctypes.byref(n)), "fbr_project")
        k = n.value
        return dict(start_ring=start, end_ring=end, col_ind=col[:k].copy(), range=rng[:k].copy(),
                    cloud=cloud[:k].copy())

    # ---- A6-A9 ----
    def extract_features(self, n_points):
        H, W = self.params.n_scan, self.params.horizon_scan
        label = np.zeros(max(n_points, 1), np.int8)
        corner = np.zeros(120 * H, POINT_XYZI)
        surf = np.zeros(max(H * W, 1), POINT_XYZI)
        nc, ns = _I64(), _I64()
        _check(lib().fbr_extract_features(self._h, ptr(label), ptr(corner), ctypes.byref(nc), ptr(surf),
                                          ctypes.byref(ns)), "fbr_extract_features")
        return dict(label=label[:n_points].copy(), corner=corner[:nc.value].copy(),
                    surf=surf[:ns.value].copy())

    def features(self, pts):
        pr = self.project(pts)
        f = self.extract_features(len(pr["col_ind"]))
        f["n_points"] = len(pr["col_ind"])
        return f

    # ---- A10-A18 ----
    def register(self, corner, surf, pose, trace=False):
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        pose = np.ascontiguousarray(pose, dtype=np.float32).copy()
        st = FbrRegStats()
        if trace:
            tr = np.zeros((self.params.max_iterations, 6), np.float32)
            _check(lib().fbr_register_trace(self._h, ptr(corner), len(corner), ptr(surf), len(surf),
                                            ptr(pose), ctypes.byref(st), ptr(tr)), "fbr_register_trace")
            d = st.as_dict()
            return pose, d, tr[:d["iterations"]].copy()
        _check(lib().fbr_register(self._h, ptr(corner), len(corner), ptr(surf), len(surf), ptr(pose),
                                  ctypes.byref(st)), "fbr_register")
        return pose, st.as_dict()

    def process_scan(self, pts, stamp, pose):
        pts = _as_points(pts, POINT_XYZIRT)
        pose = np.ascontiguousarray(pose, dtype=np.float32).copy()
        st = FbrRegStats()
        _check(lib().fbr_process_scan(self._h, ptr(pts), len(pts), ctypes.c_double(stamp), ptr(pose),
                                      ctypes.byref(st)), "fbr_process_scan")
        return pose, st.as_dict()

    def project_msg(self, msg):
        """project() from a raw PointCloud2 (unpacked on the device); also returns msg_flags."""
        H = self.params.n_scan
        cap = max(msg.c.width * msg.c.height, 1)
        start, end = np.zeros(H, np.int32), np.zeros(H, np.int32)
        col, rng, cloud = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, POINT_XYZI)
        n, fl = _I64(), _I32()
        _check(lib().fbr_project_msg(self._h, ctypes.byref(msg.c), ptr(start), ptr(end), ptr(col), ptr(rng),
                                     ptr(cloud), ctypes.byref(n), ctypes.byref(fl)), "fbr_project_msg")
        k = n.value
        return dict(start_ring=start, end_ring=end, col_ind=col[:k].copy(), range=rng[:k].copy(),
                    cloud=cloud[:k].copy(), msg_flags=fl.value)

    def process_msg(self, msg, stamp, pose):
        pose = np.ascontiguousarray(pose, dtype=np.float32).copy()
        st, fl = FbrRegStats(), _I32()
        _check(lib().fbr_process_msg(self._h, ctypes.byref(msg.c), ctypes.c_double(stamp), ptr(pose),
                                     ctypes.byref(st), ctypes.byref(fl)), "fbr_process_msg")
        return pose, st.as_dict(), fl.value

    def set_motion(self, motions):
        """Motion records (MOTION) for the following calls: job j of a batch uses motions[j], the
        single-scan calls motions[0]; None turns the motion deskew off."""
        if motions is None:
            _check(lib().fbr_set_motion(self._h, None, 0), "fbr_set_motion")
            return
        m = np.ascontiguousarray(np.array(motions, MOTION).reshape(-1))
        _check(lib().fbr_set_motion(self._h, ptr(m), len(m)), "fbr_set_motion")

    def set_deskew(self, tables):
        """IMU deskew tables (DESKEW_TABLE records) for the following calls: job j of a batch uses
        tables[j], single-scan calls tables[0]; None restores the reference's runtime path."""
        if tables is None:
            _check(lib().fbr_set_deskew(self._h, None, 0), "fbr_set_deskew")
            return
        t = np.ascontiguousarray(np.array(tables, DESKEW_TABLE).reshape(-1))
        _check(lib().fbr_set_deskew(self._h, ptr(t), len(t)), "fbr_set_deskew")

    # ---- LIO-SAM keyframe local map (mapOptmization.h:857-978) ----
    def keyframes_add(self, pose, corner, surf):
        """cloudKeyPoses3D/6D + corner/surfCloudKeyFrames push_back (pose: KEYPOSE record)."""
        p = np.array(pose, KEYPOSE).reshape(1)
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        _check(lib().fbr_keyframes_add(self._h, ptr(p), ptr(corner) if len(corner) else None, len(corner),
                                       ptr(surf) if len(surf) else None, len(surf)), "fbr_keyframes_add")

    def keyframes_set_pose(self, index, pose):
        p = np.array(pose, KEYPOSE).reshape(1)
        _check(lib().fbr_keyframes_set_pose(self._h, index, ptr(p)), "fbr_keyframes_set_pose")

    def keyframes_count(self):
        n = _I64()
        _check(lib().fbr_keyframes_count(self._h, ctypes.byref(n)), "fbr_keyframes_count")
        return n.value

    def keyframes_reset(self):
        _check(lib().fbr_keyframes_reset(self._h), "fbr_keyframes_reset")

    def extract_surrounding_keyframes(self, stamp, kparams):
        """extractSurroundingKeyFrames: the local map becomes the registration map (no CropBox).
        Returns (n_corner_map, n_surf_map, n_frames)."""
        nc, ns, nf = _I64(), _I64(), ctypes.c_int32()
        _check(lib().fbr_extract_surrounding_keyframes(self._h, ctypes.c_double(stamp), ctypes.byref(kparams),
                                                       ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(nf)),
               "fbr_extract_surrounding_keyframes")
        return nc.value, ns.value, nf.value

    # ---- loop closure (mapOptmization.h:606-782) ----
    def detect_loop_closure(self, stamp, lparams=None):
        """detectLoopClosure at timeLaserCloudInfoLast = stamp: (latest_id, closest_id), or None when
        there is no candidate."""
        lp = lparams if lparams is not None else loop_params()
        a, b = _I32(), _I32()
        _check(lib().fbr_detect_loop_closure(self._h, ctypes.c_double(stamp), ctypes.byref(lp), ctypes.byref(a),
                                             ctypes.byref(b)), "fbr_detect_loop_closure")
        return None if a.value < 0 else (a.value, b.value)

    def perform_loop_closure(self, stamp, lparams=None, raw=False):
        """performLoopClosure up to the between-factor: the fbr_loop_result as a dict (raw: the
        FbrLoopResult structure itself)."""
        lp = lparams if lparams is not None else loop_params()
        r = FbrLoopResult()
        _check(lib().fbr_perform_loop_closure(self._h, ctypes.c_double(stamp), ctypes.byref(lp), ctypes.byref(r)),
               "fbr_perform_loop_closure")
        return r if raw else r.as_dict()

    def icp_align(self, source, target, iparams=None, raw=False):
        """The loop closure's ICP on two host clouds: the fbr_icp_result as a dict."""
        ip = iparams if iparams is not None else icp_params()
        source = _as_points(source, POINT_XYZI)
        target = _as_points(target, POINT_XYZI)
        r = FbrIcpResult()
        _check(lib().fbr_icp_align(self._h, ptr(source) if len(source) else None, len(source),
                                   ptr(target) if len(target) else None, len(target), ctypes.byref(ip),
                                   ctypes.byref(r)), "fbr_icp_align")
        return r if raw else r.as_dict()

    # ---- loop closure for many keyframe pairs ----
    def loop_candidates(self, lparams=None, first=0):
        """detectLoopClosure's rule for every keyframe >= first as it stood when that keyframe was the
        last one: a list of (latest_id, closest_id), at most one per keyframe, ascending."""
        lp = lparams if lparams is not None else loop_params()
        n = _I64()
        rc = lib().fbr_loop_candidates(self._h, ctypes.byref(lp), first, None, 0, ctypes.byref(n))
        if rc != -4:  # FBR_ERR_CAPACITY: the size query's answer when there are pairs
            _check(rc, "fbr_loop_candidates")
        if n.value == 0:
            return []
        pairs = (FbrLoopPair * n.value)()
        _check(lib().fbr_loop_candidates(self._h, ctypes.byref(lp), first, pairs, n.value, ctypes.byref(n)),
               "fbr_loop_candidates")
        return [(p.latest_id, p.closest_id) for p in pairs[:n.value]]

    def perform_loop_closures(self, pairs, lparams=None, chunk=0, raw=False):
        """performLoopClosure for each pair, the ICPs of a chunk in the same launches.  A pair is
        (latest_id, closest_id), (latest_id, closest_id, pose_guess) or an FbrLoopPair.  Returns one
        fbr_loop_result per pair (dicts; raw: FbrLoopResult structures, which pg_add_loop takes)."""
        lp = lparams if lparams is not None else loop_params()
        n = len(pairs)
        arr = (FbrLoopPair * max(n, 1))()
        for k, p in enumerate(pairs):
            if isinstance(p, FbrLoopPair):
                ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(p), ctypes.sizeof(FbrLoopPair))
                continue
            arr[k].latest_id, arr[k].closest_id = int(p[0]), int(p[1])
            if len(p) > 2 and p[2] is not None:
                arr[k].use_guess = 1
                arr[k].pose_guess[:] = [float(v) for v in np.asarray(p[2], np.float32)]
        out = (FbrLoopResult * max(n, 1))()
        _check(lib().fbr_perform_loop_closures(self._h, ctypes.byref(lp), arr, n, chunk, out), "fbr_perform_loop_closures")
        res = []
        for k in range(n):  # copies: an element of `out` would keep the whole array alive
            r = FbrLoopResult()
            ctypes.memmove(ctypes.byref(r), ctypes.byref(out[k]), ctypes.sizeof(FbrLoopResult))
            res.append(r if raw else r.as_dict())
        return res

    def icp_align_batch(self, sources, targets, iparams=None, chunk=0, raw=False):
        """icp_align per (source, target) pair of host clouds, the ICPs of a chunk in the same launches."""
        ip = iparams if iparams is not None else icp_params()
        assert len(sources) == len(targets)
        n = len(sources)
        src = [_as_points(s, POINT_XYZI) for s in sources]
        tgt = [_as_points(t, POINT_XYZI) for t in targets]
        sp = (_VP * max(n, 1))(*[s.ctypes.data if len(s) else None for s in src])
        tp = (_VP * max(n, 1))(*[t.ctypes.data if len(t) else None for t in tgt])
        sn = (_I64 * max(n, 1))(*[len(s) for s in src])
        tn = (_I64 * max(n, 1))(*[len(t) for t in tgt])
        out = (FbrIcpResult * max(n, 1))()
        _check(lib().fbr_icp_align_batch(self._h, sp, sn, tp, tn, n, ctypes.byref(ip), chunk, out), "fbr_icp_align_batch")
        res = []
        for k in range(n):
            r = FbrIcpResult()
            ctypes.memmove(ctypes.byref(r), ctypes.byref(out[k]), ctypes.sizeof(FbrIcpResult))
            res.append(r if raw else r.as_dict())
        return res

    def selftest_nn1(self, target, query, max_distance):
        """The ICP correspondence search alone: (index int32 [n_query], -1 = none; d2 float32)."""
        target = _as_points(target, POINT_XYZI)
        query = _as_points(query, POINT_XYZI)
        idx = np.zeros(max(len(query), 1), np.int32)
        d2 = np.zeros(max(len(query), 1), np.float32)
        _check(lib().fbr_selftest_nn1(self._h, ptr(target) if len(target) else None, len(target),
                                      ptr(query) if len(query) else None, len(query), ctypes.c_float(max_distance),
                                      ptr(idx), ptr(d2)), "fbr_selftest_nn1")
        return idx[:len(query)].copy(), d2[:len(query)].copy()

    # ---- place recognition (include/fbr.h "place recognition") ----
    def sc_describe(self, corner, surf, sc=None):
        """The scan-context descriptor of a lidar-frame cloud (corner then surf): float32 [n_ring, n_sector]."""
        sp = sc if sc is not None else sc_params()
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        out = np.zeros((sp.n_ring, sp.n_sector), np.float32)
        _check(lib().fbr_sc_describe(self._h, ctypes.byref(sp), ptr(corner) if len(corner) else None, len(corner),
                                     ptr(surf) if len(surf) else None, len(surf), ptr(out)), "fbr_sc_describe")
        return out

    def sc_update(self, sc=None):
        """Describe the keyframes added since the last call; returns how many."""
        sp = sc if sc is not None else sc_params()
        n = _I64()
        _check(lib().fbr_sc_update(self._h, ctypes.byref(sp), ctypes.byref(n)), "fbr_sc_update")
        return n.value

    def sc_descriptor(self, keyframe, sc=None):
        """The stored descriptor of one keyframe (`sc`: the shape the store was described with)."""
        sp = sc if sc is not None else sc_params()
        out = np.zeros((sp.n_ring, sp.n_sector), np.float32)
        _check(lib().fbr_sc_descriptor(self._h, int(keyframe), ptr(out)), "fbr_sc_descriptor")
        return out

    def sc_query(self, corner, surf, k=4, sc=None, raw=False):
        """The min(k, keyframes) best matches of a lidar-frame cloud in rank order, as dicts (raw: the
        FbrScMatch array and its length)."""
        sp = sc if sc is not None else sc_params()
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        out = (FbrScMatch * max(int(k), 1))()
        n = ctypes.c_int()
        _check(lib().fbr_sc_query(self._h, ctypes.byref(sp), ptr(corner) if len(corner) else None, len(corner),
                                  ptr(surf) if len(surf) else None, len(surf), int(k), out, ctypes.byref(n)),
               "fbr_sc_query")
        return (out, n.value) if raw else [out[i].as_dict() for i in range(n.value)]

    def sc_detect_loop_closure(self, stamp, lparams=None, sc=None):
        """detectLoopClosure by appearance: ((latest_id, closest_id) or None, the best candidate's match
        as a dict or None when there was no candidate at all)."""
        lp = lparams if lparams is not None else loop_params()
        sp = sc if sc is not None else sc_params()
        a, b, m = _I32(), _I32(), FbrScMatch()
        _check(lib().fbr_sc_detect_loop_closure(self._h, ctypes.c_double(stamp), ctypes.byref(lp), ctypes.byref(sp),
                                                ctypes.byref(a), ctypes.byref(b), ctypes.byref(m)),
               "fbr_sc_detect_loop_closure")
        return (None if a.value < 0 else (a.value, b.value)), (None if m.keyframe < 0 else m.as_dict())

    def perform_loop_closure_sc(self, stamp, lparams=None, sc=None, raw=False):
        """perform_loop_closure with the candidate and the last keyframe's pose taken from the scan-context
        match: (fbr_loop_result, match), dicts unless raw."""
        lp = lparams if lparams is not None else loop_params()
        sp = sc if sc is not None else sc_params()
        r, m = FbrLoopResult(), FbrScMatch()
        _check(lib().fbr_perform_loop_closure_sc(self._h, ctypes.c_double(stamp), ctypes.byref(lp), ctypes.byref(sp),
                                                 ctypes.byref(r), ctypes.byref(m)), "fbr_perform_loop_closure_sc")
        return (r, m) if raw else (r.as_dict(), None if m.keyframe < 0 else m.as_dict())

    # ---- pose graph (include/fbr.h "pose graph") ----
    def pg_reset(self):
        _check(lib().fbr_pg_reset(self._h), "fbr_pg_reset")

    def pg_add_prior(self, node, pose, variances):
        """PriorFactor<Pose3> on keyframe `node`: pose [roll, pitch, yaw, x, y, z], variances [6] in
        the same order."""
        p, v = np.ascontiguousarray(pose, np.float32), np.ascontiguousarray(variances, np.float64)
        assert p.shape == (6,) and v.shape == (6,)
        _check(lib().fbr_pg_add_prior(self._h, int(node), ptr(p), ptr(v)), "fbr_pg_add_prior")

    def pg_add_between(self, i, j, between, variances):
        """BetweenFactor<Pose3>(i, j) with the measured T_i^-1 T_j as a row-major 4x4 float matrix."""
        m, v = np.ascontiguousarray(between, np.float32).reshape(16), np.ascontiguousarray(variances, np.float64)
        assert v.shape == (6,)
        _check(lib().fbr_pg_add_between(self._h, int(i), int(j), ptr(m), ptr(v)), "fbr_pg_add_between")

    def pg_add_between_poses(self, i, j, pose_i, pose_j, variances):
        """BetweenFactor<Pose3>(i, j, pose_i.between(pose_j)): how odometry is added (:1533-1537)."""
        a, b = np.ascontiguousarray(pose_i, np.float32), np.ascontiguousarray(pose_j, np.float32)
        v = np.ascontiguousarray(variances, np.float64)
        assert a.shape == (6,) and b.shape == (6,) and v.shape == (6,)
        _check(lib().fbr_pg_add_between_poses(self._h, int(i), int(j), ptr(a), ptr(b), ptr(v)), "fbr_pg_add_between_poses")

    def pg_add_gps(self, node, xyz, variances):
        p, v = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(variances, np.float64)
        assert p.shape == (3,) and v.shape == (3,)
        _check(lib().fbr_pg_add_gps(self._h, int(node), ptr(p), ptr(v)), "fbr_pg_add_gps")

    def pg_add_loop(self, loop_result):
        """The between factor of a closed loop (perform_loop_closure(..., raw=True)'s FbrLoopResult);
        returns whether one was added (status FBR_LOOP_CLOSED)."""
        added = ctypes.c_int()
        _check(lib().fbr_pg_add_loop(self._h, ctypes.byref(loop_result), ctypes.byref(added)), "fbr_pg_add_loop")
        return bool(added.value)

    def pg_factor_count(self):
        n = _I64()
        _check(lib().fbr_pg_factor_count(self._h, ctypes.byref(n)), "fbr_pg_factor_count")
        return n.value

    def pg_poses(self):
        """The last optimise's poses: float64 [N, 6] = [roll, pitch, yaw, x, y, z]."""
        n = _I64()
        rc = lib().fbr_pg_poses(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, -4):  # FBR_ERR_CAPACITY: the count is in n
            _check(rc, "fbr_pg_poses")
        out = np.zeros((max(n.value, 1), 6), np.float64)
        _check(lib().fbr_pg_poses(self._h, ptr(out), len(out), ctypes.byref(n)), "fbr_pg_poses")
        return out[:n.value]

    def pg_optimize(self, params=None, raw=False):
        """Optimise the key poses under the factors: (poses float64 [N, 6], fbr_pg_result as a dict;
        raw: the FbrPgResult itself).  No key pose changes until pg_apply."""
        p = params if params is not None else pg_params()
        r = FbrPgResult()
        _check(lib().fbr_pg_optimize(self._h, ctypes.byref(p), ctypes.byref(r)), "fbr_pg_optimize")
        poses = self.pg_poses() if r.n_nodes > 0 else np.zeros((0, 6), np.float64)
        return poses, (r if raw else r.as_dict())

    def pg_loop_weights(self):
        """Every loop factor in add order at the last optimise's poses: (index in the factor list int32
        [K], chi2 = |r|^2 of the whitened residual float64 [K], robust weight float64 [K]; the weights
        are 1 without a robust option)."""
        n = _I64()
        rc = lib().fbr_pg_loop_weights(self._h, None, None, None, 0, ctypes.byref(n))
        if rc not in (0, -4):  # FBR_ERR_CAPACITY: the count is in n
            _check(rc, "fbr_pg_loop_weights")
        k = max(n.value, 1)
        idx, chi2, w = np.zeros(k, np.int32), np.zeros(k, np.float64), np.zeros(k, np.float64)
        _check(lib().fbr_pg_loop_weights(self._h, ptr(idx), ptr(chi2), ptr(w), k, ctypes.byref(n)), "fbr_pg_loop_weights")
        return idx[:n.value], chi2[:n.value], w[:n.value]

    def pg_apply(self):
        """correctPoses: the optimised poses, rounded to float, become the key poses."""
        _check(lib().fbr_pg_apply(self._h), "fbr_pg_apply")

    def pg_marginals(self, nodes=None, raw=False, **params):
        """Marginal covariances of key poses at the last optimise's poses: (cov float64 [n, 6, 6] in
        tangent order [rotation; translation], fbr_pg_marginal_result as a dict; raw: the struct).
        nodes: the node indices (None: every node in order); params: fbr_pg_marginal_params' fields
        (rhs_chunk, max_work_bytes).  With status FBR_PG_NUMERICAL the covariances are zero."""
        p = pg_marginal_params(**params)
        r = FbrPgMarginalResult()
        idx = None if nodes is None else np.ascontiguousarray(nodes, np.int64).reshape(-1)
        if idx is None:  # the row count first, as pg_poses
            rc = lib().fbr_pg_marginals(self._h, ctypes.byref(p), None, 0, None, 0, ctypes.byref(r))
            if rc not in (0, -4) or (rc == -4 and r.n_out == 0):
                _check(rc, "fbr_pg_marginals")
            rows = r.n_out
        else:
            rows = len(idx)
        cov = np.zeros((max(rows, 1), 6, 6), np.float64)
        _check(lib().fbr_pg_marginals(self._h, ctypes.byref(p), None if idx is None else ptr(idx), rows, ptr(cov), len(cov),
                                      ctypes.byref(r)), "fbr_pg_marginals")
        return cov[:rows], (r if raw else r.as_dict())

    def pg_gps_gate(self, threshold=25.0):
        """addGPSFactor's covariance gate (mapOptmization.h:1561) on the last key pose: (wanted,
        [cov_xx, cov_yy]); threshold = poseCovThreshold."""
        wanted, xy = ctypes.c_int(0), np.zeros(2, np.float64)
        _check(lib().fbr_pg_gps_gate(self._h, float(threshold), ctypes.byref(wanted), ptr(xy)), "fbr_pg_gps_gate")
        return bool(wanted.value), xy

    # ---- global map (mapOptmization.h:485-521) ----
    def global_map_build(self, params=None, raw=False, **kw):
        """Build the global map from every keyframe at its current key pose (params: gmap_params(), or
        its fields as keywords).  Returns fbr_gmap_result as a dict (raw: the FbrGmapResult itself)."""
        p = params if params is not None else gmap_params(**kw)
        r = FbrGmapResult()
        _check(lib().fbr_global_map_build(self._h, ctypes.byref(p), ctypes.byref(r)), "fbr_global_map_build")
        return r if raw else r.as_dict()

    def global_map(self):
        """The built (corner, surf) clouds."""
        nc, ns = _I64(), _I64()
        _check(lib().fbr_global_map_get(self._h, ctypes.byref(nc), ctypes.byref(ns), None, None), "fbr_global_map_get")
        c = np.zeros(max(nc.value, 1), POINT_XYZI)
        s = np.zeros(max(ns.value, 1), POINT_XYZI)
        _check(lib().fbr_global_map_get(self._h, None, None, ptr(c), ptr(s)), "fbr_global_map_get")
        return c[:nc.value].copy(), s[:ns.value].copy()

    def global_map_install(self):
        """What set_map(*global_map()) does, without the clouds leaving the device."""
        _check(lib().fbr_global_map_install(self._h), "fbr_global_map_install")

    def global_map_save(self, directory, cloud_global=False):
        """cloudCorner.pcd, cloudSurf.pcd, trajectory.pcd, transformations.pcd (and cloudGlobal.pcd when
        asked for and the build kept the raw clouds) into the existing `directory`."""
        _check(lib().fbr_global_map_save(self._h, os.fsencode(directory), 1 if cloud_global else 0),
               "fbr_global_map_save")

    def selftest_voxel_wide(self, pts, leaf):
        """The wide (64-bit key) VoxelGrid alone on a host cloud, overflowing or not."""
        pts = _as_points(pts, POINT_XYZI)
        out = np.zeros(max(len(pts), 1), POINT_XYZI)
        n = _I64()
        _check(lib().fbr_selftest_voxel_wide(self._h, ptr(pts) if len(pts) else None, len(pts), ctypes.c_float(leaf),
                                             ptr(out), ctypes.byref(n)), "fbr_selftest_voxel_wide")
        return out[:n.value].copy()

    def relocalize(self, points, k=4, sc=None):
        """Find the pose of one raw scan (POINT_XYZIRT) without a guess: project, extract features,
        down-sample them at the two mapping leaves, sc_query, then register from each hypothesis in
        rank order against the installed registration map (set_map / load_map; the keyframes serve only
        as the place database).  Returns (hypotheses, winner): hypotheses = [(match, pose, stats)] and
        winner = the index of the converged, non-degenerate result with the largest n_sel (the first
        of equals), or -1."""
        f = self.features(points)
        corner = self.voxel_grid(f["corner"], self.params.mapping_corner_leaf_size)
        surf = self.voxel_grid(f["surf"], self.params.mapping_surf_leaf_size)
        hyps, winner = [], -1
        for m in self.sc_query(corner, surf, k, sc):
            pose, st = self.register(f["corner"], f["surf"], m["pose_guess"])
            hyps.append((m, pose, st))
            if st["status"] == 0 and st["converged"] and not st["degenerate"] and (
                    winner < 0 or st["n_sel"] > hyps[winner][2]["n_sel"]):
                winner = len(hyps) - 1
        return hyps, winner

    # ---- pose scoring (include/fbr.h "pose scoring") ----
    def score_poses(self, corner, surf, poses, score=None, keys=False):
        """How well a scan-frame cloud (corner, surf: the mapping-leaf down-samples) fits the installed
        map at each pose [roll, pitch, yaw, x, y, z]: a POSE_SCORE record array [n_poses]; with keys,
        also the correspondence keys uint64 [n_poses, n_corner + n_surf] (~0: no inlier)."""
        sp = score if score is not None else score_params()
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        out = np.zeros(max(len(poses), 1), POSE_SCORE)
        nn = np.zeros((max(len(poses), 1), max(len(corner) + len(surf), 1)), np.uint64) if keys else None
        _check(lib().fbr_score_poses(self._h, ctypes.byref(sp), ptr(corner) if len(corner) else None, len(corner),
                                     ptr(surf) if len(surf) else None, len(surf), ptr(poses) if len(poses) else None,
                                     len(poses), ptr(out), None if nn is None else ptr(nn)), "fbr_score_poses")
        out = out[:len(poses)]
        return (out, nn[:len(poses), :len(corner) + len(surf)]) if keys else out

    def pose_search(self, corner, surf, seeds, lattice, top_k=3, score=None):
        """Score the lattice of hypotheses around the seed poses [n_seeds, 6] and return the top_k best
        by (fitness, hypothesis index): (poses float32 [m, 6], POSE_SCORE [m], hypothesis indices int64 [m])."""
        sp = score if score is not None else score_params()
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        seeds = np.ascontiguousarray(seeds, np.float32).reshape(-1, 6)
        k = max(int(top_k), 0)
        poses = np.zeros((max(k, 1), 6), np.float32)
        sc = np.zeros(max(k, 1), POSE_SCORE)
        idx = np.zeros(max(k, 1), np.int64)
        n = _I64()
        _check(lib().fbr_pose_search(self._h, ctypes.byref(sp), ptr(corner) if len(corner) else None, len(corner),
                                     ptr(surf) if len(surf) else None, len(surf), ptr(seeds) if len(seeds) else None,
                                     len(seeds), ctypes.byref(lattice), int(top_k), ptr(poses), ptr(sc), ptr(idx),
                                     ctypes.byref(n)), "fbr_pose_search")
        return poses[:n.value].copy(), sc[:n.value].copy(), idx[:n.value].copy()

    # ---- registration information (include/fbr.h "registration information") ----
    def reg_info(self, corner, surf, poses, **params):
        """How well the map determines each pose [roll, pitch, yaw, x, y, z] of a scan-frame cloud
        (corner, surf: the mapping-leaf down-samples): a REG_INFO record array [n_poses] with the
        Gauss-Newton normal matrix H at the pose, its spectrum (eig, evec, rank) and the covariance in
        the pose's own increments (cov) and in the pose graph's chart (cov_tangent, var_tangent).
        params: the fields of fbr_info_params (eig_floor, unobserved_variance, sigma2, pose_chunk)."""
        ip = info_params(**params)
        corner = _as_points(corner, POINT_XYZI)
        surf = _as_points(surf, POINT_XYZI)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        out = np.zeros(max(len(poses), 1), REG_INFO)
        _check(lib().fbr_reg_info_poses(self._h, ctypes.byref(ip), ptr(corner) if len(corner) else None, len(corner),
                                        ptr(surf) if len(surf) else None, len(surf), ptr(poses) if len(poses) else None,
                                        len(poses), ptr(out)), "fbr_reg_info_poses")
        return out[:len(poses)]

    def batch_info(self, **params):
        """The REG_INFO record of every job of the latest batch launch, at the job's result pose over
        the launch's down-sampled clouds; a job that did not register has flags FBR_INFO_NOT_REGISTERED."""
        ip = info_params(**params)
        # the library writes one record per job of the launched batch and takes no capacity: room for
        # the context's max_batch, whatever this object believes was staged
        n = getattr(self, "_staged", None)
        if n is None:
            raise FbrError(-7, "batch_info: no batch was staged or processed through this object")
        out = np.zeros(max(int(self.params.max_batch), n, 1), REG_INFO)
        _check(lib().fbr_batch_info(self._h, ctypes.byref(ip), ptr(out)), "fbr_batch_info")
        return out[:n].copy()

    def relocalize_search(self, points, seeds=None, k=4, sc=None, lattice=None, top=3, score=None):
        """Find the pose of one raw scan (POINT_XYZIRT) from coarse seeds: project, extract features,
        down-sample them at the two mapping leaves, take the seed poses from the argument ([n, 6]) or
        from sc_query's k hypotheses (seeds None), pose_search the lattice around them (default: x, y
        +-3 m in 0.5 m steps, yaw +-0.8 rad in 0.1 rad steps), register from each of the `top` best
        poses and score every registered pose again.  Returns (hypotheses, winner): hypotheses =
        [(searched pose, pose, stats, score)], score the POSE_SCORE record of the registered pose, and
        winner = the index of the converged, non-degenerate result with the smallest fitness (the
        first of equals), or -1."""
        f = self.features(points)
        corner = self.voxel_grid(f["corner"], self.params.mapping_corner_leaf_size)
        surf = self.voxel_grid(f["surf"], self.params.mapping_surf_leaf_size)
        if seeds is None:
            seeds = [m["pose_guess"] for m in self.sc_query(corner, surf, k, sc)]
        seeds = np.asarray(seeds, np.float32).reshape(-1, 6)
        lat = lattice if lattice is not None else pose_lattice((3.0, 3.0, 0.0, 0.8), (0.5, 0.5, 0.0, 0.1))
        found, _, _ = self.pose_search(corner, surf, seeds, lat, top, score)
        hyps, winner = [], -1
        for start in found:
            pose, st = self.register(f["corner"], f["surf"], start)
            hyps.append((start, pose, st))
        scores = self.score_poses(corner, surf, [h[1] for h in hyps], score) if hyps else []
        hyps = [h + (s,) for h, s in zip(hyps, scores)]
        for i, (_, _, st, s) in enumerate(hyps):
            if st["status"] == 0 and st["converged"] and not st["degenerate"] and (
                    winner < 0 or s["fitness"] < hyps[winner][3]["fitness"]):
                winner = i
        return hyps, winner

    @property
    def stream_handle(self):
        """The context's primary hipStream_t (int address): batch results and exports are ordered on it."""
        return lib().fbr_stream(self._h) or 0

    def reset_stream(self):
        _check(lib().fbr_reset_stream(self._h), "fbr_reset_stream")

    # ---- batches of independent jobs ----
    def _scan_ptrs(self, scans):
        scans = [_as_points(s, POINT_XYZIRT) for s in scans]
        arr = (ctypes.c_void_p * len(scans))(*[s.ctypes.data for s in scans])
        n_in = np.array([len(s) for s in scans], np.int64)
        return scans, arr, n_in

    def process_batch(self, scans, guesses):
        keep, arr, n_in = self._scan_ptrs(scans)
        poses = np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(-1, 6)).copy()
        stats = np.zeros(len(keep), REG_STATS)
        _check(lib().fbr_process_batch(self._h, arr, ptr(n_in), len(keep), ptr(poses), ptr(stats)),
               "fbr_process_batch")
        # fbr_process_batch runs max_batch jobs at a time and leaves the last of those batches staged
        mb = max(int(self.params.max_batch), 1)
        self._staged = len(keep) - ((len(keep) - 1) // mb) * mb if len(keep) else 0
        return poses, stats

    def map_grid_info(self):
        """The map's kNN grid: dict(sparse, dims, box_cells, stored, n_corner, n_surf)."""
        v = np.zeros(8, np.int64)
        _check(lib().fbr_map_grid_info(self._h, ptr(v)), "fbr_map_grid_info")
        return dict(sparse=bool(v[0]), dims=tuple(int(x) for x in v[1:4]), box_cells=int(v[4]), stored=int(v[5]),
                    n_corner=int(v[6]), n_surf=int(v[7]))

    def ingest_bytes(self):
        """Host-to-device scan bytes of the last process_batch."""
        v = ctypes.c_double()
        _check(lib().fbr_ingest_bytes(self._h, ctypes.byref(v)), "fbr_ingest_bytes")
        return v.value

    def batch_stage(self, scans, guesses):
        keep, arr, n_in = self._scan_ptrs(scans)
        g = np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(-1, 6))
        _check(lib().fbr_batch_stage(self._h, arr, ptr(n_in), len(keep), ptr(g)), "fbr_batch_stage")
        self._staged = len(keep)

    def batch_launch(self):
        _check(lib().fbr_batch_launch(self._h), "fbr_batch_launch")

    def batch_wait(self):
        _check(lib().fbr_batch_wait(self._h), "fbr_batch_wait")

    def batch_results(self):
        poses = np.zeros((self._staged, 6), np.float32)
        stats = np.zeros(self._staged, REG_STATS)
        _check(lib().fbr_batch_results(self._h, ptr(poses), ptr(stats)), "fbr_batch_results")
        return poses, stats

    def batch_set_full_masks(self, on=True):
        """Later batch launches compute whole feature masks (fbr_batch_set_full_masks)."""
        _check(lib().fbr_batch_set_full_masks(self._h, int(bool(on))), "fbr_batch_set_full_masks")

    def batch_labels(self, job):
        """cloudLabel of batch job `job` of the latest (full-mask) launch: int8 [n_points]."""
        n = _I64()
        rc = lib().fbr_batch_labels(self._h, int(job), None, 0, ctypes.byref(n))
        if rc not in (0, -4):  # FBR_ERR_CAPACITY: the count is in n
            _check(rc, "fbr_batch_labels")
        out = np.zeros(max(n.value, 1), np.int8)
        _check(lib().fbr_batch_labels(self._h, int(job), ptr(out), len(out), ctypes.byref(n)), "fbr_batch_labels")
        return out[:n.value]

    def feature_paths(self):
        """Tests: which walk each ring segment of the k_features launches since the last call took
        (fbr_diag_feature_paths; FeatArgs::paths in csrc/fbr_kernels.h gives the encoding): uint32
        [launch slots * max_batch, n_scan], zero where no ring ran.  The first call only arms the
        record."""
        f = lib().fbr_diag_feature_paths
        f.restype, f.argtypes = ctypes.c_int, [_VP, _VP, _I64, _VP]
        n = _I64()
        _check(f(self._h, None, 0, ctypes.byref(n)), "fbr_diag_feature_paths")
        out = np.zeros(max(n.value, 1), np.uint32)
        _check(f(self._h, ptr(out), len(out), ctypes.byref(n)), "fbr_diag_feature_paths")
        return out[:n.value].reshape(-1, self.params.n_scan)

    def batch_export(self, device_ptr):
        """Enqueue the 32 B/job pose records into device memory at `device_ptr` (int address)."""
        _check(lib().fbr_batch_export(self._h, ctypes.c_void_p(device_ptr)), "fbr_batch_export")

    def batch_flush(self):
        """Enqueue the rest of every launch in flight (no device synchronisation)."""
        _check(lib().fbr_batch_flush(self._h), "fbr_batch_flush")

    def batch_export_ready(self, device_ptr, wait_stream=0):
        """Pipelined export: the records of the latest fully enqueued, not yet exported launch into
        `device_ptr`, after the work queued on `wait_stream` (a HIP stream handle, 0 = none).
        Returns (launch_id, export stream handle); launch_id -1 = nothing exported."""
        st, lid = _VP(), _I64()
        _check(lib().fbr_batch_export_ready(self._h, ctypes.c_void_p(device_ptr), ctypes.c_void_p(wait_stream or None),
                                            ctypes.byref(st), ctypes.byref(lid)), "fbr_batch_export_ready")
        return lid.value, st.value or 0

    def diag_ring_filter(self, kernel):
        """Diagnostic: the per-ring surf filter kernel of this context (-1 by launch size, 0 the
        512-thread kernel, 2 four waves per ring; fbr_diag_ring_filter)."""
        f = lib().fbr_diag_ring_filter
        f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
        _check(f(self._h, int(kernel)), "fbr_diag_ring_filter")

    def diag_batch_cloud(self, force_wide=-1):
        """Diagnostic: force_wide 1 keeps the float4 projected cloud in the batch launches that
        would take 12-B (x, y, z) records, 0 restores the default, -1 leaves the switch
        (fbr_diag_batch_cloud).  Returns the record size of the latest batch launch's cloud: 12, 16,
        or 0 before any launch."""
        f = lib().fbr_diag_batch_cloud
        f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int, _VP]
        n = _I32()
        _check(f(self._h, int(force_wide), ctypes.byref(n)), "fbr_diag_batch_cloud")
        return n.value

    def diag_knn_last(self):
        """Diagnostic: the last neighbour search of the latest single-scan registration on this
        context (fbr_diag_knn_last).  Returns a dict: n_corner / n_surf (down-sampled query counts),
        queries (n, 3) float32 map-frame positions as that pass computed them (corner queries
        first), nbr (n, 5) int32 map indices into get_map()'s clouds in (d2, index) order (-1 five
        times: no correspondence), desc (iterations, r, rx, flat, sparse, lpq, fused, tiles of the
        kernel that ran the pass)."""
        f = lib().fbr_diag_knn_last
        f.restype, f.argtypes = ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _I64, _VP]
        nc, ns = _I32(), _I32()
        desc = (_I32 * 8)()
        _check(f(self._h, ctypes.byref(nc), ctypes.byref(ns), None, None, 0, desc), "fbr_diag_knn_last")
        n = nc.value + ns.value
        q = np.zeros((max(n, 1), 3), np.float32)
        nbr = np.zeros((max(n, 1), 5), np.int32)
        _check(f(self._h, ctypes.byref(nc), ctypes.byref(ns), ptr(q), ptr(nbr), max(n, 1), desc), "fbr_diag_knn_last")
        names = ("iterations", "r", "rx", "flat", "sparse", "lpq", "fused", "tiles")
        return dict(n_corner=nc.value, n_surf=ns.value, queries=q[:n].copy(), nbr=nbr[:n].copy(),
                    desc={k: int(v) for k, v in zip(names, desc)})

    def diag_gn_last(self):
        """Diagnostic: the residual pass behind diag_knn_last's search (fbr_diag_gn_last).  Returns a
        dict: n_corner / n_surf; per query in diag_knn_last's order points (n, 3) float32 (the
        down-sampled scan-frame point), fit_state (n,) int8 (0 none, 1
        fitted, 2 rejected), fit (n, 6) float32, nsame (n,) int8 (-1 everywhere: the fused pass keeps
        none); per work item items (m, 4) int32 {job, kind, first query, queries} and partial (m, 32)
        float64; T (12,) and trig (6,) the pass ran at."""
        f = lib().fbr_diag_gn_last
        f.restype = ctypes.c_int
        f.argtypes = [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _I64, _VP]
        nc, ns, ni = _I32(), _I32(), _I32()
        _check(f(self._h, ctypes.byref(nc), ctypes.byref(ns), None, None, None, None, 0, ctypes.byref(ni), None, None, 0,
                 None),
               "fbr_diag_gn_last")
        n, m = nc.value + ns.value, ni.value
        state, same = np.zeros(max(n, 1), np.int8), np.zeros(max(n, 1), np.int8)
        fit, pts = np.zeros((max(n, 1), 6), np.float32), np.zeros((max(n, 1), 3), np.float32)
        items = np.zeros((max(m, 1), 4), np.int32)
        partial = np.zeros((max(m, 1), 32), np.float64)
        tt = np.zeros(18, np.float32)
        _check(f(self._h, ctypes.byref(nc), ctypes.byref(ns), ptr(pts), ptr(state), ptr(fit), ptr(same), max(n, 1),
                 ctypes.byref(ni),
                 ptr(items), ptr(partial), max(m, 1), ptr(tt)), "fbr_diag_gn_last")
        return dict(n_corner=nc.value, n_surf=ns.value, points=pts[:n].copy(), fit_state=state[:n].copy(), fit=fit[:n].copy(),
                    nsame=same[:n].copy(), items=items[:m].copy(), partial=partial[:m].copy(), T=tt[:12].copy(),
                    trig=tt[12:].copy())

    def diag_force_capacity_error(self, job):
        """Diagnostic: batch job `job` of the following launches is reported as over the feature
        capacity (fbr_diag_force_capacity_error); job < 0 clears it."""
        f = lib().fbr_diag_force_capacity_error
        f.restype, f.argtypes = ctypes.c_int, [_VP, ctypes.c_int]
        _check(f(self._h, int(job)), "fbr_diag_force_capacity_error")

    def batch_bytes(self):
        t, g = ctypes.c_double(), ctypes.c_double()
        _check(lib().fbr_batch_bytes(self._h, ctypes.byref(t), ctypes.byref(g)), "fbr_batch_bytes")
        return t.value, g.value

    def set_profiling(self, on=True, kernels=None):
        """Time kernels with HIP events on the ctx stream; `kernels` restricts it to those names."""
        names = None if not kernels else ",".join(kernels).encode()
        _check(lib().fbr_set_profiling_kernels(self._h, names), "fbr_set_profiling_kernels")
        _check(lib().fbr_set_profiling(self._h, 1 if on else 0), "fbr_set_profiling")

    def kernel_time(self, name):
        ms, n = ctypes.c_double(), _I64()
        _check(lib().fbr_kernel_time(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)),
               "fbr_kernel_time")
        return ms.value, n.value

    def voxel_grid(self, pts, leaf):
        pts = _as_points(pts, POINT_XYZI)
        out = np.zeros(max(len(pts), 1), POINT_XYZI)
        n = _I64()
        _check(lib().fbr_voxel_grid(self._h, ptr(pts), len(pts), ctypes.c_float(leaf), ptr(out),
                                    ctypes.byref(n)), "fbr_voxel_grid")
        return out[:n.value].copy()


def comm_unique_id():
    """fbr_comm_unique_id: the 128-byte RCCL id rank 0 makes and hands to the other ranks."""
    buf = (ctypes.c_uint8 * 128)()
    _check(lib().fbr_comm_unique_id(buf), "fbr_comm_unique_id")
    return bytes(buf)


class Comm:
    """The pose-record communicator of one rank (fbr_comm_create): RCCL over the context's device.
    allgather(launch_id, recv_ptr, wait_stream) all-gathers that launch's 32-B records of every rank
    into the device buffer recv_ptr ([nranks][max_jobs][8] f32), after the work queued on
    wait_stream (the caller's stream still reading recv, or None), and returns the HIP stream to
    wait on before reading recv."""

    def __init__(self, ctx, uid, nranks, rank, max_jobs):
        self._h = _VP()
        idb = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().fbr_comm_create(ctypes.byref(self._h), ctx._h, idb, int(nranks), int(rank), int(max_jobs)),
               "fbr_comm_create")
        self._ctx = ctx
        self.nranks, self.rank, self.max_jobs = int(nranks), int(rank), int(max_jobs)

    def allgather(self, launch_id, recv_ptr, wait_stream=None):
        st = _VP()
        _check(lib().fbr_batch_allgather(self._ctx._h, self._h, int(launch_id), ctypes.c_void_p(recv_ptr),
                                         ctypes.c_void_p(wait_stream or None), ctypes.byref(st)), "fbr_batch_allgather")
        return st.value or 0

    def close(self):
        if self._h:
            _check(lib().fbr_comm_destroy(self._h), "fbr_comm_destroy")
            self._h = _VP()


__all__ = ["Context", "Comm", "comm_unique_id", "FbrError", "FbrParams", "default_params", "lib", "device_count",
           "affine_from_pose", "pose_from_affine", "pcd_read", "pcd_write", "pcd_write_poses", "msg_to_points", "points_to_msg", "PointCloud2",
           "imu_convert", "imu_deskew_info", "reg_info_variances",
           "EXPORTED_SYMBOLS"]
