"""Host-side mirror of the reference's interface for the hot path, on top of the C ABI.

Rust is not in the toolchain here, so the thin host layer a Rust shim would be is
written in Python with the reference's own names and argument meaning:

    reference (Rust)                                     here
    ---------------------------------------------------  -----------------------------------------
    CameraModel                  camera.rs:3-10          CameraModel
    StereoProcessor::new/process stereo.rs:37,52         StereoProcessor(camera, n_features).process
    FeatureSet / StereoFrame     stereo.rs:15-29         FeatureSet / StereoFrame
    descriptor_distance          stereo.rs:166           descriptor_distance
    BFMatcher(HAMMING,true)      tracker.rs:1001-1010    bf_match_crosscheck
    track_with_reference_kf      tracker.rs:992-1064     track_with_reference_kf / Handle.track_reference[_device]
    LocalBAConfigLM              local_ba_lm.rs:96-119   LocalBAConfigLM
    VisualBAProblemData/Result   local_ba_lm.rs:48-93    VisualBAProblemData / VisualBAResultData
    solve_visual_ba              local_ba_lm.rs:912      solve_visual_ba
    solve_pnp_ransac[_detailed]  pnp.rs:29-134           solve_pnp_ransac[_detailed] / Handle.solve_pnp_ransac_batch
    PoseInertialConfig/Result    pose_inertial_optim.rs:19-62    PoseInertialConfig / PoseInertialResult
    pose_inertial_optimization   pose_inertial_optim.rs:94-216   pose_inertial_optimization / Handle.pose_inertial_optimization[_batch]

Everything computes on the GPU through liborbx_hip.so; there is no CPU fallback, and a missing
library or device raises.
"""
import atexit
import ctypes as C
import math
import os
import weakref
from collections import deque
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from .build import LIB_PATH

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"),
                   ("distance", "<f4")])
BA_OBS = np.dtype([("kf_idx", "<i4"), ("fixed_idx", "<i4"), ("mp_idx", "<i4"), ("_pad", "<i4"),
                   ("u", "<f8"), ("v", "<f8")])
# orbx_ba_obs32 (include/orbx.h): the same observation in 16 bytes — kf_idx >= 0 optimised keyframe, < 0 fixed observer -1 - kf_idx (F = identity); u, v f32
BA_OBS32 = np.dtype([("kf_idx", "<i4"), ("mp_idx", "<i4"), ("u", "<f4"), ("v", "<f4")])


BA_OBS32_STEREO = 0x40000000   # ORBX_BA_OBS32_STEREO: is_stereo in mp_idx, read by the inertial entry points only


def ba_obs_to_obs32(obs, n_fixed, inertial=False):
    """orbx_ba_obs -> orbx_ba_obs32, or None if a coordinate is not exactly an f32 (the reference's always are: kp.pt() widened, local_ba_lm.rs:870-872).
    inertial=True: `_pad & 1` (is_stereo) is carried into mp_idx as BA_OBS32_STEREO — the form ba_solve_inertial_obs32 takes."""
    obs = np.ascontiguousarray(obs, BA_OBS)
    u32, v32 = obs["u"].astype(np.float32), obs["v"].astype(np.float32)
    if not (np.array_equal(u32.astype(np.float64), obs["u"]) and np.array_equal(v32.astype(np.float64), obs["v"])):
        return None
    out = np.zeros(len(obs), BA_OBS32)
    fixed = np.where(obs["fixed_idx"] >= 0, obs["fixed_idx"], n_fixed)
    out["kf_idx"] = np.where(obs["kf_idx"] >= 0, obs["kf_idx"], -1 - fixed)
    out["mp_idx"] = obs["mp_idx"]; out["u"] = u32; out["v"] = v32
    if inertial:
        if len(obs) and (int(obs["mp_idx"].max()) >= BA_OBS32_STEREO):
            raise ValueError("a point index reaches the stereo flag's bit")
        out["mp_idx"] = np.where((obs["_pad"] & 1) != 0, obs["mp_idx"] | BA_OBS32_STEREO, obs["mp_idx"])
    return out



ORBX_OK, ORBX_ERR_INVALID, ORBX_ERR_NO_DEVICE, ORBX_ERR_HIP = 0, -1, -2, -3
ORBX_ERR_CAPACITY, ORBX_ERR_NUMERIC, ORBX_ERR_EMPTY = -4, -5, -6

# ORB-SLAM3 matching thresholds, stereo.rs:10-12
TH_HIGH, TH_LOW, NN_RATIO = 100, 50, 0.75

# every symbol include/orbx.h declares
ABI_VERSION = 2      # = ORBX_ABI_VERSION of include/orbx.h, whose struct layouts the ctypes mirrors below restate
ABI_SYMBOLS = [
    "orbx_version", "orbx_abi_version", "orbx_last_error", "orbx_default_orb_params", "orbx_create", "orbx_destroy",
    "orbx_stream", "orbx_synchronize", "orbx_process_stereo", "orbx_process_stereo_batch_device",
    "orbx_process_stereo_batch", "orbx_host_alloc", "orbx_host_free",
    "orbx_extract_batch_device", "orbx_check_status", "orbx_stereo_match",
    "orbx_stereo_match_batch_device", "orbx_hamming_match_crosscheck",
    "orbx_hamming_match_crosscheck_device", "orbx_hamming_batch", "orbx_hamming_batch_device",
    "orbx_keyframe_create", "orbx_keyframe_destroy", "orbx_keyframe_info", "orbx_keyframe_set_pose", "orbx_keyframe_set_map_points",
    "orbx_keyframe_get_map_points", "orbx_keyframe_download", "orbx_keyframe_device_keypoints", "orbx_keyframe_device_descriptors",
    "orbx_keyframe_guided_match", "orbx_keyframe_search_for_triangulation", "orbx_keyframe_fuse_search",
    "orbx_default_ba_config", "orbx_ba_set_allreduce", "orbx_rccl_unique_id", "orbx_ba_init_rccl", "orbx_ba_set_rccl_comm", "orbx_ba_has_collective", "orbx_ba_rccl_world", "orbx_ba_solve_visual", "orbx_ba_solve_visual_obs32", "orbx_ba_solve_global_obs32", "orbx_ba_solve_visual_batch", "orbx_debug_ba_blocks", "orbx_debug_imu_residual", "orbx_ba_solve_global", "orbx_default_inertial_ba_config", "orbx_ba_solve_inertial",
    "orbx_guided_match", "orbx_guided_match_device", "orbx_search_for_triangulation", "orbx_search_for_triangulation_device", "orbx_search_for_triangulation_bow",
    "orbx_fuse_search", "orbx_fuse_search_device",
    "orbx_vocab_load_text", "orbx_vocab_create", "orbx_vocab_destroy", "orbx_vocab_info", "orbx_vocab_nodes",
    "orbx_bow_transform", "orbx_bow_transform_device", "orbx_bow_vectors", "orbx_bow_vectors_device", "orbx_bow_score",
    "orbx_png_decode_gray8", "orbx_euroc_open", "orbx_euroc_close", "orbx_euroc_len", "orbx_euroc_last_error",
    "orbx_euroc_frame_timestamp", "orbx_euroc_calibration", "orbx_euroc_read_pairs",
    "orbx_set_profiling", "orbx_set_profiling_only", "orbx_get_kernel_times", "orbx_debug_read_level",
    "orbx_debug_read_candidates",
    "orbx_default_pnp_config", "orbx_pnp_ransac", "orbx_pnp_ransac_batch", "orbx_pnp_ransac_batch_device",
    "orbx_default_pose_inertial_config", "orbx_pose_inertial_optimize", "orbx_pose_inertial_batch", "orbx_pose_inertial_batch_device",
    "orbx_default_loop_detector_config", "orbx_kfdb_create", "orbx_kfdb_destroy", "orbx_kfdb_add", "orbx_kfdb_add_device", "orbx_kfdb_erase",
    "orbx_kfdb_set_bad", "orbx_kfdb_size", "orbx_kfdb_compact", "orbx_kfdb_download", "orbx_kfdb_score", "orbx_kfdb_detect_candidates",
    "orbx_kfdb_detect_loop_candidates", "orbx_kfdb_detect_loop_candidates_batch",
    "orbx_default_triangulation_config", "orbx_triangulate_pairs", "orbx_triangulate_pairs_device", "orbx_keyframe_set_feature_nodes",
    "orbx_keyframe_triangulate_from_neighbors",
    "orbx_default_track_config", "orbx_track_frames", "orbx_track_frames_device",
    "orbx_track_reference", "orbx_track_reference_device", "orbx_keyframe_track_reference",
    "orbx_default_sim3_config", "orbx_default_loop_verify_config", "orbx_sim3_ransac_batch", "orbx_sim3_ransac_batch_device",
    "orbx_verify_loop_candidates", "orbx_verify_loop_candidates_device", "orbx_keyframe_verify_loop_candidates",
    "orbx_refresh_map_points", "orbx_refresh_map_points_device", "orbx_keyframe_refresh_map_points",
    "orbx_map_points_create", "orbx_map_points_destroy", "orbx_map_points_info", "orbx_map_points_set", "orbx_map_points_set_device",
    "orbx_map_points_erase", "orbx_map_points_download", "orbx_keyframe_set_map_point_slots", "orbx_map_select_points_device",
    "orbx_map_track_frames_device", "orbx_map_track_frames", "orbx_map_track_reference_device",
    "orbx_map_covisibility_device", "orbx_map_covisibility", "orbx_map_track_local_device", "orbx_map_track_local",
    "orbx_map_collect_ba_window_device", "orbx_map_collect_ba_window", "orbx_ba_solve_visual_obs32_device", "orbx_map_local_ba",
    "orbx_map_observations_device", "orbx_map_observations", "orbx_map_refresh_points_device", "orbx_map_refresh_points",
    "orbx_map_keyframe_redundancy_device", "orbx_map_keyframe_redundancy",
    "orbx_keyframe_get_map_point_slots", "orbx_map_fuse_device", "orbx_map_fuse", "orbx_map_search_in_neighbors",
    "orbx_keyframe_set_map_point_slots_device", "orbx_map_create_points_device", "orbx_map_create_points", "orbx_map_remove_points",
    "orbx_map_cull_points",
    "orbx_ba_solve_inertial_obs32", "orbx_ba_solve_inertial_obs32_device", "orbx_map_collect_inertial_window_device",
    "orbx_map_collect_inertial_window", "orbx_map_local_inertial_ba",
    "orbx_ba_solve_global_map", "orbx_ba_solve_global_map_obs32", "orbx_ba_solve_global_map_obs32_device", "orbx_ba_global_map_max_keyframes",
    "orbx_map_collect_global_device", "orbx_map_collect_global", "orbx_map_global_ba",
    "orbx_default_loop_correct_config", "orbx_map_loop_max_keyframes", "orbx_map_correct_loop_device", "orbx_map_correct_loop", "orbx_map_close_loop",
]
MAP_SOURCE_KEYFRAMES, MAP_SOURCE_SLOTS = 0, 1      # orbx_map_select_points_device's source kinds
MAP_CREATE_STEREO, MAP_CREATE_NEIGHBOURS = 1, 2    # orbx_map_create_points' phases (a bit mask)


BOW_VECTORS_MAX = 8192      # descriptors per orbx_bow_vectors call (bow_kernels.hip: BOWV_MAX)


def _seq_sum(a):
    """left-to-right f64 sum (the order the device kernel adds a run in)"""
    t = 0.0
    for x in a:
        t += float(x)
    return t


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbx error %d: %s" % (code, msg))
        self.code = code


class _Camera(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "baseline")]


class _OrbParams(C.Structure):
    _fields_ = [("n_features", C.c_int), ("scale_factor", C.c_float), ("n_levels", C.c_int),
                ("edge_threshold", C.c_int), ("first_level", C.c_int), ("wta_k", C.c_int),
                ("score_type", C.c_int), ("patch_size", C.c_int), ("fast_threshold", C.c_int)]


class _BaConfig(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("param_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("huber_threshold", C.c_double),
                ("max_covisible_keyframes", C.c_int)]


class _LoopCorrectConfig(C.Structure):
    _fields_ = [("min_covisibility_weight", C.c_int), ("max_propagation_depth", C.c_int)]


class _InertialBaConfig(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("window_size", C.c_int), ("huber_threshold_mono", C.c_double),
                ("huber_threshold_stereo", C.c_double), ("initial_lambda", C.c_double), ("gyro_rw_info", C.c_double),
                ("accel_rw_info", C.c_double)]


class _KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("launches", C.c_int)]


class _BaWindow(C.Structure):
    """orbx_ba_window (include/orbx.h)"""
    _fields_ = [("K", C.c_int), ("poses_cw", C.c_void_p), ("F", C.c_int), ("fixed_poses_cw", C.c_void_p), ("M", C.c_int),
                ("points", C.c_void_p), ("N", C.c_int), ("obs", C.c_void_p), ("poses_wc_out", C.c_void_p), ("status", C.c_int),
                ("iterations", C.c_int), ("initial_error", C.c_double), ("final_error", C.c_double), ("obs32", C.c_void_p)]


class _PnpConfig(C.Structure):
    """orbx_pnp_config (include/orbx.h)"""
    _fields_ = [("max_iterations", C.c_int), ("reproj_error", C.c_double), ("confidence", C.c_double), ("model_points", C.c_int),
                ("hypothesis_iterations", C.c_int), ("refine_iterations", C.c_int), ("seed", C.c_uint64)]


class _PnpResult(C.Structure):
    """orbx_pnp_result (include/orbx.h)"""
    _fields_ = [("status", C.c_int), ("n_inliers", C.c_int), ("ransac_inliers", C.c_int), ("best_hypothesis", C.c_int),
                ("hypotheses_evaluated", C.c_int), ("refine_iterations", C.c_int), ("final_rms", C.c_double)]


# orbx_pnp_result as a numpy record (the batch forms' results array)
PNP_RESULT = np.dtype([("status", "<i4"), ("n_inliers", "<i4"), ("ransac_inliers", "<i4"), ("best_hypothesis", "<i4"),
                       ("hypotheses_evaluated", "<i4"), ("refine_iterations", "<i4"), ("final_rms", "<f8")])
PNP_OK, PNP_NO_MODEL, PNP_TOO_FEW, PNP_OVER_MAX_N = 0, 1, 2, 3


class _PoseInertialConfig(C.Structure):
    """orbx_pose_inertial_config (include/orbx.h)"""
    _fields_ = [("max_iterations", C.c_int), ("chi2_mono_init", C.c_double), ("chi2_stereo_init", C.c_double),
                ("chi2_mono_final", C.c_double), ("chi2_stereo_final", C.c_double), ("imu_weight", C.c_double)]


class _PoseInertialResult(C.Structure):
    """orbx_pose_inertial_result (include/orbx.h)"""
    _fields_ = [("status", C.c_int), ("num_inliers", C.c_int), ("num_observations", C.c_int), ("iterations", C.c_int)]


# orbx_pose_inertial_result as a numpy record (the batch forms' results array)
POSE_INERTIAL_RESULT = np.dtype([("status", "<i4"), ("num_inliers", "<i4"), ("num_observations", "<i4"), ("iterations", "<i4")])
POSE_INERTIAL_OK, POSE_INERTIAL_TOO_FEW, POSE_INERTIAL_SINGULAR = 0, 1, 2


class _TrackConfig(C.Structure):
    """orbx_track_config (include/orbx.h)"""
    _fields_ = [("mode", C.c_int), ("radius", C.c_double), ("img_w", C.c_double), ("img_h", C.c_double), ("min_correspondences", C.c_int),
                ("min_inliers", C.c_int)]


# orbx_track_result as a numpy record (the results array of track_frames[_device])
TRACK_RESULT = np.dtype([("status", "<i4"), ("n_in_front", "<i4"), ("n_correspondences", "<i4"), ("n_inliers", "<i4")])
TRACK_OK, TRACK_NO_MODEL, TRACK_TOO_FEW_CORRESPONDENCES, TRACK_TOO_FEW_INLIERS = 0, 1, 2, 3
TRACK_MOTION_MODEL, TRACK_LOCAL_MAP = 0, 1      # orbx_track_config.mode
# orbx_track_ref_result as a numpy record (the results array of track_reference[_device]); statuses are TRACK_*
TRACK_REF_RESULT = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("n_correspondences", "<i4"), ("n_inliers", "<i4")])


class _Sim3Config(C.Structure):
    """orbx_sim3_config (include/orbx.h)"""
    _fields_ = [("max_iterations", C.c_int), ("inlier_threshold", C.c_double), ("min_inliers", C.c_int), ("fix_scale", C.c_int),
                ("probability", C.c_double), ("seed", C.c_uint64)]


class _LoopVerifyConfig(C.Structure):
    """orbx_loop_verify_config (include/orbx.h)"""
    _fields_ = [("min_stereo_points", C.c_int), ("min_matches", C.c_int), ("min_pairs", C.c_int), ("min_inliers", C.c_int),
                ("min_verified", C.c_int), ("match_max_dist", C.c_uint), ("match_ratio", C.c_double), ("chi2", C.c_double),
                ("scale_factor", C.c_double), ("sim3", _Sim3Config)]


# orbx_sim3_result / orbx_loop_verify_result as numpy records (the results arrays of the Sim3 and loop-verification calls)
SIM3_RESULT = np.dtype([("status", "<i4"), ("best_hypothesis", "<i4"), ("ransac_inliers", "<i4"), ("n_inliers", "<i4"), ("refined", "<i4"),
                        ("reserved_", "<i4"), ("mse", "<f8")])
LOOP_VERIFY_RESULT = np.dtype([("status", "<i4"), ("n_matches", "<i4"), ("n_pairs", "<i4"), ("best_hypothesis", "<i4"),
                               ("ransac_inliers", "<i4"), ("n_inliers", "<i4"), ("refined", "<i4"), ("n_verified", "<i4"), ("mse", "<f8")])
SIM3_OK, SIM3_NO_MODEL = 0, 1
(LOOP_OK, LOOP_TOO_FEW_POINTS, LOOP_TOO_FEW_MATCHES, LOOP_TOO_FEW_PAIRS, LOOP_NO_MODEL, LOOP_TOO_FEW_INLIERS,
 LOOP_TOO_FEW_VERIFIED) = range(7)
# orbx_mp_refresh_record
MP_REFRESH_RECORD = np.dtype([("chosen", "<i4"), ("best_max_dist", "<u4"), ("n_desc", "<u4"), ("n_observers", "<u4")])
assert MP_REFRESH_RECORD.itemsize == 16
LOOP_VERIFY_MAX_FEAT = 1 << 22            # features per keyframe (loop_verify_kernels.hip: LV_MAX_FEAT)


class _LoopDetectorConfig(C.Structure):
    """orbx_loop_detector_config (include/orbx.h)"""
    _fields_ = [("min_score_ratio", C.c_double), ("consistency_threshold", C.c_int), ("min_covisibles_for_threshold", C.c_int),
                ("max_covisibles_to_check", C.c_int), ("min_temporal_gap", C.c_int)]


class _TriangulationConfig(C.Structure):
    """orbx_triangulation_config (include/orbx.h)"""
    _fields_ = [("num_neighbors", C.c_int), ("max_descriptor_dist", C.c_uint), ("min_baseline_ratio", C.c_double),
                ("min_parallax_inertial", C.c_double), ("min_parallax_visual", C.c_double), ("max_reproj_error_mono", C.c_double),
                ("max_reproj_error_stereo", C.c_double), ("scale_ratio_factor", C.c_double)]


# ORBX_TRI_* / ORBX_TRI_METHOD_*: a pair's status word is status | method << 8
(TRI_CREATED, TRI_SKIPPED, TRI_DLT_DEGENERATE, TRI_REJ_DEPTH, TRI_REJ_REPROJ1, TRI_REJ_REPROJ2, TRI_REJ_DIST, TRI_REJ_SCALE,
 TRI_BAD_INDEX) = range(9)
TRI_METHOD_DLT, TRI_METHOD_STEREO_CURRENT, TRI_METHOD_STEREO_NEIGHBOUR = 0, 1, 2
TRI_MAX_NEIGHBOURS = 256
FEATURE_NODE_NONE = 0xFFFFFFFF            # orbx_keyframe_set_feature_nodes: the feature is in no FeatureVector list


KFDB_SCORE_L1, KFDB_SCORE_DOT = 0, 1      # ORBX_KFDB_SCORE_*
KFDB_MAX_WORDS = 8192                     # words of one BowVector in the database


SHOULD_STOP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def _stop_callback(should_stop):
    """A solve's orbx_should_stop_fn argument; the caller keeps it in a local while the C call runs (ctypes frees an unreferenced callback)."""
    return SHOULD_STOP_FN(lambda user: 1 if should_stop() else 0) if should_stop else C.cast(None, SHOULD_STOP_FN)


def _solve_outs():
    return C.c_int(), C.c_double(), C.c_double()          # a solve's iterations, initial_error, final_error: passed with C.byref

_lib = None
_live_handles = weakref.WeakSet()


@atexit.register
def _close_live_handles():
    # destroy handles while the HIP runtime is still loaded (interpreter teardown order is arbitrary)
    for h in list(_live_handles):
        try:
            h.close()
        except Exception:
            pass


def load_library():
    """dlopen liborbx_hip.so.  Raises if it has not been built: the product has no other path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "liborbx_hip.so is missing (%s): build it with __graft_entry__.build(); "
                "this package has no CPU or PyTorch fallback" % LIB_PATH)
        if not os.environ.get("ORBX_NO_TORCH_PRELOAD"):
            # PyTorch-ROCm wheels carry their own libamdhip64.so.7; two HIP runtimes in one process
            # do not coexist ("No HIP GPUs are available").  Loading torch first makes the dynamic
            # linker bind this library's libamdhip64.so.7 dependency to the copy torch already
            # mapped (same soname), so device memory and streams are shared with torch.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        L.orbx_version.restype = C.c_char_p
        abi = getattr(L, "orbx_abi_version", None)                  # (a library from before the symbol existed counts as version 0)
        if abi is None or abi() != ABI_VERSION:
            raise RuntimeError("liborbx_hip.so was built from an orbx.h of ABI version %d, this mirror restates version %d: rebuild with "
                               "__graft_entry__.build()" % (abi() if abi else 0, ABI_VERSION))
        L.orbx_last_error.restype = C.c_char_p
        L.orbx_last_error.argtypes = [C.c_void_p]
        L.orbx_stream.restype = C.c_void_p
        L.orbx_stream.argtypes = [C.c_void_p]
        L.orbx_destroy.argtypes = [C.c_void_p]
        L.orbx_euroc_close.argtypes = [C.c_void_p]
        L.orbx_euroc_close.restype = None
        L.orbx_euroc_len.argtypes = [C.c_void_p]
        L.orbx_euroc_last_error.argtypes = [C.c_void_p]
        L.orbx_euroc_last_error.restype = C.c_char_p
        L.orbx_euroc_open.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.orbx_euroc_frame_timestamp.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.orbx_euroc_calibration.argtypes = [C.c_void_p] * 5
        L.orbx_euroc_read_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.orbx_png_decode_gray8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.orbx_vocab_destroy.argtypes = [C.c_void_p]
        L.orbx_vocab_destroy.restype = None
        L.orbx_vocab_info.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.orbx_vocab_nodes.argtypes = [C.c_void_p] * 5
        L.orbx_vocab_load_text.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        L.orbx_bow_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.orbx_destroy.restype = None
        L.orbx_keyframe_set_map_point_slots_device.argtypes = [C.c_void_p] * 3
        L.orbx_map_create_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                    C.c_int] + [C.c_void_p] * 8
        L.orbx_map_create_points.argtypes = L.orbx_map_create_points_device.argtypes[:11] + [C.c_void_p] * 7
        L.orbx_map_remove_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.orbx_map_cull_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for name in ABI_SYMBOLS:
            getattr(L, name)
        _lib = L
    return _lib


def _vp(x):
    """void* from a numpy array, an int device pointer, a torch tensor, or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


@dataclass
class CameraModel:
    """camera.rs:3-10"""
    fx: float
    fy: float
    cx: float
    cy: float
    baseline: float

    def _c(self):
        return _Camera(self.fx, self.fy, self.cx, self.cy, self.baseline)


@dataclass
class LocalBAConfigLM:
    """local_ba_lm.rs:96-119 (Default impl :109-119)"""
    max_iterations: int = 10
    param_tolerance: float = 1e-8
    gradient_tolerance: float = 1e-8
    huber_threshold: float = math.sqrt(5.991)
    max_covisible_keyframes: int = 20

    def _c(self):
        return _BaConfig(self.max_iterations, self.param_tolerance, self.gradient_tolerance,
                         self.huber_threshold, self.max_covisible_keyframes)


@dataclass
class GlobalBAConfig:
    """global_ba.rs:21-46 (Default impl :36-45)"""
    max_iterations: int = 10
    param_tolerance: float = 1e-6
    gradient_tolerance: float = 1e-6
    huber_threshold: float = math.sqrt(5.991)

    def _c(self):
        return _BaConfig(self.max_iterations, self.param_tolerance, self.gradient_tolerance, self.huber_threshold, 0)


@dataclass
class LoopCorrectConfig:
    """corrector.rs:97-104 (CorrectorConfig::default)"""
    min_covisibility_weight: int = 15
    max_propagation_depth: int = 100

    def _c(self):
        return _LoopCorrectConfig(self.min_covisibility_weight, self.max_propagation_depth)


@dataclass
class LocalInertialBAConfig:
    """local_inertial_ba.rs:109-141 (Default impl :126-141)"""
    max_iterations: int = 10
    window_size: int = 10
    huber_threshold_mono: float = math.sqrt(5.991)
    huber_threshold_stereo: float = math.sqrt(7.815)
    initial_lambda: float = 1e-2
    gyro_rw_info: float = 1e6
    accel_rw_info: float = 1e4

    def _c(self):
        return _InertialBaConfig(self.max_iterations, self.window_size, self.huber_threshold_mono, self.huber_threshold_stereo,
                                 self.initial_lambda, self.gyro_rw_info, self.accel_rw_info)


@dataclass
class PnPConfig:
    """cv::solvePnPRansac's arguments of pnp.rs:71-84 (100 iterations, 8 px, confidence 0.99) and the [spec] choices of
    orbx_pnp_config (include/orbx.h): OpenCV's 5-point model, 10 LM iterations per hypothesis, 20 for the final refinement,
    the sampler's seed."""
    max_iterations: int = 100
    reproj_error: float = 8.0
    confidence: float = 0.99
    model_points: int = 5
    hypothesis_iterations: int = 10
    refine_iterations: int = 20
    seed: int = 0

    def _c(self):
        return _PnpConfig(self.max_iterations, self.reproj_error, self.confidence, self.model_points, self.hypothesis_iterations,
                          self.refine_iterations, self.seed)


@dataclass
class PnPResult:
    """pnp.rs:12-20: pose (T_wc, 7 doubles qw,qx,qy,qz,tx,ty,tz), inlier_mask [n] bool, reproj_errors [n] f64 (+inf behind the
    camera); stats = the orbx_pnp_result record as a dict (status, n_inliers, ransac_inliers, best_hypothesis,
    hypotheses_evaluated, refine_iterations, final_rms)."""
    pose: np.ndarray
    inlier_mask: np.ndarray
    reproj_errors: np.ndarray
    stats: Dict[str, float] = field(default_factory=dict)


def _pnp_stats(rec):
    return {k: (float(rec[k]) if k == "final_rms" else int(rec[k])) for k in PNP_RESULT.names}


@dataclass
class Sim3SolverConfig:
    """sim3_solver.rs:13-36 and the sampler's seed [spec].  probability is carried and has no effect, as in the reference."""
    max_iterations: int = 300
    inlier_threshold: float = 0.075
    min_inliers: int = 15
    fix_scale: bool = True
    probability: float = 0.99
    seed: int = 0

    def _c(self):
        return _Sim3Config(self.max_iterations, self.inlier_threshold, self.min_inliers, 1 if self.fix_scale else 0, self.probability, self.seed)


@dataclass
class LoopVerifyConfig:
    """The constants of verify_loop_candidate (corrector.rs:132-193, :266, :338, :368) and its solver's configuration (:183)."""
    min_stereo_points: int = 20
    min_matches: int = 15
    min_pairs: int = 15
    min_inliers: int = 15
    min_verified: int = 50
    match_max_dist: int = 50
    match_ratio: float = 0.7
    chi2: float = 5.991
    scale_factor: float = 1.2
    sim3: Sim3SolverConfig = field(default_factory=Sim3SolverConfig)

    def _c(self):
        return _LoopVerifyConfig(self.min_stereo_points, self.min_matches, self.min_pairs, self.min_inliers, self.min_verified,
                                 self.match_max_dist, self.match_ratio, self.chi2, self.scale_factor, self.sim3._c())


@dataclass
class Sim3Result:
    """sim3_solver.rs:39-49: sim3 = (qw,qx,qy,qz, tx,ty,tz, scale) with qw >= 0, inliers = the indices of the inlier
    correspondences, num_inliers, mse; stats = the orbx_sim3_result record as a dict."""
    sim3: np.ndarray
    inliers: np.ndarray
    num_inliers: int
    mse: float
    stats: Dict[str, float] = field(default_factory=dict)


@dataclass
class VerifiedLoop:
    """corrector.rs:33-45.  matched_map_points: the (current, loop) map-point ids of the gathered matches where both features have
    one (:168-173), filtered on the host; feature_matches [k,2] (current feature, loop feature).  stats = the
    orbx_loop_verify_result record as a dict, inlier_mask = Sim3's mask over feature_matches."""
    current_kf_id: int
    loop_kf_id: int
    sim3_current_to_loop: np.ndarray
    matched_map_points: List[Tuple[int, int]]
    feature_matches: np.ndarray
    inlier_mask: np.ndarray = None
    stats: Dict[str, float] = field(default_factory=dict)


@dataclass
class MapPointRefresh:
    """What orbx_refresh_map_points leaves for M map points: mp_desc [M,32] u8 and normals [M,3] (the inputs where a point was not
    updated), min_distance / max_distance [M] and records [M] (MP_REFRESH_RECORD: chosen = position of the kept descriptor in the
    point's observation list or -1, best_max_dist, n_desc, n_observers)."""
    mp_desc: np.ndarray
    normals: np.ndarray
    min_distance: np.ndarray
    max_distance: np.ndarray
    records: np.ndarray

    @property
    def num_descriptors_updated(self):
        """SearchInNeighborsResult::num_descriptors_updated (search_in_neighbors.rs:146-148)."""
        return int((self.records["chosen"] >= 0).sum())


@dataclass
class MapPointRefreshData:
    """MapSnapshot.collect_map_point_refresh: the arrays of a refresh call.  mp_ids: the requested points the snapshot holds, in
    order; positions [M,3]; obs_start [M+1], obs_kf, obs_feat: their observation lists, obs_kf indexing kf_ids (-1: a keyframe the
    snapshot does not hold); kf_ids: the distinct observing keyframes in first-seen order."""
    mp_ids: List[int]
    positions: np.ndarray
    obs_start: np.ndarray
    obs_kf: np.ndarray
    obs_feat: np.ndarray
    kf_ids: List[int]


def _rec_dict(rec):
    return {k: (float(rec[k]) if k == "mse" else int(rec[k])) for k in rec.dtype.names if k != "reserved_"}


@dataclass
class TrackConfig:
    """orbx_track_config (include/orbx.h).  TrackConfig.for_mode(mode) = orbx_default_track_config: radius 15 px, the grid's image
    752 x 480 and the reference's guards — track_local_map (mode 1, tracker.rs:937) 4 correspondences, no inlier guard;
    track_with_motion_model (mode 0, :1173, :1186) 10 and 10."""
    mode: int = TRACK_LOCAL_MAP
    radius: float = 15.0
    img_w: float = 752.0
    img_h: float = 480.0
    min_correspondences: int = 4
    min_inliers: int = 0

    @classmethod
    def for_mode(cls, mode, **kw):
        return cls(mode=mode, min_correspondences=10 if mode == TRACK_MOTION_MODEL else 4, min_inliers=10 if mode == TRACK_MOTION_MODEL else 0, **kw)

    def _c(self):
        return _TrackConfig(self.mode, self.radius, self.img_w, self.img_h, self.min_correspondences, self.min_inliers)


@dataclass
class TrackFrameResult:
    """One frame of Handle.track_frames — the tuple track_local_map returns (tracker.rs:981-988) and the arrays behind it:
    pose (T_wc), n_inliers, matched [n_features] int32 (the index of the map point in the frame's list, -1 = None), reproj_errors
    [n_corr] f64, inlier_mask [n_corr] bool; the correspondences points3d [n_corr,3] f64, points2d [n_corr,2] f32, mp_idx / feat_idx
    [n_corr] int32 in ascending map-point order; status (TRACK_*), n_in_front, and PnP's record as a dict."""
    pose: np.ndarray
    n_inliers: int
    matched: np.ndarray
    reproj_errors: np.ndarray
    inlier_mask: np.ndarray
    points3d: np.ndarray
    points2d: np.ndarray
    mp_idx: np.ndarray
    feat_idx: np.ndarray
    status: int = 0
    n_in_front: int = 0
    pnp_stats: Dict[str, float] = field(default_factory=dict)

    @property
    def inlier_indices(self):
        return np.flatnonzero(self.inlier_mask)

    @property
    def outlier_indices(self):
        return np.flatnonzero(~self.inlier_mask)


@dataclass
class TrackReferenceResult:
    """One frame of Handle.track_reference — track_with_reference_kf (tracker.rs:992-1064) with the arrays behind it: pose (T_wc;
    the prior where status is TRACK_TOO_FEW_CORRESPONDENCES or TRACK_NO_MODEL), matches (DMATCH: every mutual match, query =
    keyframe feature, train = frame feature), the correspondences points3d [n,3] f64 / points2d [n,2] f32 / kf_idx / feat_idx [n]
    int32 in ascending keyframe-feature order, PnP's inlier mask and errors over them, status (TRACK_*) and PnP's record."""
    pose: np.ndarray
    n_inliers: int
    matches: np.ndarray
    reproj_errors: np.ndarray
    inlier_mask: np.ndarray
    points3d: np.ndarray
    points2d: np.ndarray
    kf_idx: np.ndarray
    feat_idx: np.ndarray
    status: int
    pnp_stats: dict

    def pose_or_none(self):
        """the reference's Option<SE3>: Some(pose) unless there were too few correspondences (:1051-1063)"""
        return self.pose if self.status in (TRACK_OK, TRACK_NO_MODEL) else None


@dataclass
class PoseInertialConfig:
    """pose_inertial_optim.rs:19-45: 4 iterations, chi2 12.0 / 15.6 (mono / stereo) falling to 5.991 / 7.815, imu_weight 1.0."""
    max_iterations: int = 4
    chi2_mono_init: float = 12.0
    chi2_stereo_init: float = 15.6
    chi2_mono_final: float = 5.991
    chi2_stereo_final: float = 7.815
    imu_weight: float = 1.0

    def _c(self):
        return _PoseInertialConfig(self.max_iterations, self.chi2_mono_init, self.chi2_stereo_init, self.chi2_mono_final,
                                   self.chi2_stereo_final, self.imu_weight)


@dataclass
class PoseInertialResult:
    """pose_inertial_optim.rs:48-62: pose (T_wc, 7 doubles qw,qx,qy,qz,tx,ty,tz), velocity [3], bias [6] (gyro, accel), num_inliers,
    num_observations, iterations; inlier_mask [n] bool (the final mask) and status (POSE_INERTIAL_*: why the loop ended) besides."""
    pose: np.ndarray
    velocity: np.ndarray
    bias: np.ndarray
    num_inliers: int
    num_observations: int
    iterations: int
    inlier_mask: np.ndarray
    status: int


def _pose_inertial_state(problem):
    """(pose_wc [7], velocity [3], bias [6], prev_kf_pose_wc [7], prev_kf_velocity [3], preint [11]) as f64 arrays"""
    return [np.ascontiguousarray(np.asarray(x, np.float64).reshape(k)) for x, k in zip(problem, (7, 3, 6, 7, 3, 11))]


@dataclass
class TriangulationConfig:
    """TriangulationConfig, triangulation.rs:20-52"""
    num_neighbors: int = 10
    max_descriptor_dist: int = TH_LOW
    min_baseline_ratio: float = 0.01
    min_parallax_inertial: float = math.acos(0.9996)
    min_parallax_visual: float = math.acos(0.9998)
    max_reproj_error_mono: float = 5.991
    max_reproj_error_stereo: float = 7.8
    scale_ratio_factor: float = 1.5

    def _c(self):
        return _TriangulationConfig(self.num_neighbors, self.max_descriptor_dist, self.min_baseline_ratio, self.min_parallax_inertial,
                                    self.min_parallax_visual, self.max_reproj_error_mono, self.max_reproj_error_stereo, self.scale_ratio_factor)


@dataclass
class TriangulationResult:
    """TriangulationResult, triangulation.rs:55-61; per_neighbour [T,4] = searched, matches_found, triangulated, validated."""
    num_new_points: int = 0
    num_pairs_checked: int = 0
    num_matches_found: int = 0
    num_triangulated: int = 0
    num_validated: int = 0
    per_neighbour: Optional[np.ndarray] = None


@dataclass
class FeatureSet:
    """stereo.rs:15-19: keypoints (KEYPOINT records) + descriptors [N,32] u8"""
    keypoints: np.ndarray
    descriptors: np.ndarray


@dataclass
class StereoFrame:
    """stereo.rs:21-29.  points_cam is [nL,3] f64 with `has_point` as the Option mask."""
    left_features: FeatureSet
    right_features: FeatureSet
    matches_lr: np.ndarray
    points_cam: np.ndarray
    has_point: np.ndarray
    timestamp_ns: int

    def points_cam_options(self) -> List[Optional[np.ndarray]]:
        return [self.points_cam[i] if self.has_point[i] else None for i in range(len(self.has_point))]


class Handle:
    """Owns one orbx_handle (one HIP stream on one device).  Not thread-safe, like `&mut self`."""

    def __init__(self, camera: CameraModel, n_features: int, device: int = 0, max_w: int = 752,
                 max_h: int = 480, max_batch: int = 1, orb_params=None):
        L = load_library()
        self._L = L
        p = _OrbParams()
        L.orbx_default_orb_params(C.c_int(n_features), C.byref(p))
        if orb_params:
            for k, v in orb_params.items():
                setattr(p, k, v)
        self.orb_params = p
        self.camera = camera
        self._h = C.c_void_p()
        cam = camera._c()
        rc = L.orbx_create(C.byref(cam), C.byref(p), C.c_int(device), C.c_int(max_w), C.c_int(max_h),
                           C.c_int(max_batch), C.byref(self._h))
        if rc != 0:
            raise OrbxError(rc, L.orbx_last_error(None).decode())
        self.device = device
        self._keep = []
        self._ext_stream = None
        _live_handles.add(self)

    def _after_torch(self, *tensors):
        """Order the library's (non-blocking) stream after whatever torch has queued on its current stream — the
        caller's tensors may still be being written there — and keep the inputs alive until the next synchronise."""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        if self._ext_stream is None:
            self._ext_stream = torch.cuda.ExternalStream(self.stream, device=torch.device("cuda", self.device))
        self._ext_stream.wait_event(ev)
        self._keep.extend(tensors)

    def close(self):
        self._ext_stream = None
        self._keep = []
        if getattr(self, "_h", None) and self._h.value:
            self._L.orbx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise OrbxError(rc, self._L.orbx_last_error(self._h).decode())

    @property
    def stream(self):
        return self._L.orbx_stream(self._h)

    def synchronize(self):
        self._check(self._L.orbx_synchronize(self._h))
        self._keep = []

    def check_status(self):
        rc = self._L.orbx_check_status(self._h)
        self._keep = []
        self._check(rc)

    def set_profiling(self, on=True, only=None):
        """HIP events around every launch (on), or around the launches of the one kernel `only` names."""
        if on and only:
            self._check(self._L.orbx_set_profiling_only(self._h, C.c_char_p(only.encode())))
        else:
            self._check(self._L.orbx_set_profiling(self._h, C.c_int(1 if on else 0)))

    def kernel_times(self):
        arr = (_KernelTime * 64)()
        n = self._L.orbx_get_kernel_times(self._h, arr, C.c_int(64))
        return {arr[i].name.decode(): (arr[i].ms, arr[i].launches) for i in range(min(n, 64))}

    # ---- host-buffer entry points -------------------------------------------------------------
    def process_stereo(self, left, right, cap_kp=None):
        left = np.ascontiguousarray(left, np.uint8)
        right = np.ascontiguousarray(right, np.uint8)
        if left.ndim != 2 or left.shape != right.shape:
            raise ValueError("left/right must be 2-d u8 images of equal size")
        hh, ww = left.shape
        cap = cap_kp or (self.orb_params.n_features + 2048)
        kpL = np.zeros(cap, KEYPOINT); kpR = np.zeros(cap, KEYPOINT)
        dL = np.zeros((cap, 32), np.uint8); dR = np.zeros((cap, 32), np.uint8)
        m = np.zeros(cap, DMATCH); pts = np.zeros((cap, 3), np.float64); has = np.zeros(cap, np.uint8)
        nL = C.c_int(); nR = C.c_int(); nm = C.c_int()
        self._check(self._L.orbx_process_stereo(
            self._h, _vp(left), C.c_size_t(left.strides[0]), _vp(right), C.c_size_t(right.strides[0]),
            C.c_int(ww), C.c_int(hh), _vp(kpL), _vp(dL), C.byref(nL), _vp(kpR), _vp(dR), C.byref(nR),
            C.c_int(cap), _vp(m), C.byref(nm), _vp(pts), _vp(has)))
        return (kpL[:nL.value].copy(), dL[:nL.value].copy(), kpR[:nR.value].copy(), dR[:nR.value].copy(),
                m[:nm.value].copy(), pts[:nL.value].copy(), has[:nL.value].copy())

    def stereo_match(self, kpL, descL, kpR, descR):
        kpL = np.ascontiguousarray(kpL, KEYPOINT); kpR = np.ascontiguousarray(kpR, KEYPOINT)
        descL = np.ascontiguousarray(descL, np.uint8).reshape(-1, 32)
        descR = np.ascontiguousarray(descR, np.uint8).reshape(-1, 32)
        nL, nR = len(kpL), len(kpR)
        m = np.zeros(max(nL, 1), DMATCH); pts = np.zeros((max(nL, 1), 3)); has = np.zeros(max(nL, 1), np.uint8)
        nm = C.c_int()
        self._check(self._L.orbx_stereo_match(self._h, _vp(kpL), _vp(descL), C.c_int(nL), _vp(kpR),
                                              _vp(descR), C.c_int(nR), _vp(m), C.byref(nm), _vp(pts), _vp(has)))
        return m[:nm.value].copy(), pts[:nL].copy(), has[:nL].copy()

    def hamming_match_crosscheck(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros(max(len(q), 1), DMATCH)
        n = C.c_int()
        self._check(self._L.orbx_hamming_match_crosscheck(self._h, _vp(q), C.c_int(len(q)), _vp(t),
                                                          C.c_int(len(t)), _vp(out), C.byref(n)))
        return out[:n.value].copy()

    def guided_match(self, kp, desc, img_w, img_h, q_uv, q_desc, radius, mode):
        """FeatureGrid + descriptor search (tracking_frame.rs:52-128; tracker.rs:880-923 mode 1, :1126-1157 mode 0)."""
        kp = np.ascontiguousarray(kp, KEYPOINT); desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        q_uv = np.ascontiguousarray(q_uv, np.float64).reshape(-1, 2)
        q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        nq = len(q_uv)
        idx = np.zeros(max(nq, 1), np.int32); dist = np.zeros(max(nq, 1), np.uint32)
        self._check(self._L.orbx_guided_match(self._h, _vp(kp), _vp(desc), C.c_int(len(kp)), C.c_double(img_w),
                                              C.c_double(img_h), _vp(q_uv), _vp(q_desc), C.c_int(nq), C.c_double(radius),
                                              C.c_int(mode), _vp(idx), _vp(dist)))
        return idx[:nq].copy(), dist[:nq].copy()

    def solve_pnp_ransac_detailed(self, camera, points3d, points2d, prior_wc, cfg: PnPConfig = None) -> PnPResult:
        """pnp.rs:100-134 on one problem: points3d [n,3] f64 world points, points2d [n,2] (taken as f32, cv::Point2f), prior_wc
        [7] T_wc.  The pose comes back as T_wc; a problem without a model returns the prior (status in .stats)."""
        return self.solve_pnp_ransac_batch(camera, [(points3d, points2d, prior_wc)], cfg)[0]

    def solve_pnp_ransac_batch(self, camera, problems, cfg: PnPConfig = None) -> List[PnPResult]:
        """Many problems [(points3d, points2d, prior_wc), ...] in one call (one upload, one download); each result equals the
        single-problem call's byte for byte."""
        pts3d = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a, _, _ in problems]
        pts2d = [np.ascontiguousarray(b, np.float32).reshape(-1, 2) for _, b, _ in problems]
        if any(len(a) != len(b) for a, b in zip(pts3d, pts2d)):
            raise ValueError("points3d and points2d differ in length")
        P = len(problems)
        off = np.zeros(P + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in pts3d])
        N = int(off[-1])
        p3 = np.concatenate(pts3d) if N else np.zeros((1, 3), np.float64)
        p2 = np.concatenate(pts2d) if N else np.zeros((1, 2), np.float32)
        priors = np.ascontiguousarray(np.stack([np.asarray(c, np.float64).reshape(7) for _, _, c in problems]) if P else
                                      np.zeros((1, 7)), np.float64)
        poses = np.zeros((max(P, 1), 7), np.float64)
        inl = np.zeros(max(N, 1), np.uint8); err = np.zeros(max(N, 1), np.float64)
        res = np.zeros(max(P, 1), PNP_RESULT)
        c = (cfg or PnPConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_pnp_ransac_batch(self._h, C.byref(cam), C.byref(c), C.c_int(P), _vp(off), _vp(p3), _vp(p2), _vp(priors),
                                                  _vp(poses), _vp(inl), _vp(err), _vp(res)))
        return [PnPResult(poses[p].copy(), inl[off[p]:off[p + 1]].astype(bool), err[off[p]:off[p + 1]].copy(), _pnp_stats(res[p]))
                for p in range(P)]

    def solve_pnp_ransac_batch_device(self, camera, offsets, points3d, points2d, priors_wc, max_n, cfg: PnPConfig = None):
        """Device-resident batch: torch CUDA tensors offsets [P+1] int32 (ascending from 0), points3d [N,3] f64, points2d [N,2] f32,
        priors_wc [P,7] f64; max_n bounds a problem's n (larger ones get PNP_OVER_MAX_N and the prior).  Returns (poses_wc [P,7] f64,
        inlier [N] u8, err [N] f64, results [P,32] u8 — view the bytes as PNP_RESULT); asynchronous on the handle's stream."""
        import torch
        P, N = int(offsets.shape[0]) - 1, int(points3d.shape[0])
        dev = points3d.device
        poses = torch.empty((max(P, 1), 7), dtype=torch.float64, device=dev)
        inl = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
        err = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
        res = torch.empty((max(P, 1), PNP_RESULT.itemsize), dtype=torch.uint8, device=dev)
        c = (cfg or PnPConfig())._c(); cam = camera._c()
        self._after_torch(offsets, points3d, points2d, priors_wc, poses, inl, err, res)
        self._check(self._L.orbx_pnp_ransac_batch_device(self._h, C.byref(cam), C.byref(c), C.c_int(P), C.c_int(int(max_n)), _vp(offsets),
                                                         _vp(points3d), _vp(points2d), _vp(priors_wc), _vp(poses), _vp(inl), _vp(err),
                                                         _vp(res)))
        return poses[:P], inl[:N], err[:N], res[:P]

    def track_frames(self, camera, frames, cfg: "TrackConfig" = None, pnp_cfg: PnPConfig = None) -> List["TrackFrameResult"]:
        """The tracker's per-frame step (tracker.rs:863-988 mode 1, :1086-1192 mode 0) for many frames in one call, host arrays, one
        upload and one download.  frames: [(kp, desc, positions, mp_desc, search_pose_wc, prior_wc), ...] — the frame's keypoints
        (KEYPOINT) and descriptors [n,32], its map points' positions [m,3] f64 and descriptors [m,32], the pose the points are
        projected with and PnP's prior (both T_wc; mode 0 passes the predicted pose twice)."""
        B = len(frames)
        kps = [np.ascontiguousarray(f[0], KEYPOINT).reshape(-1) for f in frames]
        des = [np.ascontiguousarray(f[1], np.uint8).reshape(-1, 32) for f in frames]
        pos = [np.ascontiguousarray(f[2], np.float64).reshape(-1, 3) for f in frames]
        mds = [np.ascontiguousarray(f[3], np.uint8).reshape(-1, 32) for f in frames]
        if any(len(a) != len(b) for a, b in zip(kps, des)) or any(len(a) != len(b) for a, b in zip(pos, mds)):
            raise ValueError("keypoints / descriptors or positions / map-point descriptors differ in length")
        fo = np.zeros(B + 1, np.int32); fo[1:] = np.cumsum([len(a) for a in kps])
        mo = np.zeros(B + 1, np.int32); mo[1:] = np.cumsum([len(a) for a in pos])
        NF, M = int(fo[-1]), int(mo[-1])
        kp = np.concatenate(kps) if NF else np.zeros(1, KEYPOINT)
        de = np.concatenate(des) if NF else np.zeros((1, 32), np.uint8)
        po = np.concatenate(pos) if M else np.zeros((1, 3), np.float64)
        md = np.concatenate(mds) if M else np.zeros((1, 32), np.uint8)
        sp = np.ascontiguousarray(np.stack([np.asarray(f[4], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        pr = np.ascontiguousarray(np.stack([np.asarray(f[5], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        off = np.zeros(B + 1, np.int32)
        p3 = np.zeros((max(M, 1), 3)); p2 = np.zeros((max(M, 1), 2), np.float32)
        mi = np.zeros(max(M, 1), np.int32); fi = np.zeros(max(M, 1), np.int32)
        poses = np.zeros((max(B, 1), 7)); inl = np.zeros(max(M, 1), np.uint8); err = np.zeros(max(M, 1))
        pres = np.zeros(max(B, 1), PNP_RESULT); matched = np.zeros(max(NF, 1), np.int32); res = np.zeros(max(B, 1), TRACK_RESULT)
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_track_frames(self._h, C.byref(cam), C.byref(c), C.byref(pc), C.c_int(B), _vp(kp), _vp(de), _vp(fo), _vp(po),
                                              _vp(md), _vp(mo), _vp(sp), _vp(pr), _vp(off), _vp(p3), _vp(p2), _vp(mi), _vp(fi), _vp(poses),
                                              _vp(inl), _vp(err), _vp(pres), _vp(matched), _vp(res)))
        out = []
        for b in range(B):
            s = slice(int(off[b]), int(off[b + 1]))
            out.append(TrackFrameResult(poses[b].copy(), int(res[b]["n_inliers"]), matched[fo[b]:fo[b + 1]].copy(), err[s].copy(),
                                        inl[s].astype(bool), p3[s].copy(), p2[s].copy(), mi[s].copy(), fi[s].copy(), int(res[b]["status"]),
                                        int(res[b]["n_in_front"]), _pnp_stats(pres[b])))
        return out

    def track_frames_device(self, camera, kp, desc, feat_start, feat_count, max_feat, positions, mp_desc, mp_offsets, search_poses_wc,
                            priors_wc, cfg: "TrackConfig" = None, pnp_cfg: PnPConfig = None):
        """Device-resident form: torch CUDA tensors kp [*,7] f32 and desc [*,32] u8 as the extractor writes them, feat_start /
        feat_count [B] int32 (frame b's features are rows feat_start[b] .. + feat_count[b]; feat_count may be a strided 1-d view,
        such as the column of the extractor's counts that track_feature_slots returns: the kernels read it where it lies, on the
        handle's stream, behind the extraction), positions [M,3] f64, mp_desc [M,32] u8, search_poses_wc / priors_wc [B,7] f64; mp_offsets [B+1] is a
        host array (ascending from 0); max_feat bounds a frame's count.  Returns a dict of tensors: offsets [B+1] int32, points3d
        [M,3] f64, points2d [M,2] f32, mp_idx / feat_idx [M] int32, poses [B,7] f64, inlier [M] u8, err [M] f64, pnp_results [B,32] u8
        (PNP_RESULT), matched [B,max_feat] int32, results [B,16] u8 (TRACK_RESULT).  offsets / points3d / points2d / poses feed
        pose_inertial_optimization_batch_device unchanged.  Asynchronous on the handle's stream."""
        import torch
        mo = np.ascontiguousarray(mp_offsets, np.int32).reshape(-1)
        B, M = len(mo) - 1, int(mo[-1]) if len(mo) else 0
        dev = search_poses_wc.device
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(offsets=mk(max(B, 0) + 1, torch.int32), points3d=mk((max(M, 1), 3), torch.float64), points2d=mk((max(M, 1), 2), torch.float32),
                 mp_idx=mk(max(M, 1), torch.int32), feat_idx=mk(max(M, 1), torch.int32), poses=mk((max(B, 1), 7), torch.float64),
                 inlier=mk(max(M, 1), torch.uint8), err=mk(max(M, 1), torch.float64), pnp_results=mk((max(B, 1), PNP_RESULT.itemsize), torch.uint8),
                 matched=mk((max(B, 1), max(int(max_feat), 1)), torch.int32), results=mk((max(B, 1), TRACK_RESULT.itemsize), torch.uint8))
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        ins = (kp, desc, feat_start, feat_count, positions, mp_desc, search_poses_wc, priors_wc)
        self._after_torch(*ins, *o.values())
        self._check(self._L.orbx_track_frames_device(
            self._h, C.byref(cam), C.byref(c), C.byref(pc), C.c_int(B), _vp(kp), _vp(desc), _vp(feat_start), _vp(feat_count), C.c_int(fc_stride), C.c_int(int(max_feat)),
            _vp(positions), _vp(mp_desc), _vp(mo), _vp(search_poses_wc), _vp(priors_wc), _vp(o["offsets"]), _vp(o["points3d"]), _vp(o["points2d"]),
            _vp(o["mp_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]), _vp(o["err"]), _vp(o["pnp_results"]), _vp(o["matched"]),
            _vp(o["results"])))
        o["matched"] = o["matched"][:, :int(max_feat)]
        for k in ("points3d", "points2d", "mp_idx", "feat_idx", "inlier", "err"):
            o[k] = o[k][:M]
        return o

    @staticmethod
    def track_feature_slots(out, batch=None, side=0):
        """feat_start / feat_count for track_frames_device from an alloc_batch_outputs() dict: frame b is the left (side 0) or right
        (side 1) image of pair b; its slot starts at row (2 b + side) * cap_kp of out['kp'].view(-1, 7) / out['desc'].view(-1, 32).
        feat_count is out['nkp'][:batch, side] itself — a strided view of the extractor's device-side counts, not a copy: nothing
        is read here, so it may be taken before or after process_stereo_batch_device is enqueued, and track_frames_device's kernels
        read the counts on the handle's stream behind the extraction.  feat_start does not depend on the frame and can be kept.
        max_feat = out['cap_kp']."""
        import torch
        b = batch or out["batch"]
        start = (torch.arange(b, dtype=torch.int32, device=out["nkp"].device) * 2 + side) * out["cap_kp"]
        return start, out["nkp"][:b, side]

    def track_reference(self, camera, frames, min_correspondences=4, pnp_cfg: PnPConfig = None) -> List["TrackReferenceResult"]:
        """track_with_reference_kf (tracker.rs:992-1064) for many frames in one call, host arrays, one upload and one download.
        frames: [(kp, desc, kf_desc, kf_positions, kf_valid, prior_wc), ...] — the frame's keypoints (KEYPOINT) and descriptors [n,32];
        its reference keyframe's descriptors [m,32], per keyframe feature the map point's position [m,3] f64 and a validity byte [m]
        (1: the feature has a map point the map still holds); PnP's prior (T_wc, self.pose)."""
        B = len(frames)
        kps = [np.ascontiguousarray(f[0], KEYPOINT).reshape(-1) for f in frames]
        des = [np.ascontiguousarray(f[1], np.uint8).reshape(-1, 32) for f in frames]
        kds = [np.ascontiguousarray(f[2], np.uint8).reshape(-1, 32) for f in frames]
        pos = [np.ascontiguousarray(f[3], np.float64).reshape(-1, 3) for f in frames]
        val = [np.ascontiguousarray(f[4], np.uint8).reshape(-1) for f in frames]
        if any(len(a) != len(b) for a, b in zip(kps, des)) or any(not (len(a) == len(b) == len(c)) for a, b, c in zip(kds, pos, val)):
            raise ValueError("keypoints / descriptors or keyframe descriptors / positions / valid differ in length")
        fo = np.zeros(B + 1, np.int32); fo[1:] = np.cumsum([len(a) for a in kps])
        ko = np.zeros(B + 1, np.int32); ko[1:] = np.cumsum([len(a) for a in kds])
        NF, K = int(fo[-1]), int(ko[-1])
        kp = np.concatenate(kps) if NF else np.zeros(1, KEYPOINT)
        de = np.concatenate(des) if NF else np.zeros((1, 32), np.uint8)
        kd = np.concatenate(kds) if K else np.zeros((1, 32), np.uint8)
        po = np.concatenate(pos) if K else np.zeros((1, 3), np.float64)
        va = np.concatenate(val) if K else np.zeros(1, np.uint8)
        pr = np.ascontiguousarray(np.stack([np.asarray(f[5], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        Kz, Bz = max(K, 1), max(B, 1)
        ma = np.zeros(Kz, DMATCH); off = np.zeros(B + 1, np.int32); p3 = np.zeros((Kz, 3)); p2 = np.zeros((Kz, 2), np.float32)
        ki = np.zeros(Kz, np.int32); fi = np.zeros(Kz, np.int32); poses = np.zeros((Bz, 7)); inl = np.zeros(Kz, np.uint8); err = np.zeros(Kz)
        pres = np.zeros(Bz, PNP_RESULT); res = np.zeros(Bz, TRACK_REF_RESULT)
        pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_track_reference(self._h, C.byref(cam), C.byref(pc), C.c_int(int(min_correspondences)), C.c_int(B), _vp(kp), _vp(de),
                                                 _vp(fo), _vp(kd), _vp(po), _vp(va), _vp(ko), _vp(pr), _vp(ma), _vp(off), _vp(p3), _vp(p2), _vp(ki),
                                                 _vp(fi), _vp(poses), _vp(inl), _vp(err), _vp(pres), _vp(res)))
        out = []
        for b in range(B):
            s = slice(int(off[b]), int(off[b + 1]))
            out.append(TrackReferenceResult(poses[b].copy(), int(res[b]["n_inliers"]), ma[ko[b]:ko[b] + int(res[b]["n_matches"])].copy(), err[s].copy(),
                                            inl[s].astype(bool), p3[s].copy(), p2[s].copy(), ki[s].copy(), fi[s].copy(), int(res[b]["status"]),
                                            _pnp_stats(pres[b])))
        return out

    def _track_reference_outputs(self, B, K, dev):
        import torch
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        Kz, Bz = max(K, 1), max(B, 1)
        return dict(matches=mk((Kz, DMATCH.itemsize), torch.uint8), offsets=mk(max(B, 0) + 1, torch.int32), points3d=mk((Kz, 3), torch.float64),
                    points2d=mk((Kz, 2), torch.float32), kf_idx=mk(Kz, torch.int32), feat_idx=mk(Kz, torch.int32), poses=mk((Bz, 7), torch.float64),
                    inlier=mk(Kz, torch.uint8), err=mk(Kz, torch.float64), pnp_results=mk((Bz, PNP_RESULT.itemsize), torch.uint8),
                    results=mk((Bz, TRACK_REF_RESULT.itemsize), torch.uint8))

    @staticmethod
    def _feat_count_stride(feat_count, B):
        import torch
        if feat_count.dim() != 1 or feat_count.dtype != torch.int32 or (B > 1 and feat_count.stride(0) < 1):
            raise ValueError("feat_count must be a 1-d int32 tensor or view with a positive stride")
        return int(feat_count.stride(0)) if B > 1 else 1

    def track_reference_device(self, camera, kp, desc, feat_start, feat_count, max_feat, kf_desc, kf_positions, kf_valid, kf_offsets, priors_wc,
                               min_correspondences=4, pnp_cfg: PnPConfig = None):
        """Device-resident form: torch CUDA tensors kp [*,7] f32 / desc [*,32] u8 / feat_start / feat_count [B] int32 / max_feat as
        track_frames_device (feat_count may be the strided view track_feature_slots returns); the reference keyframes packed: kf_desc
        [K,32] u8, kf_positions [K,3] f64, kf_valid [K] u8, frame b's keyframe owning rows kf_offsets[b] .. kf_offsets[b+1] (a host
        array, ascending from 0); priors_wc [B,7] f64.  Returns a dict of tensors: matches [K,16] u8 (DMATCH; frame b's from row
        kf_offsets[b], results n_matches of them), offsets [B+1] int32, points3d [K,3] f64, points2d [K,2] f32, kf_idx / feat_idx [K]
        int32, poses [B,7] f64, inlier [K] u8, err [K] f64, pnp_results [B,32] u8 (PNP_RESULT), results [B,16] u8 (TRACK_REF_RESULT).
        offsets / points3d / points2d / poses feed pose_inertial_optimization_batch_device unchanged.  Asynchronous on the handle's
        stream."""
        ko = np.ascontiguousarray(kf_offsets, np.int32).reshape(-1)
        B, K = len(ko) - 1, int(ko[-1]) if len(ko) else 0
        o = self._track_reference_outputs(B, K, priors_wc.device)
        pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        self._after_torch(kp, desc, feat_start, feat_count, kf_desc, kf_positions, kf_valid, priors_wc, *o.values())
        self._check(self._L.orbx_track_reference_device(
            self._h, C.byref(cam), C.byref(pc), C.c_int(int(min_correspondences)), C.c_int(B), _vp(kp), _vp(desc), _vp(feat_start), _vp(feat_count),
            C.c_int(fc_stride), C.c_int(int(max_feat)), _vp(kf_desc), _vp(kf_positions), _vp(kf_valid), _vp(ko), _vp(priors_wc), _vp(o["matches"]),
            _vp(o["offsets"]), _vp(o["points3d"]), _vp(o["points2d"]), _vp(o["kf_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]),
            _vp(o["err"]), _vp(o["pnp_results"]), _vp(o["results"])))
        for k in ("matches", "points3d", "points2d", "kf_idx", "feat_idx", "inlier", "err"):
            o[k] = o[k][:K]
        return o

    def keyframe_track_reference(self, camera, keyframes, kp, desc, feat_start, feat_count, max_feat, kf_positions, kf_valid, priors_wc,
                                 min_correspondences=4, pnp_cfg: PnPConfig = None):
        """track_reference_device against resident keyframes: frame b is matched against keyframes[b] (KeyFrame; one may be listed
        several times), whose descriptors are read where they lie.  kf_positions / kf_valid are HOST arrays, one [n_b,3] f64 / [n_b] u8
        pair per frame in a list (n_b = the keyframe's feature count); they travel in the call's one upload.  Frames, priors_wc and
        the returned dict as track_reference_device."""
        B = len(keyframes)
        pos = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in kf_positions]
        val = [np.ascontiguousarray(a, np.uint8).reshape(-1) for a in kf_valid]
        if len(pos) != B or len(val) != B or any(len(a) != len(b) for a, b in zip(pos, val)):
            raise ValueError("one positions / valid pair per keyframe, of equal length")
        ko = np.zeros(B + 1, np.int32); ko[1:] = np.cumsum([len(a) for a in pos])
        K = int(ko[-1])
        po = np.concatenate(pos) if K else np.zeros((1, 3), np.float64)
        va = np.concatenate(val) if K else np.zeros(1, np.uint8)
        arr = (C.c_void_p * max(B, 1))(*[k._p for k in keyframes])
        o = self._track_reference_outputs(B, K, priors_wc.device)
        pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        self._after_torch(kp, desc, feat_start, feat_count, priors_wc, *o.values())
        self._check(self._L.orbx_keyframe_track_reference(
            self._h, C.byref(cam), C.byref(pc), C.c_int(int(min_correspondences)), C.c_int(B), arr, _vp(kp), _vp(desc), _vp(feat_start), _vp(feat_count),
            C.c_int(fc_stride), C.c_int(int(max_feat)), _vp(po), _vp(va), _vp(ko), _vp(priors_wc), _vp(o["matches"]), _vp(o["offsets"]),
            _vp(o["points3d"]), _vp(o["points2d"]), _vp(o["kf_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]), _vp(o["err"]),
            _vp(o["pnp_results"]), _vp(o["results"])))
        for k in ("matches", "points3d", "points2d", "kf_idx", "feat_idx", "inlier", "err"):
            o[k] = o[k][:K]
        return o

    # ---- resident map points (include/orbx.h, "resident map points") ----
    def _map_source(self, mp, keyframes, src_slots, src_offsets):
        """The source arguments of the orbx_map_* calls and the host-known bound of every frame's list: keyframes = one list of
        KeyFrame per frame (MAP_SOURCE_KEYFRAMES), or src_slots (int32, one array of all frames' entries) with src_offsets [B+1]
        (MAP_SOURCE_SLOTS).  -> (source, kfs, kf_offsets, src_slots, src_offsets, bounds [B], keep-alive)"""
        if (keyframes is None) == (src_slots is None):
            raise ValueError("give keyframes (one list per frame) or src_slots with src_offsets")
        if keyframes is not None:
            flat = [k for ks in keyframes for k in ks]
            ko = np.zeros(len(keyframes) + 1, np.int32); ko[1:] = np.cumsum([len(ks) for ks in keyframes])
            arr = (C.c_void_p * max(len(flat), 1))(*[k._p for k in flat])
            bounds = [min(sum(k.n for k in ks), mp.capacity) for ks in keyframes]
            return MAP_SOURCE_KEYFRAMES, arr, _vp(ko), None, None, bounds, (arr, ko)
        so = np.ascontiguousarray(src_offsets, np.int32).reshape(-1)
        return MAP_SOURCE_SLOTS, None, None, _vp(src_slots), _vp(so), [int(x) for x in np.diff(so)], (so, src_slots)

    def _map_list_outputs(self, B, cap, dev):
        import torch
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        return dict(list_offsets=mk(max(B, 0) + 1, torch.int32), list_slot=mk(max(cap, 1), torch.int32), positions=mk((max(cap, 1), 3), torch.float64),
                    mp_desc=mk((max(cap, 1), 32), torch.uint8))

    def map_select_points_device(self, mp: "MapPointStore", keyframes=None, src_slots=None, src_offsets=None, device=None):
        """Every frame's list of map points from the resident store, made on the device (orbx_map_select_points_device): the distinct
        live slots of the frame's keyframes in first-seen order (keyframes: one list of KeyFrame per frame), or the live entries of
        the frame's slot array in order, repeats kept (src_slots: an int32 CUDA tensor, src_offsets: host [B+1]).  Returns a dict of
        tensors: list_offsets [B+1] int32, list_slot [cap] int32, positions [cap,3] f64, mp_desc [cap,32] u8, cap = the sum of the
        frames' bounds; rows [0, list_offsets[B]) are written.  Asynchronous on the handle's stream."""
        import torch
        src, kfs, ko, ss, so, bounds, keep = self._map_source(mp, keyframes, src_slots, src_offsets)
        B, cap = len(bounds), int(sum(bounds))
        dev = device or (src_slots.device if src_slots is not None else torch.device("cuda", self.device))
        o = self._map_list_outputs(B, cap, dev)
        self._after_torch(*([src_slots] if src_slots is not None else []), *o.values())
        self._check(self._L.orbx_map_select_points_device(self._h, mp._p, C.c_int(src), C.c_int(B), kfs, ko, ss, so, C.c_int(cap), _vp(o["list_offsets"]),
                                                          _vp(o["list_slot"]), _vp(o["positions"]), _vp(o["mp_desc"])))
        return o

    def map_track_frames_device(self, camera, mp: "MapPointStore", kp, desc, feat_start, feat_count, max_feat, search_poses_wc, priors_wc,
                                keyframes=None, src_slots=None, src_offsets=None, cfg: "TrackConfig" = None, pnp_cfg: PnPConfig = None):
        """track_frames_device with the map points taken from the resident store: the selection of map_select_points_device, then the
        tracker's launches on the lists where they lie.  Frames, poses and configurations as track_frames_device; the source as
        map_select_points_device.  Returns that call's dict (arrays sized by the lists' bound instead of M) plus list_offsets,
        list_slot, positions, mp_desc and matched_slot [B,max_feat] int32: matched mapped through the list to slots, -1 = none —
        matched_slot.view(-1) with src_offsets = arange(B+1) * max_feat is the next frame's slot source."""
        import torch
        src, kfs, ko, ss, so, bounds, keep = self._map_source(mp, keyframes, src_slots, src_offsets)
        B, M = len(bounds), int(sum(bounds))
        dev = search_poses_wc.device
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(offsets=mk(max(B, 0) + 1, torch.int32), points3d=mk((max(M, 1), 3), torch.float64), points2d=mk((max(M, 1), 2), torch.float32),
                 mp_idx=mk(max(M, 1), torch.int32), feat_idx=mk(max(M, 1), torch.int32), poses=mk((max(B, 1), 7), torch.float64),
                 inlier=mk(max(M, 1), torch.uint8), err=mk(max(M, 1), torch.float64), pnp_results=mk((max(B, 1), PNP_RESULT.itemsize), torch.uint8),
                 matched=mk((max(B, 1), max(int(max_feat), 1)), torch.int32), matched_slot=mk((max(B, 1), max(int(max_feat), 1)), torch.int32),
                 results=mk((max(B, 1), TRACK_RESULT.itemsize), torch.uint8))
        o.update(self._map_list_outputs(B, M, dev))
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        self._after_torch(kp, desc, feat_start, feat_count, search_poses_wc, priors_wc, *([src_slots] if src_slots is not None else []), *o.values())
        self._check(self._L.orbx_map_track_frames_device(
            self._h, C.byref(cam), C.byref(c), C.byref(pc), mp._p, C.c_int(src), C.c_int(B), kfs, ko, ss, so, _vp(kp), _vp(desc), _vp(feat_start),
            _vp(feat_count), C.c_int(fc_stride), C.c_int(int(max_feat)), _vp(search_poses_wc), _vp(priors_wc), C.c_int(M), _vp(o["list_offsets"]),
            _vp(o["list_slot"]), _vp(o["positions"]), _vp(o["mp_desc"]), _vp(o["offsets"]), _vp(o["points3d"]), _vp(o["points2d"]), _vp(o["mp_idx"]),
            _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]), _vp(o["err"]), _vp(o["pnp_results"]), _vp(o["matched"]), _vp(o["matched_slot"]),
            _vp(o["results"])))
        o["matched"] = o["matched"][:, :int(max_feat)]; o["matched_slot"] = o["matched_slot"][:, :int(max_feat)]
        for k in ("points3d", "points2d", "mp_idx", "feat_idx", "inlier", "err", "list_slot", "positions", "mp_desc"):
            o[k] = o[k][:M]
        return o

    def map_track_frames(self, camera, mp: "MapPointStore", frames, keyframes=None, src_slots=None, cfg: "TrackConfig" = None,
                         pnp_cfg: PnPConfig = None):
        """The host form (orbx_map_track_frames): frames = [(kp, desc, search_pose_wc, prior_wc), ...] in host arrays; the source is
        keyframes (one list of KeyFrame per frame) or src_slots (one host int32 array per frame).  One upload, one download.
        Returns [(TrackFrameResult, list_slot, matched_slot), ...]: the frame's result as track_frames gives it (mp_idx and matched
        index the frame's list), the list's slots and matched as slots."""
        B = len(frames)
        so = None
        if src_slots is not None:
            parts = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in src_slots]
            so = np.zeros(B + 1, np.int32); so[1:] = np.cumsum([len(a) for a in parts])
            src_slots = np.concatenate(parts + [np.zeros(1, np.int32)])
        src, kfs, ko, ss, so_p, bounds, keep = self._map_source(mp, keyframes, src_slots, so)
        if len(bounds) != B:
            raise ValueError("one source per frame")
        kps = [np.ascontiguousarray(f[0], KEYPOINT).reshape(-1) for f in frames]
        des = [np.ascontiguousarray(f[1], np.uint8).reshape(-1, 32) for f in frames]
        if any(len(a) != len(b) for a, b in zip(kps, des)):
            raise ValueError("keypoints / descriptors differ in length")
        fo = np.zeros(B + 1, np.int32); fo[1:] = np.cumsum([len(a) for a in kps])
        NF, M = int(fo[-1]), int(sum(bounds))
        kp = np.concatenate(kps) if NF else np.zeros(1, KEYPOINT)
        de = np.concatenate(des) if NF else np.zeros((1, 32), np.uint8)
        sp = np.ascontiguousarray(np.stack([np.asarray(f[2], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        pr = np.ascontiguousarray(np.stack([np.asarray(f[3], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        Mz, Bz = max(M, 1), max(B, 1)
        lo = np.zeros(B + 1, np.int32); ls = np.zeros(Mz, np.int32); off = np.zeros(B + 1, np.int32)
        p3 = np.zeros((Mz, 3)); p2 = np.zeros((Mz, 2), np.float32); mi = np.zeros(Mz, np.int32); fi = np.zeros(Mz, np.int32)
        poses = np.zeros((Bz, 7)); inl = np.zeros(Mz, np.uint8); err = np.zeros(Mz)
        pres = np.zeros(Bz, PNP_RESULT); matched = np.zeros(max(NF, 1), np.int32); mslot = np.zeros(max(NF, 1), np.int32); res = np.zeros(Bz, TRACK_RESULT)
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_map_track_frames(
            self._h, C.byref(cam), C.byref(c), C.byref(pc), mp._p, C.c_int(src), C.c_int(B), kfs, ko, ss, so_p, _vp(kp), _vp(de), _vp(fo), _vp(sp), _vp(pr),
            C.c_int(M), _vp(lo), _vp(ls), _vp(off), _vp(p3), _vp(p2), _vp(mi), _vp(fi), _vp(poses), _vp(inl), _vp(err), _vp(pres), _vp(matched), _vp(mslot),
            _vp(res)))
        out = []
        for b in range(B):
            s = slice(int(off[b]), int(off[b + 1]))
            t = TrackFrameResult(poses[b].copy(), int(res[b]["n_inliers"]), matched[fo[b]:fo[b + 1]].copy(), err[s].copy(), inl[s].astype(bool), p3[s].copy(),
                                 p2[s].copy(), mi[s].copy(), fi[s].copy(), int(res[b]["status"]), int(res[b]["n_in_front"]), _pnp_stats(pres[b]))
            out.append((t, ls[lo[b]:lo[b + 1]].copy(), mslot[fo[b]:fo[b + 1]].copy()))
        return out

    def map_track_reference_device(self, camera, mp: "MapPointStore", keyframes, kp, desc, feat_start, feat_count, max_feat, priors_wc,
                                   min_correspondences=4, pnp_cfg: PnPConfig = None):
        """keyframe_track_reference with kf_positions / kf_valid made on the device from every keyframe's slot table and the store
        (valid = the feature has a slot and the slot is live; positions = that slot's, else zeros).  Returns that call's dict plus
        kf_positions [K,3] f64 and kf_valid [K] u8 as the kernels read them."""
        import torch
        B = len(keyframes)
        K = int(sum(k.n for k in keyframes))
        arr = (C.c_void_p * max(B, 1))(*[k._p for k in keyframes])
        o = self._track_reference_outputs(B, K, priors_wc.device)
        o["kf_positions"] = torch.empty((max(K, 1), 3), dtype=torch.float64, device=priors_wc.device)
        o["kf_valid"] = torch.empty(max(K, 1), dtype=torch.uint8, device=priors_wc.device)
        pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        self._after_torch(kp, desc, feat_start, feat_count, priors_wc, *o.values())
        self._check(self._L.orbx_map_track_reference_device(
            self._h, C.byref(cam), C.byref(pc), C.c_int(int(min_correspondences)), mp._p, C.c_int(B), arr, _vp(kp), _vp(desc), _vp(feat_start),
            _vp(feat_count), C.c_int(fc_stride), C.c_int(int(max_feat)), _vp(priors_wc), _vp(o["kf_positions"]), _vp(o["kf_valid"]), _vp(o["matches"]),
            _vp(o["offsets"]), _vp(o["points3d"]), _vp(o["points2d"]), _vp(o["kf_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]),
            _vp(o["err"]), _vp(o["pnp_results"]), _vp(o["results"])))
        for k in ("matches", "points3d", "points2d", "kf_idx", "feat_idx", "inlier", "err", "kf_positions", "kf_valid"):
            o[k] = o[k][:K]
        return o

    # ---- covisibility from the resident map (include/orbx.h, "covisibility from the resident map") ----
    @staticmethod
    def _kf_array(keyframes):
        return (C.c_void_p * max(len(keyframes), 1))(*[k._p for k in keyframes])

    @staticmethod
    def _local_bounds(mp, keyframes, ref_kf, n_best):
        """per frame the host-known bound of its list: the reference keyframe's feature count plus the n_best largest of the
        others', every keyframe's where the reference is -1, at most the capacity"""
        ns = np.array([k.n for k in keyframes], np.int64)
        K = len(ns)
        order = np.argsort(-ns, kind="stable")
        place = np.empty(K, np.int64); place[order] = np.arange(K)
        top = np.concatenate([[0], np.cumsum(ns[order])])                  # top[i]: the i largest feature counts summed
        nb = min(max(n_best, 0), max(K - 1, 0))
        out = []
        for r in ref_kf:
            c = top[K] if r < 0 or r >= K else (top[nb + 1] if place[r] < nb else top[nb] + ns[r])
            out.append(int(min(c, mp.capacity)))
        return out

    def map_covisibility_device(self, mp: "MapPointStore", keyframes, queries, n_best=0, weights=True, device=None):
        """Covisibility weights and best neighbours of keyframes[q] for q in queries (indices into `keyframes`, a list of KeyFrame),
        counted on the device from the slot tables and the store's live bytes (orbx_map_covisibility_device).  Returns a dict of
        CUDA tensors: weights [Q,n_kfs] int32 (absent with weights=False), and with n_best > 0 best [Q,n_best] int32 (indices into
        `keyframes`, weight descending then index ascending, -1 padded) and n_best [Q] int32.  Asynchronous on the handle's stream."""
        import torch
        q = np.ascontiguousarray(queries, np.int32).reshape(-1)
        Q, K, nb = len(q), len(keyframes), int(n_best)
        dev = device or torch.device("cuda", self.device)
        o = {}
        if weights:
            o["weights"] = torch.zeros((Q, K), dtype=torch.int32, device=dev)
        if nb > 0:
            o["best"] = torch.full((Q, nb), -1, dtype=torch.int32, device=dev)
            o["n_best"] = torch.zeros(Q, dtype=torch.int32, device=dev)
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_covisibility_device(self._h, mp._p, C.c_int(K), self._kf_array(keyframes), C.c_int(Q), _vp(q if Q else np.zeros(1, np.int32)),
                                                         C.c_int(nb), _vp(o.get("weights")), _vp(o.get("best")), _vp(o.get("n_best"))))
        return o

    def map_covisibility(self, mp: "MapPointStore", keyframes, queries, n_best=0):
        """The host form (orbx_map_covisibility), synchronous: (weights [Q,n_kfs] int32, best [Q,n_best] int32, n_best [Q] int32)
        as numpy arrays."""
        q = np.ascontiguousarray(queries, np.int32).reshape(-1)
        Q, K, nb = len(q), len(keyframes), int(n_best)
        w = np.zeros((Q, K), np.int32); best = np.full((Q, max(nb, 0)), -1, np.int32); cnt = np.zeros(Q, np.int32)
        self._check(self._L.orbx_map_covisibility(self._h, mp._p, C.c_int(K), self._kf_array(keyframes), C.c_int(Q), _vp(q if Q else np.zeros(1, np.int32)),
                                                  C.c_int(nb), _vp(w) if w.size else None, _vp(best) if best.size else None, _vp(cnt) if Q else None))
        return w, best, cnt

    def map_track_local_device(self, camera, mp: "MapPointStore", keyframes, ref_kf, n_best, kp, desc, feat_start, feat_count, max_feat, search_poses_wc,
                               priors_wc, cfg: "TrackConfig" = None, pnp_cfg: PnPConfig = None):
        """map_track_frames_device with every frame's keyframe list chosen on the device (orbx_map_track_local_device): frame b's
        list is [ref_kf[b]] + its n_best best covisibles among `keyframes` (a list of KeyFrame; ref_kf holds indices into it), or
        all of `keyframes` where ref_kf[b] is -1.  Returns map_track_frames_device's dict plus local_kf [B,1+n_best] int32: the
        keyframes chosen, -1 padded (all -1 for ref_kf[b] = -1)."""
        import torch
        ref = np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
        B, nb = len(ref), int(n_best)
        bounds = self._local_bounds(mp, keyframes, ref.tolist(), nb)
        M = int(sum(bounds))
        dev = search_poses_wc.device
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(offsets=mk(max(B, 0) + 1, torch.int32), points3d=mk((max(M, 1), 3), torch.float64), points2d=mk((max(M, 1), 2), torch.float32),
                 mp_idx=mk(max(M, 1), torch.int32), feat_idx=mk(max(M, 1), torch.int32), poses=mk((max(B, 1), 7), torch.float64),
                 inlier=mk(max(M, 1), torch.uint8), err=mk(max(M, 1), torch.float64), pnp_results=mk((max(B, 1), PNP_RESULT.itemsize), torch.uint8),
                 matched=mk((max(B, 1), max(int(max_feat), 1)), torch.int32), matched_slot=mk((max(B, 1), max(int(max_feat), 1)), torch.int32),
                 results=mk((max(B, 1), TRACK_RESULT.itemsize), torch.uint8), local_kf=mk((max(B, 1), 1 + max(nb, 0)), torch.int32))
        o.update(self._map_list_outputs(B, M, dev))
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        fc_stride = self._feat_count_stride(feat_count, B)
        self._after_torch(kp, desc, feat_start, feat_count, search_poses_wc, priors_wc, *o.values())
        self._check(self._L.orbx_map_track_local_device(
            self._h, C.byref(cam), C.byref(c), C.byref(pc), mp._p, C.c_int(B), C.c_int(len(keyframes)), self._kf_array(keyframes),
            _vp(ref if B else np.zeros(1, np.int32)), C.c_int(nb), _vp(kp), _vp(desc), _vp(feat_start), _vp(feat_count), C.c_int(fc_stride), C.c_int(int(max_feat)),
            _vp(search_poses_wc), _vp(priors_wc), C.c_int(M), _vp(o["local_kf"]), _vp(o["list_offsets"]), _vp(o["list_slot"]), _vp(o["positions"]),
            _vp(o["mp_desc"]), _vp(o["offsets"]), _vp(o["points3d"]), _vp(o["points2d"]), _vp(o["mp_idx"]), _vp(o["feat_idx"]), _vp(o["poses"]), _vp(o["inlier"]),
            _vp(o["err"]), _vp(o["pnp_results"]), _vp(o["matched"]), _vp(o["matched_slot"]), _vp(o["results"])))
        o["matched"] = o["matched"][:, :int(max_feat)]; o["matched_slot"] = o["matched_slot"][:, :int(max_feat)]
        for k in ("points3d", "points2d", "mp_idx", "feat_idx", "inlier", "err", "list_slot", "positions", "mp_desc"):
            o[k] = o[k][:M]
        return o

    def map_track_local(self, camera, mp: "MapPointStore", frames, keyframes, ref_kf, n_best, cfg: "TrackConfig" = None, pnp_cfg: PnPConfig = None):
        """The host form (orbx_map_track_local): frames = [(kp, desc, search_pose_wc, prior_wc), ...] in host arrays, keyframes /
        ref_kf / n_best as map_track_local_device.  One upload, one download.  Returns [(TrackFrameResult, list_slot, matched_slot,
        local_kf [1+n_best]), ...]."""
        B, nb = len(frames), int(n_best)
        ref = np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
        if len(ref) != B:
            raise ValueError("one reference keyframe index per frame")
        bounds = self._local_bounds(mp, keyframes, ref.tolist(), nb)
        kps = [np.ascontiguousarray(f[0], KEYPOINT).reshape(-1) for f in frames]
        des = [np.ascontiguousarray(f[1], np.uint8).reshape(-1, 32) for f in frames]
        if any(len(a) != len(b) for a, b in zip(kps, des)):
            raise ValueError("keypoints / descriptors differ in length")
        fo = np.zeros(B + 1, np.int32); fo[1:] = np.cumsum([len(a) for a in kps])
        NF, M = int(fo[-1]), int(sum(bounds))
        kp = np.concatenate(kps) if NF else np.zeros(1, KEYPOINT)
        de = np.concatenate(des) if NF else np.zeros((1, 32), np.uint8)
        sp = np.ascontiguousarray(np.stack([np.asarray(f[2], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        pr = np.ascontiguousarray(np.stack([np.asarray(f[3], np.float64).reshape(7) for f in frames]) if B else np.zeros((1, 7)), np.float64)
        Mz, Bz = max(M, 1), max(B, 1)
        lo = np.zeros(B + 1, np.int32); ls = np.zeros(Mz, np.int32); off = np.zeros(B + 1, np.int32); lk = np.full((Bz, 1 + max(nb, 0)), -1, np.int32)
        p3 = np.zeros((Mz, 3)); p2 = np.zeros((Mz, 2), np.float32); mi = np.zeros(Mz, np.int32); fi = np.zeros(Mz, np.int32)
        poses = np.zeros((Bz, 7)); inl = np.zeros(Mz, np.uint8); err = np.zeros(Mz)
        pres = np.zeros(Bz, PNP_RESULT); matched = np.zeros(max(NF, 1), np.int32); mslot = np.zeros(max(NF, 1), np.int32); res = np.zeros(Bz, TRACK_RESULT)
        c = (cfg or TrackConfig())._c(); pc = (pnp_cfg or PnPConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_map_track_local(
            self._h, C.byref(cam), C.byref(c), C.byref(pc), mp._p, C.c_int(B), C.c_int(len(keyframes)), self._kf_array(keyframes),
            _vp(ref if B else np.zeros(1, np.int32)), C.c_int(nb), _vp(kp), _vp(de), _vp(fo), _vp(sp), _vp(pr), C.c_int(M), _vp(lk), _vp(lo), _vp(ls), _vp(off),
            _vp(p3), _vp(p2), _vp(mi), _vp(fi), _vp(poses), _vp(inl), _vp(err), _vp(pres), _vp(matched), _vp(mslot), _vp(res)))
        out = []
        for b in range(B):
            s = slice(int(off[b]), int(off[b + 1]))
            t = TrackFrameResult(poses[b].copy(), int(res[b]["n_inliers"]), matched[fo[b]:fo[b + 1]].copy(), err[s].copy(), inl[s].astype(bool), p3[s].copy(),
                                 p2[s].copy(), mi[s].copy(), fi[s].copy(), int(res[b]["status"]), int(res[b]["n_in_front"]), _pnp_stats(pres[b]))
            out.append((t, ls[lo[b]:lo[b + 1]].copy(), mslot[fo[b]:fo[b + 1]].copy(), lk[b].copy()))
        return out

    # ---- local BA from the resident map (include/orbx.h, "local BA from the resident map") ----
    def _ba_window_bounds(self, mp, keyframes, cur, max_covisible):
        """(list bound, observation bound) of a collection call: map_track_local_device's bound for one frame with reference
        `cur`, and every feature of `keyframes`"""
        return self._local_bounds(mp, keyframes, [int(cur)], int(max_covisible))[0], int(sum(k.n for k in keyframes))

    def map_collect_ba_window_device(self, mp: "MapPointStore", keyframes, cur, max_covisible, device=None):
        """The local-BA window of keyframes[cur], collected on the device from the slot tables, the keypoints and the store
        (orbx_map_collect_ba_window_device).  Returns a dict of CUDA tensors: counts [4] int32 = (K, F, M, N), local_kf
        [1+max_covisible] int32 (-1 padded; [0] is the anchor, [1:1+K] the optimised keyframes), fixed_kf [n_kfs] int32 (the F-1
        other observers, ascending, then -1), list_slot [cap] int32 and positions [cap,3] f64 (the window's points, rows [0, M)),
        obs32 [obs_cap,16] u8 (rows [0, N) are BA_OBS32 records).  Every index is a position in `keyframes`.  Asynchronous on the
        handle's stream."""
        import torch
        cap, ocap = self._ba_window_bounds(mp, keyframes, cur, max_covisible)
        dev = device or torch.device("cuda", self.device)
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(counts=mk(4, torch.int32), local_kf=mk(1 + max(int(max_covisible), 0), torch.int32), fixed_kf=mk(max(len(keyframes), 1), torch.int32),
                 list_slot=mk(max(cap, 1), torch.int32), positions=mk((max(cap, 1), 3), torch.float64), obs32=mk((max(ocap, 1), BA_OBS32.itemsize), torch.uint8))
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_collect_ba_window_device(
            self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(int(cur)), C.c_int(int(max_covisible)), C.c_int(cap), C.c_int(ocap),
            _vp(o["counts"]), _vp(o["local_kf"]), _vp(o["fixed_kf"]), _vp(o["list_slot"]), _vp(o["positions"]), _vp(o["obs32"])))
        o["fixed_kf"] = o["fixed_kf"][:len(keyframes)]; o["list_slot"] = o["list_slot"][:cap]; o["positions"] = o["positions"][:cap]; o["obs32"] = o["obs32"][:ocap]
        return o

    def map_collect_ba_window(self, mp: "MapPointStore", keyframes, cur, max_covisible):
        """The host form (orbx_map_collect_ba_window), synchronous: a dict of numpy arrays cut to their sizes — counts [4],
        local_kf [1+max_covisible], fixed_kf [F-1], list_slot [M], positions [M,3], obs32 [N] BA_OBS32 — or None where the window
        is empty (the reference's None, local_ba_lm.rs:813-815, :884-886)."""
        cap, ocap = self._ba_window_bounds(mp, keyframes, cur, max_covisible)
        counts = np.zeros(4, np.int32); lk = np.full(1 + max(int(max_covisible), 0), -1, np.int32); fx = np.full(max(len(keyframes), 1), -1, np.int32)
        ls = np.zeros(max(cap, 1), np.int32); pos = np.zeros((max(cap, 1), 3)); obs = np.zeros(max(ocap, 1), BA_OBS32)
        rc = self._L.orbx_map_collect_ba_window(
            self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(int(cur)), C.c_int(int(max_covisible)), C.c_int(cap), C.c_int(ocap),
            _vp(counts), _vp(lk), _vp(fx), _vp(ls), _vp(pos), _vp(obs))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        K, F, M, N = (int(x) for x in counts)
        return dict(counts=counts, local_kf=lk, fixed_kf=fx[:F - 1].copy(), list_slot=ls[:M].copy(), positions=pos[:M].copy(), obs32=obs[:N].copy())

    # ---- local inertial BA from the resident map (include/orbx.h, "local INERTIAL BA from the resident map") ----
    @staticmethod
    def _inertial_window_bounds(mp, keyframes, chain):
        """(list bound, observation bound): the chain's feature counts summed, at most the capacity; every feature of `keyframes`"""
        n = len(keyframes)
        cap = sum(keyframes[i].n for i in chain if 0 <= i < n)
        return int(min(cap, mp.capacity)), int(sum(k.n for k in keyframes))

    def map_collect_inertial_window_device(self, mp: "MapPointStore", keyframes, chain, device=None):
        """The inertial local-BA window of the temporal chain `chain` (positions in `keyframes`, oldest first), collected on the
        device (orbx_map_collect_inertial_window_device).  Returns a dict of CUDA tensors: counts [4] int32 = (K, F, M, N), fixed_kf
        [n_kfs] int32 (the F-1 other observers, ascending, then -1), list_slot [cap] int32 and positions [cap,3] f64 (rows [0, M)),
        obs32 [obs_cap,16] u8 (rows [0, N) are BA_OBS32 records whose mp_idx carries BA_OBS32_STEREO).  Asynchronous on the
        handle's stream.  None where the chain has fewer than two keyframes."""
        import torch
        ch = np.ascontiguousarray(chain, np.int32).reshape(-1)
        cap, ocap = self._inertial_window_bounds(mp, keyframes, ch)
        dev = device or torch.device("cuda", self.device)
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(counts=mk(4, torch.int32), fixed_kf=mk(max(len(keyframes), 1), torch.int32), list_slot=mk(max(cap, 1), torch.int32),
                 positions=mk((max(cap, 1), 3), torch.float64), obs32=mk((max(ocap, 1), BA_OBS32.itemsize), torch.uint8))
        self._after_torch(*o.values())
        rc = self._L.orbx_map_collect_inertial_window_device(
            self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(ch)), _vp(ch if len(ch) else np.zeros(1, np.int32)), C.c_int(cap),
            C.c_int(ocap), _vp(o["counts"]), _vp(o["fixed_kf"]), _vp(o["list_slot"]), _vp(o["positions"]), _vp(o["obs32"]))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        o["fixed_kf"] = o["fixed_kf"][:len(keyframes)]; o["list_slot"] = o["list_slot"][:cap]; o["positions"] = o["positions"][:cap]; o["obs32"] = o["obs32"][:ocap]
        return o

    def map_collect_inertial_window(self, mp: "MapPointStore", keyframes, chain, empty_info=None):
        """The host form (orbx_map_collect_inertial_window), synchronous: a dict of numpy arrays cut to their sizes — counts [4],
        fixed_kf [F-1], list_slot [M], positions [M,3], obs32 [N] BA_OBS32 — or None where the window is empty (the reference's
        None, local_inertial_ba.rs:940-942, :946-948).  empty_info: a dict that then receives counts and fixed_kf as written."""
        ch = np.ascontiguousarray(chain, np.int32).reshape(-1)
        cap, ocap = self._inertial_window_bounds(mp, keyframes, ch)
        counts = np.zeros(4, np.int32); fx = np.full(max(len(keyframes), 1), -1, np.int32)
        ls = np.zeros(max(cap, 1), np.int32); pos = np.zeros((max(cap, 1), 3)); obs = np.zeros(max(ocap, 1), BA_OBS32)
        rc = self._L.orbx_map_collect_inertial_window(
            self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(ch)), _vp(ch if len(ch) else np.zeros(1, np.int32)), C.c_int(cap),
            C.c_int(ocap), _vp(counts), _vp(fx), _vp(ls), _vp(pos), _vp(obs))
        if rc == ORBX_ERR_EMPTY:
            if empty_info is not None:
                empty_info["counts"] = counts; empty_info["fixed_kf"] = fx[:len(keyframes)]
            return None
        self._check(rc)
        K, F, M, N = (int(x) for x in counts)
        return dict(counts=counts, fixed_kf=fx[:F - 1].copy(), list_slot=ls[:M].copy(), positions=pos[:M].copy(), obs32=obs[:N].copy())

    def map_local_inertial_ba(self, camera, mp: "MapPointStore", keyframes, chain, velocities, biases, edge_kf, preint,
                              cfg: "LocalInertialBAConfig" = None, should_stop=None):
        """Inertial local BA of the temporal chain `chain` (positions in `keyframes`, oldest first) on the resident map
        (orbx_map_local_inertial_ba): the window is collected on the device, solved with its observations where they lie, and the
        optimised positions are written back into the store if the solve iterated.  velocities [K,3], biases [K,6], edge_kf [E,2]
        (positions in `chain`) and preint [E,11] as for ba_solve_inertial.  Returns a dict — poses_wc [K,7], velocities [K,3],
        biases [K,6] for every keyframe of the chain (apply the poses with KeyFrame.set_pose), fixed_kf [F-1], counts (K, F, M, N),
        iterations, initial_error, final_error — or None where the reference returns None."""
        cfg = cfg or LocalInertialBAConfig()
        ch = np.ascontiguousarray(chain, np.int32).reshape(-1)
        K = len(ch)
        vel = np.ascontiguousarray(velocities, np.float64).reshape(-1, 3); bias = np.ascontiguousarray(biases, np.float64).reshape(-1, 6)
        ek = np.ascontiguousarray(edge_kf, np.int32).reshape(-1, 2); pre = np.ascontiguousarray(preint, np.float64).reshape(-1, 11)
        if len(vel) != K or len(bias) != K or len(pre) != len(ek):
            raise ValueError("map_local_inertial_ba: inconsistent array lengths")
        out_p = np.zeros((max(K, 1), 7)); out_v = np.zeros((max(K, 1), 3)); out_b = np.zeros((max(K, 1), 6))
        fx = np.full(max(len(keyframes), 1), -1, np.int32); counts = np.zeros(4, np.int32)
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        pad = lambda a, shape: a if len(a) else np.zeros(shape, a.dtype)
        rc = self._L.orbx_map_local_inertial_ba(
            self._h, C.byref(cam), C.byref(c), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(K), _vp(pad(ch, 1)), _vp(pad(vel, (1, 3))),
            _vp(pad(bias, (1, 6))), C.c_int(len(ek)), _vp(pad(ek, (1, 2))), _vp(pad(pre, (1, 11))), cb, None, _vp(out_p), _vp(out_v), _vp(out_b), _vp(fx),
            _vp(counts), C.byref(it), C.byref(e0), C.byref(e1))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        F = int(counts[1])
        return dict(poses_wc=out_p[:K], velocities=out_v[:K], biases=out_b[:K], fixed_kf=fx[:F - 1].copy(), counts=counts, iterations=it.value,
                    initial_error=e0.value, final_error=e1.value)

    # ---- global BA from the resident map (include/orbx.h, "global BA from the resident map") ----
    @staticmethod
    def _global_bounds(mp, keyframes):
        """(list bound, observation bound): every feature of `keyframes`, the list's at most the capacity"""
        n = int(sum(k.n for k in keyframes))
        return int(min(n, mp.capacity)), n

    def map_collect_global_device(self, mp: "MapPointStore", keyframes, device=None, list_cap=None, obs_cap=None):
        """The whole map's global-BA problem (global_ba.rs:100-181), collected on the device from the slot tables, the keypoints and the
        store (orbx_map_collect_global_device): keyframes[0] is the anchor, keyframes[1:] the K optimised keyframes.  Returns a dict of
        CUDA tensors: counts [4] int32 = (K, 1, M, N), list_slot [cap] int32 and positions [cap,3] f64 (the distinct live slots in
        first-seen order, rows [0, M)), obs32 [obs_cap,16] u8 (rows [0, N) are BA_OBS32 records, kf_idx -1 the anchor's).
        Asynchronous on the handle's stream.  list_cap / obs_cap: other capacities than the bounds (one below its bound is refused)."""
        import torch
        cap, ocap = self._global_bounds(mp, keyframes)
        cap = cap if list_cap is None else int(list_cap); ocap = ocap if obs_cap is None else int(obs_cap)
        dev = device or torch.device("cuda", self.device)
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(counts=mk(4, torch.int32), list_slot=mk(max(cap, 1), torch.int32), positions=mk((max(cap, 1), 3), torch.float64),
                 obs32=mk((max(ocap, 1), BA_OBS32.itemsize), torch.uint8))
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_collect_global_device(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(cap), C.c_int(ocap),
                                                           _vp(o["counts"]), _vp(o["list_slot"]), _vp(o["positions"]), _vp(o["obs32"])))
        o["list_slot"] = o["list_slot"][:cap]; o["positions"] = o["positions"][:cap]; o["obs32"] = o["obs32"][:ocap]
        return o

    def map_collect_global(self, mp: "MapPointStore", keyframes, list_cap=None, obs_cap=None):
        """The host form (orbx_map_collect_global), synchronous: a dict of numpy arrays cut to their sizes — counts [4], list_slot [M],
        positions [M,3], obs32 [N] BA_OBS32 — or None where the keyframes observe no live map point (global_ba.rs:176-178)."""
        cap, ocap = self._global_bounds(mp, keyframes)
        cap = cap if list_cap is None else int(list_cap); ocap = ocap if obs_cap is None else int(obs_cap)
        counts = np.zeros(4, np.int32); ls = np.zeros(max(cap, 1), np.int32); pos = np.zeros((max(cap, 1), 3)); obs = np.zeros(max(ocap, 1), BA_OBS32)
        rc = self._L.orbx_map_collect_global(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(cap), C.c_int(ocap), _vp(counts), _vp(ls),
                                             _vp(pos), _vp(obs))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        K, F, M, N = (int(x) for x in counts)
        return dict(counts=counts, list_slot=ls[:M].copy(), positions=pos[:M].copy(), obs32=obs[:N].copy())

    def map_global_ba(self, camera, mp: "MapPointStore", keyframes, cfg: "GlobalBAConfig" = None, should_stop=None):
        """Global BA of the whole resident map (orbx_map_global_ba): keyframes[0] stays fixed, the problem is collected on the device,
        solved by the whole-map solver with its observations where they lie, and the optimised positions are written back into the
        store if the solve iterated.  Returns a dict — poses_wc [K,7] of keyframes[1:] (apply them with KeyFrame.set_pose), counts
        (K, 1, M, N), iterations, initial_error, final_error — or None where the reference returns None."""
        cfg = cfg or GlobalBAConfig()
        K = max(len(keyframes) - 1, 0)
        out_p = np.zeros((max(K, 1), 7)); counts = np.zeros(4, np.int32)
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        rc = self._L.orbx_map_global_ba(self._h, C.byref(cam), C.byref(c), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), cb, None, _vp(out_p),
                                        _vp(counts), C.byref(it), C.byref(e0), C.byref(e1))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        return dict(poses_wc=out_p[:K], counts=counts, iterations=it.value, initial_error=e0.value, final_error=e1.value)

    # ---- observations from the resident map (include/orbx.h, "observations from the resident map") ----
    @staticmethod
    def _obs_slots(slots):
        a = np.ascontiguousarray(slots, np.int32).reshape(-1)
        return a, (a if len(a) else np.zeros(1, np.int32))

    def map_observations_device(self, mp: "MapPointStore", keyframes, slots, device=None):
        """mp.observations of the points in `slots` (a host array of live slots, none twice), derived on the device from the slot
        tables of `keyframes` (orbx_map_observations_device).  Returns a dict of CUDA tensors: obs_start [M+1] int32, obs_kf / obs_feat
        [cap] int32 with cap = the keyframes' feature counts summed; point p owns rows obs_start[p]..obs_start[p+1]: the keyframes
        (positions in `keyframes`, ascending) that observe it and the first feature of each that names it.  The arguments of
        refresh_map_points_device.  Asynchronous on the handle's stream."""
        import torch
        a, ap = self._obs_slots(slots)
        cap = int(sum(k.n for k in keyframes))
        dev = device or torch.device("cuda", self.device)
        mk = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        o = dict(obs_start=mk(len(a) + 1), obs_kf=mk(max(cap, 1)), obs_feat=mk(max(cap, 1)))
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_observations_device(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(a)), _vp(ap), C.c_int(cap),
                                                         _vp(o["obs_start"]), _vp(o["obs_kf"]), _vp(o["obs_feat"])))
        o["obs_kf"] = o["obs_kf"][:cap]; o["obs_feat"] = o["obs_feat"][:cap]
        return o

    def map_observations(self, mp: "MapPointStore", keyframes, slots):
        """The host form (orbx_map_observations), synchronous: (obs_start [M+1], obs_kf [N], obs_feat [N]) as numpy int32 arrays cut
        to N = obs_start[M].  A point's observer count, obs_start[p+1] - obs_start[p], is what map-point culling compares with
        min_observations."""
        a, ap = self._obs_slots(slots)
        cap = int(sum(k.n for k in keyframes))
        os_ = np.zeros(len(a) + 1, np.int32); ok = np.zeros(max(cap, 1), np.int32); of = np.zeros(max(cap, 1), np.int32)
        self._check(self._L.orbx_map_observations(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(a)), _vp(ap), C.c_int(cap),
                                                  _vp(os_), _vp(ok), _vp(of)))
        N = int(os_[-1])
        return os_, ok[:N].copy(), of[:N].copy()

    def map_refresh_points_device(self, mp: "MapPointStore", keyframes, slots, scale_range, normals):
        """Phase 4 of search_in_neighbors on the resident map (orbx_map_refresh_points_device): the observation lists of `slots` from
        the tables, refresh_map_points' kernels on the keyframes' own descriptors and camera centres and the store's rows, and the
        chosen descriptors written back into the store.  normals: CUDA tensor [M,3] f64, updated IN PLACE (the store keeps none).
        Returns a dict of CUDA tensors: mp_desc [M,32] u8, min_distance / max_distance [M] f64, records [M,16] u8
        (MP_REFRESH_RECORD).  Asynchronous on the handle's stream."""
        import torch
        a, ap = self._obs_slots(slots)
        M = len(a)
        if tuple(normals.shape) != (M, 3) or normals.dtype != torch.float64 or not normals.is_contiguous():
            raise ValueError("map_refresh_points_device: normals is a contiguous [M,3] f64 tensor")
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=normals.device)
        o = dict(mp_desc=mk((max(M, 1), 32), torch.uint8), min_distance=mk(max(M, 1), torch.float64), max_distance=mk(max(M, 1), torch.float64),
                 records=mk((max(M, 1), MP_REFRESH_RECORD.itemsize), torch.uint8))
        self._after_torch(normals, *o.values())
        self._check(self._L.orbx_map_refresh_points_device(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(M), _vp(ap),
                                                           C.c_double(scale_range), _vp(o["mp_desc"]), _vp(normals), _vp(o["min_distance"]),
                                                           _vp(o["max_distance"]), _vp(o["records"])))
        return {k: v[:M] for k, v in o.items()}

    def map_refresh_points(self, mp: "MapPointStore", keyframes, slots, scale_range, normals) -> "MapPointRefresh":
        """The host form (orbx_map_refresh_points), synchronous: normals [M,3] are the points' current normals (not modified); the
        result is KeyFrame.refresh_map_points' on the derived lists and the store's rows, byte for byte, and the store holds its
        mp_desc afterwards."""
        a, ap = self._obs_slots(slots)
        M = len(a)
        nr = np.array(normals, np.float64).reshape(-1, 3)
        if len(nr) != M:
            raise ValueError("map_refresh_points: one normal per slot")
        out = MapPointRefresh(np.zeros((M, 32), np.uint8), nr, np.zeros(M), np.zeros(M), np.zeros(M, MP_REFRESH_RECORD))
        self._after_torch()
        self._check(self._L.orbx_map_refresh_points(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(M), _vp(ap), C.c_double(scale_range),
                                                    _vp(out.mp_desc) if M else None, _vp(out.normals) if M else None, _vp(out.min_distance) if M else None,
                                                    _vp(out.max_distance) if M else None, _vp(out.records) if M else None))
        return out

    def map_keyframe_redundancy_device(self, mp: "MapPointStore", keyframes, candidates, min_observations=3, threshold=0.9, device=None):
        """cull_keyframes' decision (local_mapper.rs:487-583) for keyframes[c], c in candidates (orbx_map_keyframe_redundancy_device).
        Returns a dict of CUDA tensors: total [n_cand] int32 (features with a live point), redundant [n_cand] int32 (those whose point
        has min_observations other observers among `keyframes`), cull [n_cand] u8 (redundant / total > threshold).  Asynchronous."""
        import torch
        c = np.ascontiguousarray(candidates, np.int32).reshape(-1)
        n = len(c)
        dev = device or torch.device("cuda", self.device)
        o = dict(total=torch.zeros(max(n, 1), dtype=torch.int32, device=dev), redundant=torch.zeros(max(n, 1), dtype=torch.int32, device=dev),
                 cull=torch.zeros(max(n, 1), dtype=torch.uint8, device=dev))
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_keyframe_redundancy_device(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(n),
                                                                _vp(c if n else np.zeros(1, np.int32)), C.c_int(int(min_observations)), C.c_double(threshold),
                                                                _vp(o["total"]), _vp(o["redundant"]), _vp(o["cull"])))
        return {k: v[:n] for k, v in o.items()}

    def map_keyframe_redundancy(self, mp: "MapPointStore", keyframes, candidates, min_observations=3, threshold=0.9):
        """The host form (orbx_map_keyframe_redundancy), synchronous: (total int32 [n_cand], redundant int32 [n_cand], cull u8 [n_cand])."""
        c = np.ascontiguousarray(candidates, np.int32).reshape(-1)
        n = len(c)
        total = np.zeros(max(n, 1), np.int32); red = np.zeros(max(n, 1), np.int32); cull = np.zeros(max(n, 1), np.uint8)
        self._check(self._L.orbx_map_keyframe_redundancy(self._h, mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(n),
                                                         _vp(c if n else np.zeros(1, np.int32)), C.c_int(int(min_observations)), C.c_double(threshold), _vp(total),
                                                         _vp(red), _vp(cull)))
        return total[:n], red[:n], cull[:n]

    # ---- fuse and merge on the resident map (include/orbx.h, "fuse and merge on the resident map") ----
    @staticmethod
    def _fuse_bounds(mp, keyframes, src, tgt):
        """(L's bound, the goner lists' bound) of one pass: the features of keyframes[src[..]], at most the capacity; that plus the
        targets' features.  Indices out of range count nothing: the library refuses them."""
        n = lambda idx: int(sum(keyframes[i].n for i in idx if 0 <= i < len(keyframes)))
        bound = min(n(src), mp.capacity)
        return bound, bound + n(tgt)

    def map_fuse_device(self, camera, mp: "MapPointStore", keyframes, src, tgt, radius_scale, desc_threshold=TH_LOW, device=None):
        """One pass fuse(src, tgt) of search_in_neighbors' fuse and merge on the resident map (orbx_map_fuse_device): the distinct
        live points of keyframes[src[..]] are searched in keyframes[tgt[..]], matches associate or merge, and every table of
        `keyframes` is rewritten where it lies.  Returns a dict of CUDA tensors: counts [4] int32 = (P, matches, added, goners),
        list_slot [cap] int32 (rows [0, P)), match [cap, n_tgt] int32 (rows [0, P): the matched feature or -1), goner / keeper
        [goner cap] int32 (rows [0, goners), by ascending goner slot).  The store's live bytes are untouched: erasing the goners is
        the caller's (map_fuse does it).  Asynchronous on the handle's stream."""
        import torch
        src = np.ascontiguousarray(src, np.int32).reshape(-1); tgt = np.ascontiguousarray(tgt, np.int32).reshape(-1)
        cap, gcap = self._fuse_bounds(mp, keyframes, src, tgt)
        dev = device or torch.device("cuda", self.device)
        mk = lambda shape: torch.empty(shape, dtype=torch.int32, device=dev)
        o = dict(counts=mk(4), list_slot=mk(max(cap, 1)), match=mk((max(cap, 1), max(len(tgt), 1))), goner=mk(max(gcap, 1)), keeper=mk(max(gcap, 1)))
        cam = camera._c()
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_fuse_device(self._h, C.byref(cam), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(src)),
                                                 _vp(src if len(src) else np.zeros(1, np.int32)), C.c_int(len(tgt)), _vp(tgt if len(tgt) else np.zeros(1, np.int32)),
                                                 C.c_double(radius_scale), C.c_uint(int(desc_threshold)), C.c_int(cap), _vp(o["counts"]), _vp(o["list_slot"]),
                                                 _vp(o["match"]), _vp(o["goner"]), _vp(o["keeper"])))
        o["list_slot"] = o["list_slot"][:cap]; o["match"] = o["match"][:cap, :len(tgt)]; o["goner"] = o["goner"][:gcap]; o["keeper"] = o["keeper"][:gcap]
        return o

    def map_fuse(self, camera, mp: "MapPointStore", keyframes, src, tgt, radius_scale, desc_threshold=TH_LOW):
        """The host form (orbx_map_fuse), synchronous: a dict of numpy int32 arrays cut to their sizes — counts [4], list_slot [P],
        match [P, n_tgt], goner / keeper [goners] — and the goners erased from the store."""
        src = np.ascontiguousarray(src, np.int32).reshape(-1); tgt = np.ascontiguousarray(tgt, np.int32).reshape(-1)
        cap, gcap = self._fuse_bounds(mp, keyframes, src, tgt)
        T = len(tgt)
        counts = np.zeros(4, np.int32); ls = np.zeros(max(cap, 1), np.int32); ma = np.full(max(cap, 1) * max(T, 1), -1, np.int32)
        go = np.zeros(max(gcap, 1), np.int32); ke = np.zeros(max(gcap, 1), np.int32)
        cam = camera._c()
        self._after_torch()
        self._check(self._L.orbx_map_fuse(self._h, C.byref(cam), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(len(src)),
                                          _vp(src if len(src) else np.zeros(1, np.int32)), C.c_int(T), _vp(tgt if T else np.zeros(1, np.int32)),
                                          C.c_double(radius_scale), C.c_uint(int(desc_threshold)), C.c_int(cap), _vp(counts), _vp(ls), _vp(ma), _vp(go), _vp(ke)))
        P, G = int(counts[0]), int(counts[3])
        return dict(counts=counts, list_slot=ls[:P].copy(), match=ma[:P * T].reshape(P, T).copy(), goner=go[:G].copy(), keeper=ke[:G].copy())

    def map_search_in_neighbors(self, camera, mp: "MapPointStore", keyframes, cur, neighbours, radius_scale, scale_range, desc_threshold=TH_LOW,
                                slot_normals=None):
        """Phases 2 to 4 of search_in_neighbors for keyframes[cur] and keyframes[neighbours[..]] on the resident map
        (orbx_map_search_in_neighbors), synchronous: pass A fuse([cur], neighbours), pass B fuse(neighbours, [cur]), one download, the
        goners erased, map_refresh_points on the affected list.  slot_normals [capacity,3]: every slot's normal before the call
        (None: zeros).  Returns a dict: counts [2,4] int32, goner_a / keeper_a / goner_b / keeper_b, affected [M] int32 and
        refresh (MapPointRefresh, in the affected list's order)."""
        nb = np.ascontiguousarray(neighbours, np.int32).reshape(-1)
        n = lambda idx: int(sum(keyframes[i].n for i in idx if 0 <= i < len(keyframes)))
        f_cur, f_nb = n([int(cur)]), n(nb)
        gcap = max(min(f_cur, mp.capacity) + f_nb, min(f_nb, mp.capacity) + f_cur, 1)
        acap = max(min(f_cur + f_nb, mp.capacity), 1)
        counts = np.zeros(8, np.int32)
        g = [np.zeros(gcap, np.int32) for _ in range(4)]
        n_aff = C.c_int(0)
        aff = np.zeros(acap, np.int32)
        out = MapPointRefresh(np.zeros((acap, 32), np.uint8), np.zeros((acap, 3)), np.zeros(acap), np.zeros(acap), np.zeros(acap, MP_REFRESH_RECORD))
        sn = None
        if slot_normals is not None:
            sn = np.ascontiguousarray(slot_normals, np.float64).reshape(-1, 3)
            if len(sn) != mp.capacity:
                raise ValueError("map_search_in_neighbors: slot_normals is [capacity,3]")
        cam = camera._c()
        self._after_torch()
        self._check(self._L.orbx_map_search_in_neighbors(
            self._h, C.byref(cam), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(int(cur)), C.c_int(len(nb)),
            _vp(nb if len(nb) else np.zeros(1, np.int32)), C.c_double(radius_scale), C.c_uint(int(desc_threshold)), C.c_double(scale_range),
            _vp(sn) if sn is not None else None, C.c_int(gcap), C.c_int(acap), _vp(counts), _vp(g[0]), _vp(g[1]), _vp(g[2]), _vp(g[3]), C.byref(n_aff), _vp(aff),
            _vp(out.mp_desc), _vp(out.normals), _vp(out.min_distance), _vp(out.max_distance), _vp(out.records)))
        M, Ga, Gb = n_aff.value, int(counts[3]), int(counts[7])
        refresh = MapPointRefresh(out.mp_desc[:M].copy(), out.normals[:M].copy(), out.min_distance[:M].copy(), out.max_distance[:M].copy(), out.records[:M].copy())
        return dict(counts=counts.reshape(2, 4), goner_a=g[0][:Ga].copy(), keeper_a=g[1][:Ga].copy(), goner_b=g[2][:Gb].copy(), keeper_b=g[3][:Gb].copy(),
                    affected=aff[:M].copy(), refresh=refresh)

    # ---- loop correction on the resident map (include/orbx.h, "loop correction on the resident map") ----
    @staticmethod
    def _loop_args(mp, keyframes, parent, sim3, feature_matches):
        """(parent, sim3, matches, n_matches, list_cap) of a loop-correction call as contiguous host arrays; list_cap is the list's
        bound: the keyframes' features summed, at most the capacity"""
        par = np.ascontiguousarray(parent, np.int32).reshape(-1)
        if len(par) != len(keyframes):
            raise ValueError("loop correction: parent holds one entry per keyframe")
        s3 = np.ascontiguousarray(sim3, np.float64).reshape(8)
        fm = np.ascontiguousarray(feature_matches if feature_matches is not None else np.zeros((0, 2)), np.int32).reshape(-1, 2)
        return par, s3, fm, len(fm), min(int(sum(k.n for k in keyframes)), mp.capacity)

    def map_correct_loop_device(self, mp: "MapPointStore", keyframes, parent, cur, loop, sim3, feature_matches=None, cfg: "LoopCorrectConfig" = None,
                                device=None):
        """correct_loop on the resident map (orbx_map_correct_loop_device): the keyframes within reach of keyframes[cur] (spanning-tree
        children through `parent`, covisibility arcs), their points and poses corrected by the inverse of sim3 (qw,qx,qy,qz,tx,ty,tz,
        scale: verify_loop_candidates' sim3), and the matched points of cur and loop fused in every table.  feature_matches [n,2]
        (current feature, loop feature): a CUDA int32 tensor or a host array.  Returns a dict of CUDA tensors: counts [4] int32 =
        (affected keyframes, affected points, pairs, goners), affected [n_kfs] u8, poses_wc [n_kfs,7] f64, list_slot [cap] int32, goner /
        keeper [n_matches] int32.  The keyframes' own poses and the store's live bytes are untouched: applying the poses and erasing
        the goners is the caller's (map_correct_loop does both).  Asynchronous on the handle's stream."""
        import torch
        dev = device or torch.device("cuda", self.device)
        if getattr(feature_matches, "is_cuda", False):
            d_fm = feature_matches.to(torch.int32).contiguous().reshape(-1, 2)
            par, s3, _, M, cap = self._loop_args(mp, keyframes, parent, sim3, None)
            M = int(d_fm.shape[0])
        else:
            par, s3, fm, M, cap = self._loop_args(mp, keyframes, parent, sim3, feature_matches)
            d_fm = torch.from_numpy(fm if M else np.zeros((1, 2), np.int32)).to(dev)
        K = len(keyframes)
        mk = lambda shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=dev)
        o = dict(counts=mk(4), affected=mk(max(K, 1), torch.uint8), poses_wc=mk((max(K, 1), 7), torch.float64), list_slot=mk(max(cap, 1)),
                 goner=mk(max(M, 1)), keeper=mk(max(M, 1)))
        c = (cfg or LoopCorrectConfig())._c()
        self._after_torch(d_fm, *o.values())
        self._check(self._L.orbx_map_correct_loop_device(self._h, C.byref(c), mp._p, C.c_int(K), self._kf_array(keyframes), _vp(par if K else np.zeros(1, np.int32)),
                                                         C.c_int(int(cur)), C.c_int(int(loop)), _vp(s3), C.c_int(M), _vp(d_fm), C.c_int(cap), _vp(o["counts"]),
                                                         _vp(o["affected"]), _vp(o["poses_wc"]), _vp(o["list_slot"]), _vp(o["goner"]), _vp(o["keeper"])))
        o["affected"] = o["affected"][:K]; o["poses_wc"] = o["poses_wc"][:K]; o["list_slot"] = o["list_slot"][:cap]; o["goner"] = o["goner"][:M]; o["keeper"] = o["keeper"][:M]
        return o

    def _loop_host_outputs(self, K, M, cap):
        return dict(counts=np.zeros(4, np.int32), affected=np.zeros(max(K, 1), np.uint8), poses_wc=np.zeros((max(K, 1), 7)), list_slot=np.zeros(max(cap, 1), np.int32),
                    goner=np.zeros(max(M, 1), np.int32), keeper=np.zeros(max(M, 1), np.int32))

    @staticmethod
    def _loop_cut(o, K):
        P, G = int(o["counts"][1]), int(o["counts"][3])
        return dict(counts=o["counts"], affected=o["affected"][:K].copy(), poses_wc=o["poses_wc"][:K].copy(), list_slot=o["list_slot"][:P].copy(),
                    goner=o["goner"][:G].copy(), keeper=o["keeper"][:G].copy())

    def map_correct_loop(self, mp: "MapPointStore", keyframes, parent, cur, loop, sim3, feature_matches=None, cfg: "LoopCorrectConfig" = None):
        """The host form (orbx_map_correct_loop), synchronous: a dict of numpy arrays cut to their sizes — counts [4], affected [n_kfs],
        poses_wc [n_kfs,7], list_slot [affected points], goner / keeper [goners] — with the corrected poses applied to the affected
        keyframes and the goners erased from the store."""
        par, s3, fm, M, cap = self._loop_args(mp, keyframes, parent, sim3, feature_matches)
        K = len(keyframes)
        o = self._loop_host_outputs(K, M, cap)
        c = (cfg or LoopCorrectConfig())._c()
        self._after_torch()
        self._check(self._L.orbx_map_correct_loop(self._h, C.byref(c), mp._p, C.c_int(K), self._kf_array(keyframes), _vp(par if K else np.zeros(1, np.int32)),
                                                  C.c_int(int(cur)), C.c_int(int(loop)), _vp(s3), C.c_int(M), _vp(fm if M else np.zeros((1, 2), np.int32)), C.c_int(cap),
                                                  _vp(o["counts"]), _vp(o["affected"]), _vp(o["poses_wc"]), _vp(o["list_slot"]), _vp(o["goner"]), _vp(o["keeper"])))
        return self._loop_cut(o, K)

    def map_close_loop(self, camera, mp: "MapPointStore", keyframes, parent, cur, loop, sim3, feature_matches=None, cfg: "LoopCorrectConfig" = None,
                       ba_cfg: "GlobalBAConfig" = None, global_ba=True, should_stop=None):
        """Step 5 of LoopCloser::process_keyframe and the global BA behind it (orbx_map_close_loop): map_correct_loop, then, unless
        global_ba is False, map_global_ba on the same keyframes (keyframes[0] the anchor).  Returns map_correct_loop's dict with
        global_ba = map_global_ba's dict (None where that call returns None or was not asked for): its poses are not applied."""
        par, s3, fm, M, cap = self._loop_args(mp, keyframes, parent, sim3, feature_matches)
        K = len(keyframes)
        o = self._loop_host_outputs(K, M, cap)
        c = (cfg or LoopCorrectConfig())._c()
        bc = (ba_cfg or GlobalBAConfig())._c()
        out_p = np.zeros((max(K - 1, 1), 7)); ba_counts = np.zeros(4, np.int32)
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c()
        self._after_torch()
        rc = self._L.orbx_map_close_loop(self._h, C.byref(cam), C.byref(c), C.byref(bc) if global_ba else None, mp._p, C.c_int(K), self._kf_array(keyframes),
                                         _vp(par if K else np.zeros(1, np.int32)), C.c_int(int(cur)), C.c_int(int(loop)), _vp(s3), C.c_int(M),
                                         _vp(fm if M else np.zeros((1, 2), np.int32)), C.c_int(cap), _vp(o["counts"]), _vp(o["affected"]), _vp(o["poses_wc"]),
                                         _vp(o["list_slot"]), _vp(o["goner"]), _vp(o["keeper"]), cb, None, _vp(out_p), _vp(ba_counts), C.byref(it), C.byref(e0), C.byref(e1))
        if rc != ORBX_ERR_EMPTY:
            self._check(rc)
        res = self._loop_cut(o, K)
        res["global_ba"] = None
        if global_ba and rc == 0:
            res["global_ba"] = dict(poses_wc=out_p[:max(K - 1, 0)], counts=ba_counts, iterations=it.value, initial_error=e0.value, final_error=e1.value)
        return res

    # ---- create and cull map points on the resident map (include/orbx.h, "create and cull map points on the resident map") ----
    def map_create_points_device(self, camera, mp: "MapPointStore", cur: "KeyFrame", neighbours, free_slots, phases=MAP_CREATE_STEREO | MAP_CREATE_NEIGHBOURS,
                                 config: "TriangulationConfig" = None, is_inertial=False, device=None):
        """Steps 3 and 3b of process_keyframe on the resident map (orbx_map_create_points_device): the stereo points of `cur` and the
        points triangulated with `neighbours` take free_slots (a host array) in creation order and are written into the keyframes'
        tables where they lie.  Returns a dict of CUDA tensors: counts [4] int32 = (S, N, created, dropped), new_slot / new_neighbour /
        new_idx1 / new_idx2 [n_free] int32, new_points [n_free,3] f64, new_desc [n_free,32] u8 (rows [0, created)), stats [T,4] int32.
        The store is untouched: mp.set_device(free_slots[:created], new_points[:created], new_desc[:created]) makes the points live.
        Asynchronous on the handle's stream."""
        import torch
        fs = np.ascontiguousarray(free_slots, np.int32).reshape(-1)
        nf, T = len(fs), len(neighbours)
        dev = device or torch.device("cuda", self.device)
        mk = lambda shape, dt=torch.int32: torch.empty(shape, dtype=dt, device=dev)
        o = dict(counts=mk(4), new_slot=mk(max(nf, 1)), new_neighbour=mk(max(nf, 1)), new_idx1=mk(max(nf, 1)), new_idx2=mk(max(nf, 1)),
                 new_points=mk((max(nf, 1), 3), torch.float64), new_desc=mk((max(nf, 1), 32), torch.uint8), stats=mk((max(T, 1), 4)))
        cam = camera._c(); cfg = (config or TriangulationConfig())._c()
        self._after_torch(*o.values())
        self._check(self._L.orbx_map_create_points_device(
            self._h, C.byref(cam), C.byref(cfg), int(bool(is_inertial)), mp._p, cur._p, self._kf_array(neighbours), T, int(phases),
            _vp(fs if nf else np.zeros(1, np.int32)), nf, _vp(o["counts"]), _vp(o["new_slot"]), _vp(o["new_neighbour"]), _vp(o["new_idx1"]), _vp(o["new_idx2"]),
            _vp(o["new_points"]), _vp(o["new_desc"]), _vp(o["stats"])))
        for k in ("new_slot", "new_neighbour", "new_idx1", "new_idx2", "new_points", "new_desc"):
            o[k] = o[k][:nf]
        o["stats"] = o["stats"][:T]
        return o

    def map_create_points(self, camera, mp: "MapPointStore", cur: "KeyFrame", neighbours, free_slots, phases=MAP_CREATE_STEREO | MAP_CREATE_NEIGHBOURS,
                          config: "TriangulationConfig" = None, is_inertial=False):
        """The host form (orbx_map_create_points), synchronous: one download, then the new points are made live in the store.
        Returns a dict of numpy arrays cut to `created`: counts [4], new_slot / new_neighbour / new_idx1 / new_idx2 int32, new_points
        [created,3] f64, stats [T,4] int32."""
        fs = np.ascontiguousarray(free_slots, np.int32).reshape(-1)
        nf, T = len(fs), len(neighbours)
        counts = np.zeros(4, np.int32); stats = np.zeros((max(T, 1), 4), np.int32)
        li = [np.zeros(max(nf, 1), np.int32) for _ in range(4)]
        pts = np.zeros((max(nf, 1), 3))
        cam = camera._c(); cfg = (config or TriangulationConfig())._c()
        self._after_torch()
        self._check(self._L.orbx_map_create_points(
            self._h, C.byref(cam), C.byref(cfg), int(bool(is_inertial)), mp._p, cur._p, self._kf_array(neighbours), T, int(phases),
            _vp(fs if nf else np.zeros(1, np.int32)), nf, _vp(counts), _vp(li[0]), _vp(li[1]), _vp(li[2]), _vp(li[3]), _vp(pts), _vp(stats)))
        m = int(counts[2])
        return dict(counts=counts, new_slot=li[0][:m].copy(), new_neighbour=li[1][:m].copy(), new_idx1=li[2][:m].copy(), new_idx2=li[3][:m].copy(),
                    new_points=pts[:m].copy(), stats=stats[:T].copy())

    def map_remove_points(self, mp: "MapPointStore", keyframes, slots, count=True):
        """remove_map_point_full for a list (orbx_map_remove_points): every entry of the tables of `keyframes` that names a listed
        slot becomes -1, then the slots are erased.  Returns the number of table entries cleared (one 4-byte download), or None with
        count=False (nothing is downloaded, the call does not wait)."""
        a = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = C.c_int(0)
        self._after_torch()
        self._check(self._L.orbx_map_remove_points(self._h, mp._p, len(keyframes), self._kf_array(keyframes), len(a), _vp(a if len(a) else np.zeros(1, np.int32)),
                                                   C.byref(n) if count else None))
        return n.value if count else None

    def map_cull_points(self, mp: "MapPointStore", keyframes, candidates, min_observations):
        """cull_map_points on the resident map (orbx_map_cull_points), synchronous: the candidates (live slots, none twice) observed
        by fewer than min_observations of `keyframes` are removed as map_remove_points removes them.  Returns them, int32, in the
        candidates' order."""
        a = np.ascontiguousarray(candidates, np.int32).reshape(-1)
        n = C.c_int(0); out = np.zeros(max(len(a), 1), np.int32)
        self._after_torch()
        self._check(self._L.orbx_map_cull_points(self._h, mp._p, len(keyframes), self._kf_array(keyframes), len(a), _vp(a if len(a) else np.zeros(1, np.int32)),
                                                 int(min_observations), C.byref(n), _vp(out)))
        return out[:n.value].copy()

    def ba_solve_visual_obs32_device(self, camera, cfg, poses_cw, fixed_cw, points, obs32, n_obs, should_stop=None):
        """ba_solve_visual with the observations in device memory (orbx_ba_solve_visual_obs32_device): obs32 is a CUDA tensor whose
        first 16 * n_obs bytes are BA_OBS32 records (map_collect_ba_window_device's), 16-byte aligned.  Poses and points are host
        arrays; the result is ba_solve_visual's dict, bit for bit what it gives for a host copy of the observations."""
        poses_cw = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 7)
        fixed_cw = np.ascontiguousarray(fixed_cw, np.float64).reshape(-1, 7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        K, F, M, N = len(poses_cw), len(fixed_cw), len(pts), int(n_obs)
        if N < 0 or N * BA_OBS32.itemsize > obs32.numel() * obs32.element_size():
            raise ValueError("obs32 holds fewer than n_obs records")
        out_wc = np.zeros((max(K, 1), 7))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        self._after_torch(obs32)
        rc = self._L.orbx_ba_solve_visual_obs32_device(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_cw), C.c_int(F), _vp(fixed_cw), C.c_int(M), _vp(pts),
                                                       C.c_int(N), _vp(obs32), cb, None, _vp(out_wc), C.byref(it), C.byref(e0), C.byref(e1))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        return dict(poses_wc=out_wc[:K], points=pts, iterations=it.value, initial_error=e0.value, final_error=e1.value)

    def map_local_ba(self, camera, mp: "MapPointStore", keyframes, cur, cfg: "LocalBAConfigLM" = None, should_stop=None,
                     read_points=True) -> Optional["MapLocalBAResult"]:
        """Local BA of keyframes[cur]'s window on the resident map (orbx_map_local_ba): the window is collected on the device, solved
        with its observations where they lie, and the optimised positions are written back into the store.  Returns a
        MapLocalBAResult — optimized_poses keyed by position in `keyframes` (apply them with KeyFrame.set_pose),
        optimized_points keyed by slot, read back from the store (read_points=False leaves them out: a caller that keeps its map on
        the device has no use for them) — or None where the reference returns None."""
        import torch
        cfg = cfg or LocalBAConfigLM()
        mc = int(cfg.max_covisible_keyframes)
        lk = np.full(1 + max(mc, 0), -1, np.int32); poses = np.zeros((max(mc, 1), 7)); counts = np.zeros(4, np.int32)
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        rc = self._L.orbx_map_local_ba(self._h, C.byref(cam), C.byref(c), mp._p, C.c_int(len(keyframes)), self._kf_array(keyframes), C.c_int(int(cur)), cb, None,
                                       _vp(lk), _vp(poses), _vp(counts), C.byref(it), C.byref(e0), C.byref(e1))
        if rc == ORBX_ERR_EMPTY:
            return None
        self._check(rc)
        K, F, M, N = (int(x) for x in counts)
        opt_poses = {int(lk[1 + i]): poses[i].copy() for i in range(K)}
        if not read_points:
            return MapLocalBAResult(opt_poses, {}, it.value, e0.value, e1.value, lk, counts, None, None)
        # the window's points: the selection over the local keyframes, whose gathered positions are now the optimised ones
        sel = self.map_select_points_device(mp, keyframes=[[keyframes[i] for i in lk[:1 + K]]])
        torch.cuda.synchronize()
        slots = sel["list_slot"][:M].cpu().numpy(); pts = sel["positions"][:M].cpu().numpy()
        return MapLocalBAResult(opt_poses, {int(s): pts[j] for j, s in enumerate(slots)}, it.value, e0.value, e1.value, lk, counts, slots, pts)

    def compute_sim3_ransac_batch(self, problems, cfg: "Sim3SolverConfig" = None):
        """compute_sim3_ransac (sim3_solver.rs:63-145) for many point sets [(points1 [n,3], points2 [n,3]), ...] in one call (one
        upload, one download).  Returns (sim3 [P,8], inlier masks (list of [n] u8), results [P] SIM3_RESULT); each problem's bytes
        equal its single call's."""
        a = [np.ascontiguousarray(x, np.float64).reshape(-1, 3) for x, _ in problems]
        b = [np.ascontiguousarray(y, np.float64).reshape(-1, 3) for _, y in problems]
        if any(len(x) != len(y) for x, y in zip(a, b)):
            raise ValueError("points1 and points2 differ in length")
        P = len(problems)
        off = np.zeros(P + 1, np.int32); off[1:] = np.cumsum([len(x) for x in a])
        N = int(off[-1])
        p1 = np.concatenate(a) if N else np.zeros((1, 3)); p2 = np.concatenate(b) if N else np.zeros((1, 3))
        sim3 = np.zeros((max(P, 1), 8)); inl = np.zeros(max(N, 1), np.uint8); res = np.zeros(max(P, 1), SIM3_RESULT)
        c = (cfg or Sim3SolverConfig())._c()
        self._check(self._L.orbx_sim3_ransac_batch(self._h, C.byref(c), C.c_int(P), _vp(off), _vp(p1), _vp(p2), _vp(sim3), _vp(inl), _vp(res)))
        return sim3[:P], [inl[off[p]:off[p + 1]].copy() for p in range(P)], res[:P]

    def compute_sim3_ransac_batch_device(self, offsets, points1, points2, max_n, cfg: "Sim3SolverConfig" = None):
        """Device-resident batch: torch CUDA tensors offsets [P+1] int32 (ascending from 0), points1 / points2 [N,3] f64.  Returns
        (sim3 [P,8] f64, inlier [N] u8, results [P,32] u8 — view as SIM3_RESULT); asynchronous on the handle's stream."""
        import torch
        P, N = int(offsets.shape[0]) - 1, int(points1.shape[0])
        dev = points1.device
        sim3 = torch.empty((max(P, 1), 8), dtype=torch.float64, device=dev)
        inl = torch.zeros(max(N, 1), dtype=torch.uint8, device=dev)
        res = torch.empty((max(P, 1), SIM3_RESULT.itemsize), dtype=torch.uint8, device=dev)
        c = (cfg or Sim3SolverConfig())._c()
        self._after_torch(offsets, points1, points2, sim3, inl, res)
        self._check(self._L.orbx_sim3_ransac_batch_device(self._h, C.byref(c), C.c_int(P), C.c_int(int(max_n)), _vp(offsets), _vp(points1),
                                                          _vp(points2), _vp(sim3), _vp(inl), _vp(res)))
        return sim3[:P], inl[:N], res[:P]

    @staticmethod
    def _loop_verify_unpack(B, co, ma, fm, pc, pl, inl, sim3, res):
        out = []
        for b in range(B):
            k0, nm, npair = int(co[b]), int(res[b]["n_matches"]), int(res[b]["n_pairs"])
            out.append(dict(status=int(res[b]["status"]), matches=ma[k0:k0 + nm].copy(), feature_matches=fm[k0:k0 + npair].copy(),
                            pts_current=pc[k0:k0 + npair].copy(), pts_loop=pl[k0:k0 + npair].copy(), inlier=inl[k0:k0 + npair].copy(),
                            sim3=sim3[b].copy(), record=res[b].copy(), stats=_rec_dict(res[b])))
        return out

    @staticmethod
    def _loop_verify_pack(pairs):
        """pairs: [(cur, loop), ...], each a dict with desc [n,32] u8, points_cam [n,3] f64, has_point [n] u8, pose_wc [7], optional
        node [n] u32; loop also kp (KEYPOINT)."""
        B = len(pairs)
        cd = [np.ascontiguousarray(c["desc"], np.uint8).reshape(-1, 32) for c, _ in pairs]
        ld = [np.ascontiguousarray(l["desc"], np.uint8).reshape(-1, 32) for _, l in pairs]
        co = np.zeros(B + 1, np.int32); co[1:] = np.cumsum([len(x) for x in cd])
        lo = np.zeros(B + 1, np.int32); lo[1:] = np.cumsum([len(x) for x in ld])
        N1, N2 = int(co[-1]), int(lo[-1])

        def cat(side, key, dt, shape, n):
            parts = [np.ascontiguousarray(p[side][key], dt).reshape(shape) for p in pairs]
            return np.concatenate(parts) if n else np.zeros((1,) + tuple(shape[1:]), dt)
        a = dict(cur_desc=cat(0, "desc", np.uint8, (-1, 32), N1), cur_pts=cat(0, "points_cam", np.float64, (-1, 3), N1),
                 cur_has=cat(0, "has_point", np.uint8, (-1,), N1), loop_kp=cat(1, "kp", KEYPOINT, (-1,), N2),
                 loop_desc=cat(1, "desc", np.uint8, (-1, 32), N2), loop_pts=cat(1, "points_cam", np.float64, (-1, 3), N2),
                 loop_has=cat(1, "has_point", np.uint8, (-1,), N2))
        # node ids travel as one array per side; a pair without them on either side gets brute force, which the library selects per
        # pair from both arrays being present — so a mixed batch is passed pair by pair through the keyframe form or split by the caller
        has_nodes = [c.get("node") is not None and l.get("node") is not None for c, l in pairs]
        if any(has_nodes) and not all(has_nodes):
            raise ValueError("the packed forms take node ids for every pair or for none; use KeyFrame.verify_loop_candidates for a mixed batch")
        cn = cat(0, "node", np.uint32, (-1,), N1) if all(has_nodes) and B else None
        ln = cat(1, "node", np.uint32, (-1,), N2) if all(has_nodes) and B else None
        cp = np.ascontiguousarray(np.stack([np.asarray(c["pose_wc"], np.float64).reshape(7) for c, _ in pairs]) if B else np.zeros((1, 7)))
        lp = np.ascontiguousarray(np.stack([np.asarray(l["pose_wc"], np.float64).reshape(7) for _, l in pairs]) if B else np.zeros((1, 7)))
        return a, cn, ln, co, lo, cp, lp

    def verify_loop_candidates(self, camera, pairs, cfg: "LoopVerifyConfig" = None):
        """verify_loop_candidate's numeric part (corrector.rs:127-195) for many (current, loop) keyframe pairs in one call, host
        arrays, one upload and one download.  pairs as _loop_verify_pack describes.  Returns one dict per pair: status (LOOP_*),
        matches (DMATCH), feature_matches [k,2] int32, pts_current / pts_loop [k,3], inlier [k] u8, sim3 [8], record
        (LOOP_VERIFY_RESULT), stats."""
        B = len(pairs)
        a, cn, ln, co, lo, cp, lp = self._loop_verify_pack(pairs)
        N1 = max(int(co[-1]), 1)
        ma = np.zeros(N1, DMATCH); fm = np.zeros((N1, 2), np.int32); pc = np.zeros((N1, 3)); pl = np.zeros((N1, 3)); inl = np.zeros(N1, np.uint8)
        sim3 = np.zeros((max(B, 1), 8)); res = np.zeros(max(B, 1), LOOP_VERIFY_RESULT)
        c = (cfg or LoopVerifyConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_verify_loop_candidates(
            self._h, C.byref(cam), C.byref(c), C.c_int(B), _vp(a["cur_desc"]), _vp(a["cur_pts"]), _vp(a["cur_has"]), _vp(cn), _vp(co), _vp(cp),
            _vp(a["loop_kp"]), _vp(a["loop_desc"]), _vp(a["loop_pts"]), _vp(a["loop_has"]), _vp(ln), _vp(lo), _vp(lp), _vp(ma), _vp(fm), _vp(pc),
            _vp(pl), _vp(inl), _vp(sim3), _vp(res)))
        return self._loop_verify_unpack(B, co, ma, fm, pc, pl, inl, sim3, res)

    def verify_loop_candidates_device(self, camera, cur_desc, cur_points_cam, cur_has_point, cur_offsets, cur_poses_wc, loop_kp, loop_desc,
                                      loop_points_cam, loop_has_point, loop_offsets, loop_poses_wc, cur_node=None, loop_node=None,
                                      cfg: "LoopVerifyConfig" = None):
        """Device-resident form: torch CUDA tensors cur_desc [N1,32] u8, cur_points_cam [N1,3] f64, cur_has_point [N1] u8, loop_kp [N2,7]
        f32 (KEYPOINT rows), loop_desc / loop_points_cam / loop_has_point likewise; HOST arrays cur_offsets / loop_offsets [B+1],
        cur_poses_wc / loop_poses_wc [B,7] and, optionally, cur_node [N1] / loop_node [N2] u32.  Returns a dict of tensors packed from
        cur_offsets[b]: matches [N1,16] u8 (DMATCH), feature_matches [N1,2] int32, pts_current / pts_loop [N1,3] f64, inlier [N1] u8;
        sim3 [B,8] f64, results [B,40] u8 (LOOP_VERIFY_RESULT).  Asynchronous on the handle's stream."""
        import torch
        co = np.ascontiguousarray(cur_offsets, np.int32).reshape(-1); lo = np.ascontiguousarray(loop_offsets, np.int32).reshape(-1)
        B = len(co) - 1
        N1 = max(int(co[-1]), 1)
        dev = cur_desc.device
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        o = dict(matches=mk((N1, DMATCH.itemsize), torch.uint8), feature_matches=mk((N1, 2), torch.int32), pts_current=mk((N1, 3), torch.float64),
                 pts_loop=mk((N1, 3), torch.float64), inlier=mk(N1, torch.uint8), sim3=mk((max(B, 1), 8), torch.float64),
                 results=mk((max(B, 1), LOOP_VERIFY_RESULT.itemsize), torch.uint8))
        cp = np.ascontiguousarray(cur_poses_wc, np.float64).reshape(-1, 7); lp = np.ascontiguousarray(loop_poses_wc, np.float64).reshape(-1, 7)
        cn = None if cur_node is None else np.ascontiguousarray(cur_node, np.uint32).reshape(-1)
        ln = None if loop_node is None else np.ascontiguousarray(loop_node, np.uint32).reshape(-1)
        c = (cfg or LoopVerifyConfig())._c(); cam = camera._c()
        self._after_torch(cur_desc, cur_points_cam, cur_has_point, loop_kp, loop_desc, loop_points_cam, loop_has_point, *o.values())
        self._check(self._L.orbx_verify_loop_candidates_device(
            self._h, C.byref(cam), C.byref(c), C.c_int(B), _vp(cur_desc), _vp(cur_points_cam), _vp(cur_has_point), _vp(cn), _vp(co), _vp(cp),
            _vp(loop_kp), _vp(loop_desc), _vp(loop_points_cam), _vp(loop_has_point), _vp(ln), _vp(lo), _vp(lp), _vp(o["matches"]),
            _vp(o["feature_matches"]), _vp(o["pts_current"]), _vp(o["pts_loop"]), _vp(o["inlier"]), _vp(o["sim3"]), _vp(o["results"])))
        return o

    def pose_inertial_optimization(self, camera, pose_wc, velocity, bias, prev_kf_pose_wc, prev_kf_velocity, preint, points3d, points2d,
                                   is_stereo, cfg: PoseInertialConfig = None) -> PoseInertialResult:
        """pose_inertial_optim.rs:94-216 on one problem: the initial state pose_wc [7] (T_wc), velocity [3], bias [6]; the previous
        keyframe's pose [7] and velocity [3]; preint [11] (delta_rot qw,qx,qy,qz | delta_vel | delta_pos | dt); points3d [n,3] f64 world
        points, points2d [n,2] (taken as f32, the keypoints' positions), is_stereo [n] bool."""
        return self.pose_inertial_optimization_batch(camera, [(pose_wc, velocity, bias, prev_kf_pose_wc, prev_kf_velocity, preint, points3d,
                                                               points2d, is_stereo)], cfg)[0]

    def pose_inertial_optimization_batch(self, camera, problems, cfg: PoseInertialConfig = None) -> List[PoseInertialResult]:
        """Many problems [(pose_wc, velocity, bias, prev_kf_pose_wc, prev_kf_velocity, preint, points3d, points2d, is_stereo), ...] in
        one call (one upload, one download); each result equals the single-problem call's byte for byte."""
        P = len(problems)
        states = [_pose_inertial_state(pr[:6]) for pr in problems]
        pts3d = [np.ascontiguousarray(pr[6], np.float64).reshape(-1, 3) for pr in problems]
        pts2d = [np.ascontiguousarray(pr[7], np.float32).reshape(-1, 2) for pr in problems]
        stereo = [np.ascontiguousarray(np.asarray(pr[8]).reshape(-1) != 0, np.uint8) for pr in problems]
        if any(len(a) != len(b) or len(a) != len(c) for a, b, c in zip(pts3d, pts2d, stereo)):
            raise ValueError("points3d, points2d and is_stereo differ in length")
        off = np.zeros(P + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in pts3d])
        N = int(off[-1])
        p3 = np.concatenate(pts3d) if N else np.zeros((1, 3), np.float64)
        p2 = np.concatenate(pts2d) if N else np.zeros((1, 2), np.float32)
        st = np.concatenate(stereo) if N else np.zeros(1, np.uint8)
        ins = [np.ascontiguousarray(np.stack([s[k] for s in states]) if P else np.zeros((1, w)), np.float64)
               for k, w in enumerate((7, 3, 6, 7, 3, 11))]
        poses = np.zeros((max(P, 1), 7)); vel = np.zeros((max(P, 1), 3)); bias = np.zeros((max(P, 1), 6))
        inl = np.zeros(max(N, 1), np.uint8)
        res = np.zeros(max(P, 1), POSE_INERTIAL_RESULT)
        c = (cfg or PoseInertialConfig())._c(); cam = camera._c()
        self._check(self._L.orbx_pose_inertial_batch(self._h, C.byref(cam), C.byref(c), C.c_int(P), _vp(off), _vp(p3), _vp(p2), _vp(st),
                                                     *[_vp(a) for a in ins], _vp(poses), _vp(vel), _vp(bias), _vp(inl), _vp(res)))
        return [PoseInertialResult(poses[p].copy(), vel[p].copy(), bias[p].copy(), int(res[p]["num_inliers"]), int(res[p]["num_observations"]),
                                   int(res[p]["iterations"]), inl[off[p]:off[p + 1]].astype(bool), int(res[p]["status"])) for p in range(P)]

    def pose_inertial_optimization_batch_device(self, camera, offsets, points3d, points2d, is_stereo, poses_wc, velocities, biases,
                                                prev_kf_poses_wc, prev_kf_velocities, preints, cfg: PoseInertialConfig = None):
        """Device-resident batch: torch CUDA tensors offsets [P+1] int32 (ascending from 0), points3d [N,3] f64, points2d [N,2] f32,
        is_stereo [N] u8, poses_wc [P,7], velocities [P,3], biases [P,6], prev_kf_poses_wc [P,7], prev_kf_velocities [P,3], preints
        [P,11] f64 — the layout of solve_pnp_ransac_batch_device, whose offsets / points and output poses can be passed straight in.
        Returns (poses [P,7], velocities [P,3], biases [P,6] f64, inlier [N] u8, results [P,16] u8 — view the bytes as
        POSE_INERTIAL_RESULT); asynchronous on the handle's stream."""
        import torch
        P, N = int(offsets.shape[0]) - 1, int(points3d.shape[0])
        dev = points3d.device
        poses = torch.empty((max(P, 1), 7), dtype=torch.float64, device=dev)
        vel = torch.empty((max(P, 1), 3), dtype=torch.float64, device=dev)
        bias = torch.empty((max(P, 1), 6), dtype=torch.float64, device=dev)
        inl = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
        res = torch.empty((max(P, 1), POSE_INERTIAL_RESULT.itemsize), dtype=torch.uint8, device=dev)
        ins = (offsets, points3d, points2d, is_stereo, poses_wc, velocities, biases, prev_kf_poses_wc, prev_kf_velocities, preints)
        c = (cfg or PoseInertialConfig())._c(); cam = camera._c()
        self._after_torch(*ins, poses, vel, bias, inl, res)
        self._check(self._L.orbx_pose_inertial_batch_device(self._h, C.byref(cam), C.byref(c), C.c_int(P), *[_vp(t) for t in ins], _vp(poses),
                                                            _vp(vel), _vp(bias), _vp(inl), _vp(res)))
        return poses[:P], vel[:P], bias[:P], inl[:N], res[:P]

    def search_for_triangulation(self, camera, kp1, desc1, mp1, stereo1, kp2, desc2, mp2, pose1_wc, pose2_wc, max_dist=50):
        """triangulation.rs:401-527.  Returns [(idx1, idx2)] as an int32 [n,2] array, ascending idx1."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT); kp2 = np.ascontiguousarray(kp2, KEYPOINT)
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        mp1 = np.ascontiguousarray(mp1, np.uint8); mp2 = np.ascontiguousarray(mp2, np.uint8)
        stereo1 = np.ascontiguousarray(stereo1, np.uint8)
        p1 = np.ascontiguousarray(pose1_wc, np.float64); p2 = np.ascontiguousarray(pose2_wc, np.float64)
        out = np.zeros((max(len(kp1), 1), 2), np.int32)
        n = C.c_int()
        cam = camera._c()
        self._check(self._L.orbx_search_for_triangulation(
            self._h, C.byref(cam), _vp(kp1), _vp(desc1), _vp(mp1), _vp(stereo1), C.c_int(len(kp1)), _vp(kp2), _vp(desc2),
            _vp(mp2), C.c_int(len(kp2)), _vp(p1), _vp(p2), C.c_uint(max_dist), _vp(out), C.byref(n)))
        return out[:n.value].copy()

    def search_for_triangulation_device(self, camera, kp1, desc1, mp1, stereo1, kp2, desc2, mp2, pose1_wc, pose2_wc, max_dist=50):
        """Device-resident form: torch CUDA tensors (kp [n,7] f32 as the extractor writes them, desc [n,32] u8, flags [n] u8).
        Returns (pairs [n1,2] int32 tensor, count [1] int32 tensor); asynchronous."""
        import torch
        n1, n2 = kp1.shape[0], kp2.shape[0]
        pairs = torch.empty((max(n1, 1), 2), dtype=torch.int32, device=kp1.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=kp1.device)
        p1 = np.ascontiguousarray(pose1_wc, np.float64); p2 = np.ascontiguousarray(pose2_wc, np.float64)
        cam = camera._c()
        self._after_torch(kp1, desc1, mp1, stereo1, kp2, desc2, mp2, pairs, cnt)
        self._check(self._L.orbx_search_for_triangulation_device(
            self._h, C.byref(cam), _vp(kp1), _vp(desc1), _vp(mp1), _vp(stereo1), C.c_int(n1), _vp(kp2), _vp(desc2), _vp(mp2), C.c_int(n2),
            _vp(p1), _vp(p2), C.c_uint(max_dist), _vp(pairs), _vp(cnt)))
        return pairs, cnt

    def triangulate_pairs(self, camera, kp1, points_cam1, has_point1, pose1_wc, kp2, points_cam2, has_point2, pose2_wc, pairs,
                          config: "TriangulationConfig" = None, is_inertial=False):
        """The pair loop of triangulate_from_neighbors (triangulation.rs:184-293) on host arrays.  Returns (points [n,3] f64,
        status [n] u16 = TRI_* | TRI_METHOD_* << 8).  points_cam / has_point may both be None (every point None)."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT); kp2 = np.ascontiguousarray(kp2, KEYPOINT)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        f = lambda a, t, shape: None if a is None else np.ascontiguousarray(a, t).reshape(shape)
        p1, h1, p2, h2 = f(points_cam1, np.float64, (-1, 3)), f(has_point1, np.uint8, -1), f(points_cam2, np.float64, (-1, 3)), f(has_point2, np.uint8, -1)
        q1 = np.ascontiguousarray(pose1_wc, np.float64).reshape(7); q2 = np.ascontiguousarray(pose2_wc, np.float64).reshape(7)
        n = len(pairs)
        pts = np.zeros((max(n, 1), 3)); st = np.zeros(max(n, 1), np.uint16)
        cam = camera._c(); cfg = (config or TriangulationConfig())._c()
        self._check(self._L.orbx_triangulate_pairs(self._h, C.byref(cam), C.byref(cfg), C.c_int(int(bool(is_inertial))), _vp(kp1), _vp(p1), _vp(h1),
                                                   C.c_int(len(kp1)), _vp(q1), _vp(kp2), _vp(p2), _vp(h2), C.c_int(len(kp2)), _vp(q2), _vp(pairs),
                                                   C.c_int(n), _vp(pts), _vp(st)))
        return pts[:n], st[:n]

    def triangulate_pairs_device(self, camera, kp1, points_cam1, has_point1, pose1_wc, kp2, points_cam2, has_point2, pose2_wc, pairs,
                                 config: "TriangulationConfig" = None, is_inertial=False):
        """Device-resident form: torch CUDA tensors (kp [n,7] f32 as the extractor writes them, points [n,3] f64, flags [n] u8, pairs
        [m,2] int32), poses on the host.  Returns (points [m,3] f64, status [m] int16 view of u16) tensors; asynchronous.  A pair
        whose index is out of range comes back TRI_BAD_INDEX."""
        import torch
        n1, n2, n = kp1.shape[0], kp2.shape[0], pairs.shape[0]
        pts = torch.zeros((max(n, 1), 3), dtype=torch.float64, device=pairs.device)
        st = torch.zeros(max(n, 1), dtype=torch.int16, device=pairs.device)
        q1 = np.ascontiguousarray(pose1_wc, np.float64).reshape(7); q2 = np.ascontiguousarray(pose2_wc, np.float64).reshape(7)
        cam = camera._c(); cfg = (config or TriangulationConfig())._c()
        self._after_torch(kp1, kp2, pairs, pts, st, *[t for t in (points_cam1, has_point1, points_cam2, has_point2) if t is not None])
        self._check(self._L.orbx_triangulate_pairs_device(self._h, C.byref(cam), C.byref(cfg), C.c_int(int(bool(is_inertial))), _vp(kp1),
                                                          _vp(points_cam1), _vp(has_point1), C.c_int(n1), _vp(q1), _vp(kp2), _vp(points_cam2),
                                                          _vp(has_point2), C.c_int(n2), _vp(q2), _vp(pairs), C.c_int(n), _vp(pts), _vp(st)))
        return pts[:n], st[:n]

    def fuse_search_device(self, camera, positions, mp_desc, kf_poses_wc, kf_feat_offset, kps, descs, radius_scale, desc_threshold=TH_LOW):
        """Device-resident form of fuse_search: torch CUDA tensors except the poses.  Returns (idx [P,T] int32, dist [P,T] int32 view of u32)."""
        import torch
        P_, T = positions.shape[0], len(kf_poses_wc)
        idx = torch.empty((P_, T), dtype=torch.int32, device=positions.device)
        dist = torch.empty((P_, T), dtype=torch.int32, device=positions.device)
        poses = np.ascontiguousarray(kf_poses_wc, np.float64).reshape(-1, 7)
        cam = camera._c()
        self._after_torch(positions, mp_desc, kf_feat_offset, kps, descs, idx, dist)
        self._check(self._L.orbx_fuse_search_device(self._h, C.byref(cam), _vp(positions), _vp(mp_desc), C.c_int(P_), _vp(poses),
                                                    _vp(kf_feat_offset), _vp(kps), _vp(descs), C.c_int(T), C.c_double(radius_scale),
                                                    C.c_uint(desc_threshold), _vp(idx), _vp(dist)))
        return idx, dist

    def search_for_triangulation_bow(self, camera, kp1, desc1, mp1, stereo1, node1, kp2, desc2, mp2, node2, pose1_wc, pose2_wc,
                                     max_dist=50):
        """triangulation.rs:541-658.  node1/node2: FeatureVector key per feature.  int32 [n,2], ascending idx1."""
        kp1 = np.ascontiguousarray(kp1, KEYPOINT); kp2 = np.ascontiguousarray(kp2, KEYPOINT)
        desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        mp1 = np.ascontiguousarray(mp1, np.uint8); mp2 = np.ascontiguousarray(mp2, np.uint8)
        stereo1 = np.ascontiguousarray(stereo1, np.uint8)
        node1 = np.ascontiguousarray(node1, np.uint32); node2 = np.ascontiguousarray(node2, np.uint32)
        p1 = np.ascontiguousarray(pose1_wc, np.float64); p2 = np.ascontiguousarray(pose2_wc, np.float64)
        out = np.zeros((max(len(kp1), 1), 2), np.int32)
        n = C.c_int()
        cam = camera._c()
        self._check(self._L.orbx_search_for_triangulation_bow(
            self._h, C.byref(cam), _vp(kp1), _vp(desc1), _vp(mp1), _vp(stereo1), _vp(node1), C.c_int(len(kp1)), _vp(kp2), _vp(desc2),
            _vp(mp2), _vp(node2), C.c_int(len(kp2)), _vp(p1), _vp(p2), C.c_uint(max_dist), _vp(out), C.byref(n)))
        return out[:n.value].copy()

    def fuse_search(self, camera, positions, mp_desc, kf_poses_wc, kf_feat_offset, kps, descs, radius_scale, desc_threshold=TH_LOW):
        """search_in_neighbors.rs:273-343 for every (map point, keyframe) pair -> (idx [P,T] int32, dist [P,T] uint32)."""
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        poses = np.ascontiguousarray(kf_poses_wc, np.float64).reshape(-1, 7)
        off = np.ascontiguousarray(kf_feat_offset, np.int32)
        kps = np.ascontiguousarray(kps, KEYPOINT); descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        P, T = len(positions), len(poses)
        if len(off) != T + 1 or len(mp_desc) != P or len(kps) != len(descs):
            raise ValueError("fuse_search: inconsistent array lengths")
        idx = np.full((P, T), -1, np.int32); dist = np.zeros((P, T), np.uint32)
        cam = camera._c()
        self._check(self._L.orbx_fuse_search(self._h, C.byref(cam), _vp(positions), _vp(mp_desc), C.c_int(P), _vp(poses), _vp(off),
                                             _vp(kps), _vp(descs), C.c_int(T), C.c_double(radius_scale), C.c_uint(desc_threshold),
                                             _vp(idx), _vp(dist)))
        return idx, dist

    @staticmethod
    def _refresh_inputs(positions, obs_start, obs_kf, obs_feat, mp_desc, normals):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        obs_kf = np.ascontiguousarray(obs_kf, np.int32).reshape(-1); obs_feat = np.ascontiguousarray(obs_feat, np.int32).reshape(-1)
        M = len(positions)
        mp_desc = np.array(mp_desc, np.uint8).reshape(-1, 32); normals = np.array(normals, np.float64).reshape(-1, 3)       # copies: in/out
        if len(obs_start) != M + 1 or len(mp_desc) != M or len(normals) != M or len(obs_kf) != len(obs_feat) or \
                (M > 0 and len(obs_kf) != int(obs_start[-1])):
            raise ValueError("refresh_map_points: inconsistent array lengths")
        out = MapPointRefresh(mp_desc, normals, np.zeros(M), np.zeros(M), np.zeros(M, MP_REFRESH_RECORD))
        return positions, obs_start, obs_kf, obs_feat, out

    def refresh_map_points(self, positions, obs_start, obs_kf, obs_feat, kf_poses_wc, kf_feat_offset, descs, scale_range, mp_desc,
                           normals) -> "MapPointRefresh":
        """Phase 4 of search_in_neighbors (search_in_neighbors.rs:139-150) for M map points: compute_distinctive_descriptors and
        update_map_point_normal_and_depth (orbx.h: orbx_refresh_map_points).  Point p owns observations obs_start[p]..obs_start[p+1] of
        obs_kf (index into the T keyframes) / obs_feat; keyframe t owns rows kf_feat_offset[t]..kf_feat_offset[t+1] of descs [F,32].
        scale_range = scale_factor ** (num_levels - 1).  mp_desc / normals are the points' current values (not modified)."""
        positions, obs_start, obs_kf, obs_feat, out = self._refresh_inputs(positions, obs_start, obs_kf, obs_feat, mp_desc, normals)
        poses = np.ascontiguousarray(kf_poses_wc, np.float64).reshape(-1, 7)
        off = np.ascontiguousarray(kf_feat_offset, np.int32).reshape(-1)
        descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
        T = len(poses)
        if len(off) != T + 1 or (T > 0 and len(descs) != int(off[-1])):
            raise ValueError("refresh_map_points: inconsistent keyframe arrays")
        self._check(self._L.orbx_refresh_map_points(self._h, C.c_int(len(positions)), _vp(positions), _vp(obs_start), _vp(obs_kf), _vp(obs_feat),
                                                    C.c_int(T), _vp(poses), _vp(off), _vp(descs), C.c_double(scale_range), _vp(out.mp_desc),
                                                    _vp(out.normals), _vp(out.min_distance), _vp(out.max_distance), _vp(out.records)))
        return out

    def refresh_map_points_device(self, positions, obs_start, obs_kf, obs_feat, n_obs, kf_poses_wc, kf_feat_offset, descs, scale_range,
                                  mp_desc, normals):
        """Device-resident form: torch CUDA tensors positions [M,3] f64, obs_start [M+1] / obs_kf / obs_feat int32, descs [F,32] u8,
        mp_desc [M,32] u8 and normals [M,3] f64 (both updated IN PLACE); HOST arrays kf_poses_wc [T,7] and kf_feat_offset [T+1];
        n_obs = obs_start[M] as the host knows it.  Returns a dict of tensors: min_distance / max_distance [M] f64, records [M,16] u8
        (MP_REFRESH_RECORD).  Asynchronous on the handle's stream."""
        import torch
        M = positions.shape[0]
        poses = np.ascontiguousarray(kf_poses_wc, np.float64).reshape(-1, 7)
        off = np.ascontiguousarray(kf_feat_offset, np.int32).reshape(-1)
        if len(off) != len(poses) + 1:
            raise ValueError("refresh_map_points_device: inconsistent keyframe arrays")
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=positions.device)
        o = dict(min_distance=mk(max(M, 1), torch.float64), max_distance=mk(max(M, 1), torch.float64),
                 records=mk((max(M, 1), MP_REFRESH_RECORD.itemsize), torch.uint8))
        self._after_torch(positions, obs_start, obs_kf, obs_feat, descs, mp_desc, normals, *o.values())
        self._check(self._L.orbx_refresh_map_points_device(self._h, C.c_int(M), C.c_int(int(n_obs)), _vp(positions), _vp(obs_start), _vp(obs_kf),
                                                           _vp(obs_feat), C.c_int(len(poses)), _vp(poses), _vp(off), _vp(descs),
                                                           C.c_double(scale_range), _vp(mp_desc), _vp(normals), _vp(o["min_distance"]),
                                                           _vp(o["max_distance"]), _vp(o["records"])))
        return {k: v[:M] for k, v in o.items()}

    def hamming_batch(self, a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
        if len(a) != len(b):
            raise ValueError("hamming_batch: row counts differ")
        out = np.zeros(len(a), np.uint32)
        self._check(self._L.orbx_hamming_batch(self._h, _vp(a), _vp(b), C.c_int(len(a)), _vp(out)))
        return out

    # ---- device-resident batch entry points (torch tensors on this handle's GPU) ----------------
    def alloc_batch_outputs(self, batch, cap_kp):
        import torch
        dev = torch.device("cuda", self.device)
        return dict(
            kp=torch.zeros((batch, 2, cap_kp, 7), dtype=torch.float32, device=dev),
            desc=torch.zeros((batch, 2, cap_kp, 32), dtype=torch.uint8, device=dev),
            nkp=torch.zeros((batch, 2), dtype=torch.int32, device=dev),
            matches=torch.zeros((batch, cap_kp, 4), dtype=torch.int32, device=dev),
            nmatches=torch.zeros((batch,), dtype=torch.int32, device=dev),
            points=torch.zeros((batch, cap_kp, 3), dtype=torch.float64, device=dev),
            has_point=torch.zeros((batch, cap_kp), dtype=torch.uint8, device=dev),
            cap_kp=cap_kp, batch=batch)

    def process_stereo_batch_device(self, images, out):
        """images: torch u8 [batch,2,h,w] on the GPU; out: alloc_batch_outputs().  Asynchronous."""
        b, two, hh, ww = images.shape
        assert two == 2 and images.is_contiguous() and b <= out["batch"]
        self._after_torch(images)
        self._check(self._L.orbx_process_stereo_batch_device(
            self._h, _vp(images), C.c_int(b), C.c_int(ww), C.c_int(hh), C.c_size_t(ww), _vp(out["kp"]),
            _vp(out["desc"]), _vp(out["nkp"]), C.c_int(out["cap_kp"]), _vp(out["matches"]),
            _vp(out["nmatches"]), _vp(out["points"]), _vp(out["has_point"])))

    def process_stereo_batch_host(self, images, out):
        """Pipelined host-buffer form: `images` and every tensor of `out` are (ideally pinned) CPU torch tensors with
        the layouts of alloc_batch_outputs.  Synchronous."""
        b, two, hh, ww = images.shape
        assert two == 2 and images.is_contiguous() and not images.is_cuda and b <= out["batch"]
        self._check(self._L.orbx_process_stereo_batch(
            self._h, _vp(images), C.c_int(b), C.c_int(ww), C.c_int(hh), C.c_size_t(ww), _vp(out["kp"]),
            _vp(out["desc"]), _vp(out["nkp"]), C.c_int(out["cap_kp"]), _vp(out["matches"]),
            _vp(out["nmatches"]), _vp(out["points"]), _vp(out["has_point"])))

    @staticmethod
    def alloc_host_outputs(batch, cap_kp, pin=True):
        import torch
        mk = lambda shape, dt: (torch.zeros(shape, dtype=dt).pin_memory() if pin else torch.zeros(shape, dtype=dt))
        return dict(kp=mk((batch, 2, cap_kp, 7), torch.float32), desc=mk((batch, 2, cap_kp, 32), torch.uint8),
                    nkp=mk((batch, 2), torch.int32), matches=mk((batch, cap_kp, 4), torch.int32),
                    nmatches=mk((batch,), torch.int32), points=mk((batch, cap_kp, 3), torch.float64),
                    has_point=mk((batch, cap_kp), torch.uint8), cap_kp=cap_kp, batch=batch)

    def extract_batch_device(self, images, out):
        """images: torch u8 [n,h,w]; writes out['kp'|'desc'|'nkp'] viewed as n slots."""
        n, hh, ww = images.shape
        assert images.is_contiguous() and n <= 2 * out["batch"]
        self._after_torch(images)
        self._check(self._L.orbx_extract_batch_device(
            self._h, _vp(images), C.c_int(n), C.c_int(ww), C.c_int(hh), C.c_size_t(ww), _vp(out["kp"]),
            _vp(out["desc"]), _vp(out["nkp"]), C.c_int(out["cap_kp"])))

    def stereo_match_batch_device(self, out, batch=None):
        b = batch or out["batch"]
        self._after_torch()
        self._check(self._L.orbx_stereo_match_batch_device(
            self._h, C.c_int(b), _vp(out["kp"]), _vp(out["desc"]), _vp(out["nkp"]), C.c_int(out["cap_kp"]),
            _vp(out["matches"]), _vp(out["nmatches"]), _vp(out["points"]), _vp(out["has_point"])))

    @staticmethod
    def unpack_batch_outputs(out, b):
        """Host copies of pair `b` in the reference's containers (synchronise first)."""
        nkp = out["nkp"][b].cpu().numpy()
        kp = out["kp"][b].cpu().numpy()
        desc = out["desc"][b].cpu().numpy()
        nm = int(out["nmatches"][b].item())
        res = []
        for s in range(2):
            k = np.ascontiguousarray(kp[s, :nkp[s]]).view(np.uint8).reshape(-1, 28).copy().view(KEYPOINT).reshape(-1)
            res.append(FeatureSet(k, desc[s, :nkp[s]].copy()))
        m = np.ascontiguousarray(out["matches"][b, :nm].cpu().numpy()).view(np.uint8).reshape(-1, 16).copy().view(DMATCH).reshape(-1)
        pts = out["points"][b, :nkp[0]].cpu().numpy()
        has = out["has_point"][b, :nkp[0]].cpu().numpy()
        return res[0], res[1], m, pts, has

    # ---- stage inspection -----------------------------------------------------------------------
    def debug_level(self, image_index, level, blurred=False):
        w = C.c_int(); hh = C.c_int()
        self._check(self._L.orbx_debug_read_level(self._h, C.c_int(image_index), C.c_int(level),
                                                  C.c_int(1 if blurred else 0), None, C.byref(w), C.byref(hh)))
        out = np.zeros((hh.value, w.value), np.uint8)
        self._check(self._L.orbx_debug_read_level(self._h, C.c_int(image_index), C.c_int(level),
                                                  C.c_int(1 if blurred else 0), _vp(out), C.byref(w), C.byref(hh)))
        return out

    def debug_candidates(self, image_index, level):
        n = C.c_int()
        self._check(self._L.orbx_debug_read_candidates(self._h, C.c_int(image_index), C.c_int(level), None,
                                                       C.c_int(0), C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self._check(self._L.orbx_debug_read_candidates(self._h, C.c_int(image_index), C.c_int(level), _vp(out),
                                                       C.c_int(len(out)), C.byref(n)))
        return out[:n.value].copy()

    # ---- BA -----------------------------------------------------------------------------------------
    def set_allreduce(self, fn):
        """fn(dev_ptr:int, n_doubles:int, hip_stream:int) -> None, or None to clear."""
        if fn is None:
            self._ar = None
            self._check(self._L.orbx_ba_set_allreduce(self._h, None, None))
            return

        def tramp(user, ptr, n, stream):
            try:
                fn(int(ptr), int(n), int(stream) if stream else 0)
                return 0
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return -1
        self._ar = ALLREDUCE_FN(tramp)
        self._check(self._L.orbx_ba_set_allreduce(self._h, self._ar, None))

    # ---- native RCCL collective of the point-partitioned solve (include/orbx.h) -----------------------------------
    @staticmethod
    def rccl_unique_id():
        """ncclGetUniqueId through the library (rank 0); hand the bytes to every rank, then init_rccl."""
        buf = (C.c_uint8 * 256)()
        n = load_library().orbx_rccl_unique_id(buf, C.c_size_t(256))
        if n <= 0:
            raise OrbxError(n, "ncclGetUniqueId failed")
        return bytes(buf[:n])

    def init_rccl(self, unique_id: bytes, rank: int, world: int):
        """ncclCommInitRank on this handle's device; collective over all ranks.  The library owns the communicator."""
        b = (C.c_uint8 * len(unique_id)).from_buffer_copy(unique_id)
        self._L.orbx_ba_init_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
        self._check(self._L.orbx_ba_init_rccl(self._h, b, C.c_size_t(len(unique_id)), C.c_int(rank), C.c_int(world)))

    def set_rccl_comm(self, comm_ptr):
        """Use an existing ncclComm_t (integer address), e.g. torch's; None / 0 clears."""
        self._L.orbx_ba_set_rccl_comm.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self._L.orbx_ba_set_rccl_comm(self._h, C.c_void_p(comm_ptr or None)))

    def has_collective(self):
        """Bit 0: an RCCL communicator is installed on the handle; bit 1: the all-reduce hook is (orbx_ba_has_collective)."""
        self._L.orbx_ba_has_collective.argtypes = [C.c_void_p]
        self._L.orbx_ba_has_collective.restype = C.c_int
        return int(self._L.orbx_ba_has_collective(self._h))

    def rccl_world(self):
        """(ranks, this rank) of the handle's RCCL communicator, from ncclCommCount / ncclCommUserRank (orbx_ba_rccl_world)."""
        n, r = C.c_int(0), C.c_int(-1)
        self._L.orbx_ba_rccl_world.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._L.orbx_ba_rccl_world.restype = C.c_int
        self._check(self._L.orbx_ba_rccl_world(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def ba_solve_visual(self, camera, cfg, poses_cw, fixed_cw, points, obs, should_stop=None):
        poses_cw = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 7)
        fixed_cw = np.ascontiguousarray(fixed_cw, np.float64).reshape(-1, 7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        # observations of dtype BA_OBS32 (ba_obs_to_obs32: the 16-byte form, f32 pixel coordinates as the reference's keypoints are) go through
        # orbx_ba_solve_visual_obs32: the same result bit for bit, half the upload
        o32 = getattr(obs, "dtype", None) == BA_OBS32
        obs = np.ascontiguousarray(obs, BA_OBS32 if o32 else BA_OBS)
        K, F, M, N = len(poses_cw), len(fixed_cw), len(pts), len(obs)
        out_wc = np.zeros((max(K, 1), 7))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        fn = self._L.orbx_ba_solve_visual_obs32 if o32 else self._L.orbx_ba_solve_visual
        rc = fn(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_cw),
                C.c_int(F), _vp(fixed_cw), C.c_int(M), _vp(pts), C.c_int(N),
                _vp(obs), cb, None, _vp(out_wc), C.byref(it), C.byref(e0), C.byref(e1))
        if rc in (ORBX_ERR_EMPTY,):
            return None                      # reference returns None, local_ba_lm.rs:923-925
        self._check(rc)
        return dict(poses_wc=out_wc[:K], points=pts, iterations=it.value, initial_error=e0.value,
                    final_error=e1.value)

    @staticmethod
    def pack_ba_windows(windows, obs32=False):
        """The same windows with every `obs` array a consecutive slice of ONE page-locked host buffer (window order): what a caller that
        owns its observation storage would hand to orbx_ba_solve_visual_batch — the copy engine then reads the observations where they lie
        and each half of the batch travels as one copy (orbx.h).  The buffer is a pinned torch tensor kept alive by the returned dicts."""
        import torch
        dt = BA_OBS32 if obs32 else BA_OBS
        if obs32:       # (coordinates that are not f32 values cannot take the 16-byte form: ba_obs_to_obs32 answers None)
            arrs = [w["obs"] if getattr(w["obs"], "dtype", None) == BA_OBS32 else ba_obs_to_obs32(np.ascontiguousarray(w["obs"], BA_OBS), len(np.asarray(w["fixed_cw"]).reshape(-1, 7))) for w in windows]
            if any(a is None for a in arrs):
                raise ValueError("pack_ba_windows(obs32=True): an observation's pixel coordinates are not f32 values")
        else:
            arrs = [np.ascontiguousarray(w["obs"], BA_OBS) for w in windows]
        total = sum(len(a) for a in arrs)
        buf = torch.empty(max(total, 1) * dt.itemsize, dtype=torch.uint8).pin_memory()
        flat = buf.numpy().view(dt)
        out, o = [], 0
        for w, a in zip(windows, arrs):
            flat[o:o + len(a)] = a
            d = dict(w); d["obs"] = flat[o:o + len(a)]; d["_pinned_obs"] = buf
            out.append(d); o += len(a)
        return out

    def ba_solve_visual_batch(self, camera, cfg, windows, should_stop=None):
        """orbx_ba_solve_visual_batch: `windows` = list of dicts with poses_cw, fixed_cw, points, obs (as ba_solve_visual).
        Returns one result dict per window (None where the reference returns None)."""
        keep = []
        arr = (_BaWindow * max(len(windows), 1))()
        # the in/out points and the output poses of ALL windows live in two arrays allocated once per call (a fresh 48 KB copy per
        # window cost 19 us each in page faults: 0.6 ms of a 5.6 ms call at 32 windows); the per-window results are views of them
        in_pts = [np.asarray(w["points"], np.float64).reshape(-1, 3) for w in windows]
        in_poses = [np.ascontiguousarray(w["poses_cw"], np.float64).reshape(-1, 7) for w in windows]
        all_pts = np.concatenate(in_pts) if in_pts else np.zeros((0, 3))
        all_out = np.zeros((sum(max(len(p), 1) for p in in_poses), 7))
        p_pts, p_out, o_pts, o_out = all_pts.ctypes.data, all_out.ctypes.data, 0, 0
        for i, w in enumerate(windows):
            poses_cw = in_poses[i]
            fixed_cw = np.ascontiguousarray(w["fixed_cw"], np.float64).reshape(-1, 7)
            obs = np.ascontiguousarray(w["obs"], BA_OBS)
            M, Ko = len(in_pts[i]), max(len(poses_cw), 1)
            pts = all_pts[o_pts:o_pts + M]; out_wc = all_out[o_out:o_out + Ko]
            keep.append((poses_cw, fixed_cw, pts, obs, out_wc))
            a = arr[i]
            a.K, a.F, a.M, a.N = len(poses_cw), len(fixed_cw), M, len(obs)
            a.poses_cw = poses_cw.ctypes.data; a.fixed_poses_cw = fixed_cw.ctypes.data; a.points = p_pts + 24 * o_pts
            a.obs = obs.ctypes.data; a.poses_wc_out = p_out + 56 * o_out
            o_pts += M; o_out += Ko
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        self._check(self._L.orbx_ba_solve_visual_batch(self._h, C.byref(cam), C.byref(c), C.c_int(len(windows)), arr, cb, None))
        res = []
        for i, (poses_cw, fixed_cw, pts, obs, out_wc) in enumerate(keep):
            a = arr[i]
            if a.status == ORBX_ERR_EMPTY:
                res.append(None)
                continue
            res.append(dict(poses_wc=out_wc[:len(poses_cw)], points=pts, iterations=a.iterations, initial_error=a.initial_error,
                            final_error=a.final_error))
        return res

    def prepare_ba_batch(self, windows, obs32=False):
        """A BaBatch: the windows laid out once the way orbx_ba_solve_visual_batch takes them (see BaBatch)."""
        return BaBatch(self, windows, obs32=obs32)

    def debug_ba_blocks(self, camera, cfg, poses_cw, fixed_cw, points, obs, global_mode=False):
        """orbx_debug_ba_blocks: (residual [N,2], A [N,2,6], B [N,2,3]) of every observation, from the solver's device functions."""
        poses_cw = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 7)
        fixed_cw = np.ascontiguousarray(fixed_cw, np.float64).reshape(-1, 7)
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, BA_OBS)
        out = np.zeros((max(len(obs), 1), 20))
        cam = camera._c(); c = cfg._c()
        self._check(self._L.orbx_debug_ba_blocks(self._h, C.byref(cam), C.byref(c), C.c_int(len(poses_cw)), _vp(poses_cw), C.c_int(len(fixed_cw)),
                                                 _vp(fixed_cw), C.c_int(len(pts)), _vp(pts), C.c_int(len(obs)), _vp(obs),
                                                 C.c_int(1 if global_mode else 0), _vp(out)))
        out = out[:len(obs)]
        return out[:, 0:2].copy(), out[:, 2:14].reshape(-1, 2, 6).copy(), out[:, 14:20].reshape(-1, 2, 3).copy()

    def debug_imu_residual(self, poses_wc, velocities, edge_kf, preint):
        """orbx_debug_imu_residual: compute_imu_residual (imu_factors.rs:66-103) of every edge, [E, 9], from the solver's device function."""
        poses_wc = np.ascontiguousarray(poses_wc, np.float64).reshape(-1, 7)
        vel = np.ascontiguousarray(velocities, np.float64).reshape(-1, 3)
        ek = np.ascontiguousarray(edge_kf, np.int32).reshape(-1, 2); pre = np.ascontiguousarray(preint, np.float64).reshape(-1, 11)
        if len(vel) != len(poses_wc) or len(pre) != len(ek):
            raise ValueError("debug_imu_residual: one velocity per pose and one preintegration per edge")
        out = np.zeros((max(len(ek), 1), 9))
        self._check(self._L.orbx_debug_imu_residual(self._h, C.c_int(len(poses_wc)), _vp(poses_wc), _vp(vel), C.c_int(len(ek)), _vp(ek), _vp(pre), _vp(out)))
        return out[:len(ek)]

    def ba_solve_inertial(self, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs, edge_kf, preint, should_stop=None):
        """solve_inertial_ba (local_inertial_ba.rs:1074-1275) on flat arrays; every keyframe of the window is returned."""
        poses_wc = np.ascontiguousarray(poses_wc, np.float64).reshape(-1, 7)
        vel = np.ascontiguousarray(velocities, np.float64).reshape(-1, 3); bias = np.ascontiguousarray(biases, np.float64).reshape(-1, 6)
        fixed_cw = np.ascontiguousarray(fixed_cw, np.float64).reshape(-1, 7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        obs = np.ascontiguousarray(obs, BA_OBS)
        ek = np.ascontiguousarray(edge_kf, np.int32).reshape(-1, 2); pre = np.ascontiguousarray(preint, np.float64).reshape(-1, 11)
        K, F, M, N, E = len(poses_wc), len(fixed_cw), len(pts), len(obs), len(ek)
        if len(vel) != K or len(bias) != K or len(pre) != E:
            raise ValueError("ba_solve_inertial: inconsistent array lengths")
        out_p = np.zeros((max(K, 1), 7)); out_v = np.zeros((max(K, 1), 3)); out_b = np.zeros((max(K, 1), 6))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        rc = self._L.orbx_ba_solve_inertial(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_wc), _vp(vel), _vp(bias), C.c_int(F),
                                            _vp(fixed_cw), C.c_int(M), _vp(pts), C.c_int(N), _vp(obs), C.c_int(E), _vp(ek), _vp(pre), cb,
                                            None, _vp(out_p), _vp(out_v), _vp(out_b), C.byref(it), C.byref(e0), C.byref(e1))
        if rc in (ORBX_ERR_EMPTY,):
            return None                      # reference returns None, local_inertial_ba.rs:1080-1082
        self._check(rc)
        return dict(poses_wc=out_p[:K], velocities=out_v[:K], biases=out_b[:K], points=pts, iterations=it.value,
                    initial_error=e0.value, final_error=e1.value)

    def _ba_solve_inertial_obs32(self, fn, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs32, N, edge_kf, preint, should_stop):
        poses_wc = np.ascontiguousarray(poses_wc, np.float64).reshape(-1, 7)
        vel = np.ascontiguousarray(velocities, np.float64).reshape(-1, 3); bias = np.ascontiguousarray(biases, np.float64).reshape(-1, 6)
        fixed_cw = np.ascontiguousarray(fixed_cw, np.float64).reshape(-1, 7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        ek = np.ascontiguousarray(edge_kf, np.int32).reshape(-1, 2); pre = np.ascontiguousarray(preint, np.float64).reshape(-1, 11)
        K, F, M, E = len(poses_wc), len(fixed_cw), len(pts), len(ek)
        if len(vel) != K or len(bias) != K or len(pre) != E:
            raise ValueError("ba_solve_inertial_obs32: inconsistent array lengths")
        out_p = np.zeros((max(K, 1), 7)); out_v = np.zeros((max(K, 1), 3)); out_b = np.zeros((max(K, 1), 6))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        rc = fn(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_wc), _vp(vel), _vp(bias), C.c_int(F), _vp(fixed_cw), C.c_int(M), _vp(pts), C.c_int(N),
                _vp(obs32), C.c_int(E), _vp(ek), _vp(pre), cb, None, _vp(out_p), _vp(out_v), _vp(out_b), C.byref(it), C.byref(e0), C.byref(e1))
        if rc in (ORBX_ERR_EMPTY,):
            return None                      # reference returns None, local_inertial_ba.rs:1080-1082
        self._check(rc)
        return dict(poses_wc=out_p[:K], velocities=out_v[:K], biases=out_b[:K], points=pts, iterations=it.value,
                    initial_error=e0.value, final_error=e1.value)

    def ba_solve_inertial_obs32(self, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs32, edge_kf, preint, should_stop=None):
        """ba_solve_inertial on the 16-byte observations (orbx_ba_solve_inertial_obs32): obs32 is a BA_OBS32 array whose mp_idx
        carries is_stereo as BA_OBS32_STEREO (ba_obs_to_obs32(..., inertial=True)).  Bit for bit ba_solve_inertial's result on
        the widened observations."""
        obs32 = np.ascontiguousarray(obs32, BA_OBS32)
        return self._ba_solve_inertial_obs32(self._L.orbx_ba_solve_inertial_obs32, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs32, len(obs32),
                                             edge_kf, preint, should_stop)

    def ba_solve_inertial_obs32_device(self, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs32, n_obs, edge_kf, preint, should_stop=None):
        """... with the observations in device memory (orbx_ba_solve_inertial_obs32_device): obs32 is a CUDA tensor whose first
        16 * n_obs bytes are BA_OBS32 records (map_collect_inertial_window_device's), 16-byte aligned."""
        N = int(n_obs)
        if N < 0 or N * BA_OBS32.itemsize > obs32.numel() * obs32.element_size():
            raise ValueError("obs32 holds fewer than n_obs records")
        self._after_torch(obs32)
        return self._ba_solve_inertial_obs32(self._L.orbx_ba_solve_inertial_obs32_device, camera, cfg, poses_wc, velocities, biases, fixed_cw, points, obs32, N,
                                             edge_kf, preint, should_stop)

    def ba_solve_global(self, camera, cfg, poses_cw, fixed_pose_cw, points, obs, should_stop=None):
        """solve_global_ba (global_ba.rs:184-418): every keyframe but the first is optimised."""
        poses_cw = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 7)
        fixed = np.ascontiguousarray(fixed_pose_cw, np.float64).reshape(7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        o32 = getattr(obs, "dtype", None) == BA_OBS32       # (as ba_solve_visual)
        obs = np.ascontiguousarray(obs, BA_OBS32 if o32 else BA_OBS)
        K, M, N = len(poses_cw), len(pts), len(obs)
        out_wc = np.zeros((max(K, 1), 7))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        fn = self._L.orbx_ba_solve_global_obs32 if o32 else self._L.orbx_ba_solve_global
        rc = fn(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_cw), _vp(fixed), C.c_int(M),
                _vp(pts), C.c_int(N), _vp(obs), cb, None, _vp(out_wc), C.byref(it), C.byref(e0),
                C.byref(e1))
        if rc in (ORBX_ERR_EMPTY,):
            return None                      # reference returns None, global_ba.rs:194-196
        self._check(rc)
        return dict(poses_wc=out_wc[:K], points=pts, iterations=it.value, initial_error=e0.value, final_error=e1.value)

    def ba_global_map_max_keyframes(self) -> int:
        """The most optimised keyframes ba_solve_global_map takes (orbx_ba_global_map_max_keyframes)."""
        return int(self._L.orbx_ba_global_map_max_keyframes())

    def _ba_solve_global_map(self, fn, camera, cfg, poses_cw, fixed_pose_cw, points, obs, N, should_stop):
        poses_cw = np.ascontiguousarray(poses_cw, np.float64).reshape(-1, 7)
        fixed = np.ascontiguousarray(fixed_pose_cw, np.float64).reshape(7)
        pts = np.array(points, np.float64, copy=True).reshape(-1, 3)
        K, M = len(poses_cw), len(pts)
        out_wc = np.zeros((max(K, 1), 7))
        it, e0, e1 = _solve_outs()
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        rc = fn(self._h, C.byref(cam), C.byref(c), C.c_int(K), _vp(poses_cw), _vp(fixed), C.c_int(M), _vp(pts), C.c_int(N), _vp(obs), cb, None, _vp(out_wc),
                C.byref(it), C.byref(e0), C.byref(e1))
        if rc in (ORBX_ERR_EMPTY,):
            return None                      # reference returns None, global_ba.rs:194-196
        self._check(rc)
        return dict(poses_wc=out_wc[:K], points=pts, iterations=it.value, initial_error=e0.value, final_error=e1.value)

    def ba_solve_global_map(self, camera, cfg, poses_cw, fixed_pose_cw, points, obs, should_stop=None):
        """ba_solve_global for a whole map (orbx_ba_solve_global_map[_obs32]): the same arguments, semantics and result dict, on the
        path that takes up to ba_global_map_max_keyframes() optimised keyframes.  obs is a BA_OBS or a BA_OBS32 array."""
        o32 = getattr(obs, "dtype", None) == BA_OBS32
        obs = np.ascontiguousarray(obs, BA_OBS32 if o32 else BA_OBS)
        fn = self._L.orbx_ba_solve_global_map_obs32 if o32 else self._L.orbx_ba_solve_global_map
        return self._ba_solve_global_map(fn, camera, cfg, poses_cw, fixed_pose_cw, points, obs, len(obs), should_stop)

    def ba_solve_global_map_obs32(self, camera, cfg, poses_cw, fixed_pose_cw, points, obs32, should_stop=None):
        """ba_solve_global_map on the 16-byte observations (orbx_ba_solve_global_map_obs32); kf_idx -1 marks the fixed keyframe."""
        obs32 = np.ascontiguousarray(obs32, BA_OBS32)
        return self._ba_solve_global_map(self._L.orbx_ba_solve_global_map_obs32, camera, cfg, poses_cw, fixed_pose_cw, points, obs32, len(obs32), should_stop)

    def ba_solve_global_map_obs32_device(self, camera, cfg, poses_cw, fixed_pose_cw, points, obs32, n_obs, should_stop=None):
        """... with the observations in device memory (orbx_ba_solve_global_map_obs32_device): obs32 is a CUDA tensor whose first
        16 * n_obs bytes are BA_OBS32 records, 16-byte aligned.  Bit for bit the result for a host copy of the observations."""
        N = int(n_obs)
        if N < 0 or N * BA_OBS32.itemsize > obs32.numel() * obs32.element_size():
            raise ValueError("obs32 holds fewer than n_obs records")
        self._after_torch(obs32)
        return self._ba_solve_global_map(self._L.orbx_ba_solve_global_map_obs32_device, camera, cfg, poses_cw, fixed_pose_cw, points, obs32, N, should_stop)


class StereoProcessor:
    """stereo.rs:31-66.  `new` = the constructor; `process` takes two grayscale u8 images."""

    def __init__(self, camera: CameraModel, n_features: int, device: int = 0, max_w: int = 1920,
                 max_h: int = 1080):
        self.camera = camera
        self.handle = Handle(camera, n_features, device=device, max_w=max_w, max_h=max_h, max_batch=1)

    @classmethod
    def new(cls, camera: CameraModel, n_features: int, **kw):
        return cls(camera, n_features, **kw)

    def process(self, left, right, timestamp_ns: int) -> StereoFrame:
        kpL, dL, kpR, dR, m, pts, has = self.handle.process_stereo(left, right)
        return StereoFrame(FeatureSet(kpL, dL), FeatureSet(kpR, dR), m, pts, has, int(timestamp_ns))


_default_handle = None


def _handle():
    global _default_handle
    if _default_handle is None:
        from .synth import EUROC_CAMERA
        _default_handle = Handle(CameraModel(**EUROC_CAMERA), 2000)
    return _default_handle


def descriptor_distance(desc1, desc2) -> int:
    """stereo.rs:166-175 for one pair of 32-byte rows (computed on the GPU)."""
    return int(_handle().hamming_batch(np.asarray(desc1, np.uint8).reshape(1, 32),
                                       np.asarray(desc2, np.uint8).reshape(1, 32))[0])


def bf_match_crosscheck(query_descriptors, train_descriptors):
    """tracker.rs:1001-1010: BFMatcher::new(NORM_HAMMING, true).train_match(query, train)."""
    return _handle().hamming_match_crosscheck(query_descriptors, train_descriptors)


def solve_pnp_ransac_detailed(points3d, points2d, camera: CameraModel, prior=None) -> PnPResult:
    """pnp.rs:100-134: the reference's name and argument order (prior = T_wc, 7 doubles).  A prior is required: every reference call
    site passes one, and the prior-free (EPnP) path is not implemented."""
    if prior is None:
        raise ValueError("solve_pnp_ransac_detailed needs a prior pose (the prior-free solver is not implemented)")
    return _handle().solve_pnp_ransac_detailed(camera, points3d, points2d, prior)


def solve_pnp_ransac(points3d, points2d, camera: CameraModel, prior=None) -> np.ndarray:
    """pnp.rs:29-97: the pose (T_wc, 7 doubles) alone."""
    return solve_pnp_ransac_detailed(points3d, points2d, camera, prior).pose


def track_with_reference_kf(frame_keypoints, frame_descriptors, kf_descriptors, kf_positions, kf_valid, camera: CameraModel, pose,
                            min_correspondences=4):
    """tracker.rs:992-1064: the frame against its reference keyframe — cross-checked brute-force matching (query = keyframe
    feature), the matches whose keyframe feature has a live map point (kf_valid[i] = 1, position kf_positions[i]) gathered in
    match order, PnP-RANSAC from `pose` (self.pose, T_wc).  Returns the pose, or None where the reference does (fewer than
    min_correspondences correspondences, :1051).  min_correspondences below 4 is refused, as the library refuses it."""
    if int(min_correspondences) < 4:
        raise OrbxError(ORBX_ERR_INVALID, "track_with_reference_kf: min_correspondences must be at least 4 (tracker.rs:1051; PnP's own minimum)")
    r = _handle().track_reference(camera, [(frame_keypoints, frame_descriptors, kf_descriptors, kf_positions, kf_valid, pose)],
                                  min_correspondences)[0]
    return r.pose_or_none()


def compute_sim3_ransac(points1, points2, config: Sim3SolverConfig = None) -> Optional[Sim3Result]:
    """sim3_solver.rs:63-145: the Sim3 S with points2 ~ S points1, or None where the reference returns None."""
    sim3, inl, res = _handle().compute_sim3_ransac_batch([(points1, points2)], config)
    if int(res[0]["status"]) != SIM3_OK:
        return None
    return Sim3Result(sim3[0].copy(), np.flatnonzero(inl[0]), int(res[0]["n_inliers"]), float(res[0]["mse"]), _rec_dict(res[0]))


def compute_sim3_from_matches(points1, points2, fix_scale: bool) -> Optional[Sim3Result]:
    """sim3_solver.rs:318-328: the default configuration with fix_scale set"""
    return compute_sim3_ransac(points1, points2, Sim3SolverConfig(fix_scale=fix_scale))


def verify_loop_candidate(current_kf, loop_kf, camera: CameraModel, current_kf_id=0, loop_kf_id=0, config: LoopVerifyConfig = None,
                          handle: "Handle" = None) -> Optional[VerifiedLoop]:
    """corrector.rs:116-204 for one candidate.  current_kf / loop_kf: dicts as Handle.verify_loop_candidates takes them, optionally
    with map_points (a sequence of ids or None per feature).  None where the reference returns None."""
    r = (handle or _handle()).verify_loop_candidates(camera, [(current_kf, loop_kf)], config)[0]
    if r["status"] != LOOP_OK:
        return None
    cm, lm = current_kf.get("map_points"), loop_kf.get("map_points")
    mmp = []
    if cm is not None and lm is not None:
        mmp = [(int(cm[i]), int(lm[j])) for i, j in r["feature_matches"] if cm[i] is not None and lm[j] is not None and cm[i] >= 0 and lm[j] >= 0]
    return VerifiedLoop(int(current_kf_id), int(loop_kf_id), r["sim3"], mmp, r["feature_matches"], r["inlier"].astype(bool), r["stats"])


def pose_inertial_optimization(initial_pose, initial_velocity, initial_bias, prev_kf_pose, prev_kf_velocity, prev_kf_bias, preintegrated,
                               observations, camera: CameraModel, config: PoseInertialConfig = None) -> PoseInertialResult:
    """pose_inertial_optim.rs:94-216 in the reference's argument order.  Poses T_wc (7 doubles), biases [6] (gyro, accel), preintegrated
    [11] (delta_rot qw,qx,qy,qz | delta_vel | delta_pos | dt); observations = (points3d [n,3], points2d [n,2], is_stereo [n]) — the
    PoseObservation fields uv / point_world / is_stereo as arrays.  prev_kf_bias is accepted and ignored, as in the reference."""
    del prev_kf_bias
    points3d, points2d, is_stereo = observations
    return _handle().pose_inertial_optimization(camera, initial_pose, initial_velocity, initial_bias, prev_kf_pose, prev_kf_velocity,
                                                preintegrated, points3d, points2d, is_stereo, config)


@dataclass
class VisualObservation:
    """local_ba_lm.rs:68-78"""
    kf_id: int
    mp_id: int
    observed_uv: tuple
    is_kf_optimized: bool


@dataclass
class VisualBAProblemData:
    """local_ba_lm.rs:48-65.  Poses are 7-vectors (qw,qx,qy,qz,tx,ty,tz), T_cw."""
    local_kf_poses: Dict[int, np.ndarray]
    local_mp_positions: Dict[int, np.ndarray]
    fixed_kf_poses: Dict[int, np.ndarray]
    anchor_kf_id: int
    observations: List[VisualObservation]
    optimized_kf_ids: List[int]
    mp_ids: List[int]


@dataclass
class VisualBAResultData:
    """local_ba_lm.rs:81-93.  optimized_poses are T_wc."""
    optimized_poses: Dict[int, np.ndarray] = field(default_factory=dict)
    optimized_points: Dict[int, np.ndarray] = field(default_factory=dict)
    iterations: int = 0
    initial_error: float = 0.0
    final_error: float = 0.0


@dataclass
class MapLocalBAResult(VisualBAResultData):
    """Handle.map_local_ba's result: VisualBAResultData with optimized_poses keyed by position in the call's keyframe list and
    optimized_points keyed by slot, plus the window itself: local_kf [1+max_covisible] (-1 padded), counts (K, F, M, N), and the
    points as arrays in the window's order (list_slot [M], points [M,3])."""
    local_kf: np.ndarray = None
    counts: np.ndarray = None
    list_slot: np.ndarray = None
    points: np.ndarray = None


def flatten_ba_problem(problem: VisualBAProblemData):
    """The id -> index re-keying of local_ba_lm.rs:928-987 (what the Rust shim does before the FFI
    call): observations whose map point is unknown are dropped (:947), an optimised-flagged
    observation whose keyframe is not in optimized_kf_ids, or a fixed one whose id is not in
    fixed_kf_poses, falls back to the identity pose (:569)."""
    kf_idx = {k: i for i, k in enumerate(problem.optimized_kf_ids)}
    mp_idx = {m: i for i, m in enumerate(problem.mp_ids)}
    fixed_ids = list(problem.fixed_kf_poses.keys())
    fixed_idx = {k: i for i, k in enumerate(fixed_ids)}
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    # :966-977 leaves the parameters of a keyframe without a pose at zero = identity
    poses = np.array([problem.local_kf_poses.get(k, ident) for k in problem.optimized_kf_ids],
                     np.float64).reshape(-1, 7)
    fixed = np.array([problem.fixed_kf_poses[k] for k in fixed_ids], np.float64).reshape(-1, 7)
    pts = np.array([problem.local_mp_positions.get(m, np.zeros(3)) for m in problem.mp_ids],
                   np.float64).reshape(-1, 3)
    rows = []
    for o in problem.observations:
        if o.mp_id not in mp_idx:
            continue
        if o.is_kf_optimized and o.kf_id in kf_idx:
            rows.append((kf_idx[o.kf_id], -1, mp_idx[o.mp_id], 0, o.observed_uv[0], o.observed_uv[1]))
        else:
            rows.append((-1, fixed_idx.get(o.kf_id, -1), mp_idx[o.mp_id], 0, o.observed_uv[0], o.observed_uv[1]))
    return poses, fixed, pts, np.array(rows, BA_OBS)


def solve_visual_ba(problem: VisualBAProblemData, camera: CameraModel, config: LocalBAConfigLM,
                    should_stop: Callable[[], bool], handle: Handle = None) -> Optional[VisualBAResultData]:
    """local_ba_lm.rs:912-1098."""
    h = handle or _handle()
    poses, fixed, pts, obs = flatten_ba_problem(problem)
    r = h.ba_solve_visual(camera, config, poses, fixed, pts, obs, should_stop)
    if r is None:
        return None
    return VisualBAResultData(
        {k: r["poses_wc"][i] for i, k in enumerate(problem.optimized_kf_ids)},
        {m: r["points"][i] for i, m in enumerate(problem.mp_ids)},
        r["iterations"], r["initial_error"], r["final_error"])


class KeyFrame:
    """orbx_keyframe: NewKeyFrameMsg (system/messages.rs:19-51) with keypoints, descriptors, stereo points and map-point flags
    resident on the GPU.  Built from the device outputs of the extractor; feeds guided_match / search_for_triangulation /
    fuse_search without moving the features over PCIe."""

    def __init__(self, handle: "Handle", d_kp, d_desc, n, d_points_cam=None, d_has_point=None, keyframe_id=0, timestamp_ns=0,
                 pose_wc=(1.0, 0, 0, 0, 0, 0, 0)):
        self._handle = handle
        self._L = handle._L
        L = self._L
        L.orbx_keyframe_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                           C.c_void_p, C.c_void_p]
        L.orbx_keyframe_destroy.argtypes = [C.c_void_p]; L.orbx_keyframe_destroy.restype = None
        for name in ("orbx_keyframe_info", "orbx_keyframe_download"):
            getattr(L, name).argtypes = [C.c_void_p] * 5
        for name in ("orbx_keyframe_set_pose", "orbx_keyframe_set_map_points", "orbx_keyframe_get_map_points"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.orbx_keyframe_guided_match.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                                 C.c_int, C.c_void_p, C.c_void_p]
        L.orbx_keyframe_search_for_triangulation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
        L.orbx_keyframe_set_feature_nodes.argtypes = [C.c_void_p, C.c_void_p]
        L.orbx_keyframe_triangulate_from_neighbors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + \
            [C.c_void_p] * 6
        L.orbx_keyframe_fuse_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_uint,
                                                C.c_void_p, C.c_void_p]
        L.orbx_keyframe_get_map_point_slots.argtypes = [C.c_void_p, C.c_void_p]
        self._p = C.c_void_p()
        pose = np.ascontiguousarray(pose_wc, np.float64).reshape(7)
        handle._after_torch()
        handle._check(L.orbx_keyframe_create(handle._h, _vp(d_kp), _vp(d_desc), C.c_int(int(n)), _vp(d_points_cam), _vp(d_has_point),
                                             C.c_uint64(int(keyframe_id)), C.c_uint64(int(timestamp_ns)), _vp(pose), C.byref(self._p)))
        self.n = int(n)

    @classmethod
    def from_batch_outputs(cls, handle, out, pair, keyframe_id=0, timestamp_ns=0, pose_wc=(1.0, 0, 0, 0, 0, 0, 0)):
        """The LEFT feature set of stereo pair `pair` of alloc_batch_outputs() / process_stereo_batch_device (synchronise first:
        the keypoint count is read on the host; the features themselves never leave the device)."""
        n = int(out["nkp"][pair, 0].item())
        return cls(handle, out["kp"][pair, 0], out["desc"][pair, 0], n, out["points"][pair], out["has_point"][pair], keyframe_id, timestamp_ns, pose_wc)

    def set_pose(self, pose_wc):
        self._handle._check(self._L.orbx_keyframe_set_pose(self._p, _vp(np.ascontiguousarray(pose_wc, np.float64).reshape(7))))

    def set_map_points(self, mp_ids):
        """matched_map_points: iterable of ids or None."""
        a = np.array([-1 if m is None else int(m) for m in mp_ids], np.int64)
        assert len(a) == self.n
        self._handle._check(self._L.orbx_keyframe_set_map_points(self._p, _vp(a)))

    def set_map_point_slots(self, mp: "MapPointStore", slots):
        """The per-feature slot table [n] (int, -1 or None = no map point) against the resident store `mp`, kept in the keyframe's
        device block; slots=None clears it.  A CUDA tensor (int32 [n], e.g. a row of the tracker's matched_slot) goes through
        orbx_keyframe_set_map_point_slots_device: asynchronous, a value outside [-1, capacity) is stored as -1.  set_map_points and
        the ids are untouched."""
        if slots is None:
            self._handle._check(self._L.orbx_keyframe_set_map_point_slots(self._p, None, None))
            return
        if getattr(slots, "is_cuda", False):
            import torch
            if slots.dtype != torch.int32 or not slots.is_contiguous() or slots.numel() < self.n:
                raise ValueError("set_map_point_slots: a CUDA table is a contiguous int32 tensor of at least n entries")
            if slots.device.index != self._handle.device:
                raise ValueError("set_map_point_slots: the table lies on cuda:%s, the handle on cuda:%d" % (slots.device.index, self._handle.device))
            if self.n == 0:
                slots = torch.zeros(1, dtype=torch.int32, device=slots.device)     # (an empty tensor has no address)
            self._handle._after_torch(slots)
            self._handle._check(self._L.orbx_keyframe_set_map_point_slots_device(self._p, mp._p, _vp(slots)))
            return
        a = np.array([-1 if m is None else int(m) for m in slots], np.int32)
        assert len(a) == self.n
        self._handle._check(self._L.orbx_keyframe_set_map_point_slots(self._p, mp._p, _vp(a if self.n else np.zeros(1, np.int32))))

    def get_map_point_slots(self):
        """The slot table [n] int32 as it lies in device memory (orbx_keyframe_get_map_point_slots; every entry -1 without a table):
        what map_fuse / map_search_in_neighbors left, for the caller to apply to its ids.  Synchronous."""
        a = np.full(max(self.n, 1), -1, np.int32)
        self._handle._check(self._L.orbx_keyframe_get_map_point_slots(self._p, _vp(a)))
        return a[:self.n].copy()

    def map_points(self):
        a = np.zeros(max(self.n, 1), np.int64)
        self._handle._check(self._L.orbx_keyframe_get_map_points(self._p, _vp(a)))
        return [None if v < 0 else int(v) for v in a[:self.n]]

    def info(self):
        n = C.c_int(); kid = C.c_uint64(); ts = C.c_uint64(); pose = np.zeros(7)
        self._handle._check(self._L.orbx_keyframe_info(self._p, C.byref(n), C.byref(kid), C.byref(ts), _vp(pose)))
        return dict(n=n.value, keyframe_id=kid.value, timestamp_ns=ts.value, pose_wc=pose)

    def download(self):
        kp = np.zeros(max(self.n, 1), KEYPOINT); desc = np.zeros((max(self.n, 1), 32), np.uint8)
        pts = np.zeros((max(self.n, 1), 3)); has = np.zeros(max(self.n, 1), np.uint8)
        self._handle._check(self._L.orbx_keyframe_download(self._p, _vp(kp), _vp(desc), _vp(pts), _vp(has)))
        return kp[:self.n], desc[:self.n], pts[:self.n], has[:self.n]

    def guided_match(self, img_w, img_h, q_uv, q_desc, radius, mode):
        q_uv = np.ascontiguousarray(q_uv, np.float64).reshape(-1, 2); q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        nq = len(q_uv)
        idx = np.full(max(nq, 1), -1, np.int32); dist = np.zeros(max(nq, 1), np.uint32)
        self._handle._check(self._L.orbx_keyframe_guided_match(self._handle._h, self._p, float(img_w), float(img_h), _vp(q_uv), _vp(q_desc), nq,
                                                               float(radius), int(mode), _vp(idx), _vp(dist)))
        return idx[:nq], dist[:nq]

    def search_for_triangulation(self, camera, other: "KeyFrame", max_dist=50):
        pairs = np.zeros((max(self.n, 1), 2), np.int32); n = C.c_int()
        cam = camera._c()
        self._handle._check(self._L.orbx_keyframe_search_for_triangulation(self._handle._h, C.byref(cam), self._p, other._p, int(max_dist),
                                                                           _vp(pairs), C.byref(n)))
        return pairs[:n.value].copy()

    def set_feature_nodes(self, node):
        """The FeatureVector as one node id per feature (OrbVocabulary.transform_arrays' out_node; FEATURE_NODE_NONE = in no list);
        None clears it.  With nodes on both keyframes triangulate_from_neighbors searches by node (triangulation.rs:145)."""
        if node is None:
            self._handle._check(self._L.orbx_keyframe_set_feature_nodes(self._p, None))
            return
        a = np.ascontiguousarray(node, np.uint32).reshape(-1)
        assert len(a) == self.n
        self._handle._check(self._L.orbx_keyframe_set_feature_nodes(self._p, _vp(a)))

    def triangulate_from_neighbors(self, camera, neighbours, config: "TriangulationConfig" = None, is_inertial=False, cap=None):
        """triangulate_from_neighbors (triangulation.rs:71-308) with this keyframe as the current one and `neighbours` in the order
        get_neighbor_keyframes gave them: one library call.  Returns (neighbour [m] int32 index into `neighbours`, idx1 [m], idx2 [m],
        points [m,3] f64, TriangulationResult) in the reference's creation order; the caller then does create_map_point + the two
        associate calls per entry.  cap: room for the first try (default 1024; the call is repeated when more points were made)."""
        T = len(neighbours)
        arr = (C.c_void_p * max(T, 1))(*[k._p for k in neighbours])
        cam = camera._c(); cfg = (config or TriangulationConfig())._c()
        stats = np.zeros((max(T, 1), 4), np.int32)
        cap = 1024 if cap is None else int(cap)
        while True:
            nb = np.zeros(max(cap, 1), np.int32); i1 = np.zeros(max(cap, 1), np.int32); i2 = np.zeros(max(cap, 1), np.int32)
            pts = np.zeros((max(cap, 1), 3)); n = C.c_int()
            self._handle._check(self._L.orbx_keyframe_triangulate_from_neighbors(
                self._handle._h, C.byref(cam), C.byref(cfg), C.c_int(int(bool(is_inertial))), self._p, arr, C.c_int(T), C.c_int(cap), _vp(nb), _vp(i1),
                _vp(i2), _vp(pts), C.byref(n), _vp(stats)))
            if n.value <= cap:
                break
            cap = n.value
        m = n.value
        stats = stats[:T]
        res = TriangulationResult(m, T, int(stats[:, 1].sum()), int(stats[:, 2].sum()), int(stats[:, 3].sum()), stats)
        return nb[:m], i1[:m], i2[:m], pts[:m], res

    @staticmethod
    def verify_loop_candidates(handle, camera, current_kfs, loop_kfs, cfg: "LoopVerifyConfig" = None):
        """Handle.verify_loop_candidates on resident keyframes (features, stereo points, poses and FeatureVectors are the keyframes'
        own; a keyframe may be listed several times): only the results cross PCIe.  A pair uses the FeatureVector matcher iff both of
        its keyframes carry nodes (set_feature_nodes).  Returns the same list of dicts, byte for byte."""
        B = len(current_kfs)
        if len(loop_kfs) != B:
            raise ValueError("one loop keyframe per current keyframe")
        co = np.zeros(B + 1, np.int32); co[1:] = np.cumsum([k.n for k in current_kfs])
        N1 = max(int(co[-1]), 1)
        ma = np.zeros(N1, DMATCH); fm = np.zeros((N1, 2), np.int32); pc = np.zeros((N1, 3)); pl = np.zeros((N1, 3)); inl = np.zeros(N1, np.uint8)
        sim3 = np.zeros((max(B, 1), 8)); res = np.zeros(max(B, 1), LOOP_VERIFY_RESULT)
        ca = (C.c_void_p * max(B, 1))(*[k._p for k in current_kfs]); la = (C.c_void_p * max(B, 1))(*[k._p for k in loop_kfs])
        c = (cfg or LoopVerifyConfig())._c(); cam = camera._c()
        handle._after_torch()
        handle._check(handle._L.orbx_keyframe_verify_loop_candidates(handle._h, C.byref(cam), C.byref(c), C.c_int(B), ca, la, _vp(ma), _vp(fm),
                                                                     _vp(pc), _vp(pl), _vp(inl), _vp(sim3), _vp(res)))
        return Handle._loop_verify_unpack(B, co, ma, fm, pc, pl, inl, sim3, res)

    @staticmethod
    def fuse_search(handle, camera, positions, mp_desc, keyframes, radius_scale, desc_threshold=50):
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 3); mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        P, T = len(positions), len(keyframes)
        arr = (C.c_void_p * max(T, 1))(*[k._p for k in keyframes])
        idx = np.full((max(P, 1), max(T, 1)), -1, np.int32); dist = np.zeros((max(P, 1), max(T, 1)), np.uint32)
        cam = camera._c()
        handle._check(handle._L.orbx_keyframe_fuse_search(handle._h, C.byref(cam), _vp(positions), _vp(mp_desc), P, arr, T, float(radius_scale),
                                                          int(desc_threshold), _vp(idx), _vp(dist)))
        return idx[:P, :T], dist[:P, :T]

    @staticmethod
    def refresh_map_points(handle, keyframes, positions, obs_start, obs_kf, obs_feat, scale_range, mp_desc, normals) -> "MapPointRefresh":
        """Handle.refresh_map_points on resident keyframes: obs_kf indexes `keyframes`, whose descriptors and poses are their own;
        only the points, their observation lists and the results cross PCIe.  The same bytes as the packed form."""
        positions, obs_start, obs_kf, obs_feat, out = Handle._refresh_inputs(positions, obs_start, obs_kf, obs_feat, mp_desc, normals)
        T = len(keyframes)
        arr = (C.c_void_p * max(T, 1))(*[k._p for k in keyframes])
        handle._after_torch()
        handle._check(handle._L.orbx_keyframe_refresh_map_points(handle._h, C.c_int(len(positions)), _vp(positions), _vp(obs_start), _vp(obs_kf),
                                                                 _vp(obs_feat), arr, C.c_int(T), C.c_double(scale_range), _vp(out.mp_desc),
                                                                 _vp(out.normals), _vp(out.min_distance), _vp(out.max_distance), _vp(out.records)))
        return out

    def close(self):
        if self._p:
            self._L.orbx_keyframe_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            if self._handle._h:
                self.close()
        except Exception:
            pass


class MapPointStore:
    """orbx_map_points: map points resident on the GPU — per slot a position, a descriptor and a live byte.  capacity is fixed; the
    caller owns the id -> slot assignment.  All work is ordered on the handle's stream."""

    def __init__(self, handle: "Handle", capacity: int):
        self._handle = handle
        self._L = handle._L
        L = self._L
        L.orbx_map_points_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.orbx_map_points_destroy.argtypes = [C.c_void_p]; L.orbx_map_points_destroy.restype = None
        L.orbx_map_points_info.argtypes = [C.c_void_p] * 3
        for name in ("orbx_map_points_set", "orbx_map_points_set_device"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.orbx_map_points_erase.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.orbx_map_points_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.orbx_keyframe_set_map_point_slots.argtypes = [C.c_void_p] * 3
        self._p = C.c_void_p()
        handle._check(L.orbx_map_points_create(handle._h, int(capacity), C.byref(self._p)))
        self.capacity = int(capacity)

    @staticmethod
    def _slots(slots):
        a = np.ascontiguousarray(slots, np.int32).reshape(-1)
        return a, (a if len(a) else np.zeros(1, np.int32))

    def set(self, slots, positions=None, descriptors=None):
        """rows of positions [n,3] f64 / descriptors [n,32] u8 (host arrays; either may be None: the field stays) into slots [n]"""
        a, ap = self._slots(slots)
        po = None if positions is None else np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        de = None if descriptors is None else np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        if (po is not None and len(po) != len(a)) or (de is not None and len(de) != len(a)):
            raise ValueError("one row per slot")
        self._handle._check(self._L.orbx_map_points_set(self._p, _vp(ap), len(a), _vp(po), _vp(de)))

    def set_device(self, slots, positions=None, descriptors=None):
        """the same from CUDA tensors (positions [n,3] f64, descriptors [n,32] u8, contiguous); slots stays a host array.  Asynchronous."""
        a, ap = self._slots(slots)
        self._handle._after_torch(*[t for t in (positions, descriptors) if t is not None])
        self._handle._check(self._L.orbx_map_points_set_device(self._p, _vp(ap), len(a), _vp(positions), _vp(descriptors)))

    def erase(self, slots):
        a, ap = self._slots(slots)
        self._handle._check(self._L.orbx_map_points_erase(self._p, _vp(ap), len(a)))

    def download(self, slots=None):
        """(positions [n,3], descriptors [n,32], live [n]) of the listed slots (default: all).  Synchronous."""
        a, ap = self._slots(np.arange(self.capacity) if slots is None else slots)
        n = len(a)
        po = np.zeros((max(n, 1), 3)); de = np.zeros((max(n, 1), 32), np.uint8); li = np.zeros(max(n, 1), np.uint8)
        self._handle._check(self._L.orbx_map_points_download(self._p, _vp(ap), n, _vp(po), _vp(de), _vp(li)))
        return po[:n], de[:n], li[:n]

    def info(self):
        cap = C.c_int(); live = C.c_int()
        self._handle._check(self._L.orbx_map_points_info(self._p, C.byref(cap), C.byref(live)))
        return dict(capacity=cap.value, n_live=live.value)

    def close(self):
        if self._p:
            self._L.orbx_map_points_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            if self._handle._h:
                self.close()
        except Exception:
            pass


class BaBatch:
    """A batch of local-BA windows kept in the layout orbx_ba_solve_visual_batch takes — what a host that owns its window storage (the Rust
    crate behind INTEGRATION.md's shim) hands over without any marshalling: the orbx_ba_window array filled once, every window's
    observations consecutive slices of ONE page-locked buffer (the copy engine reads them where they lie, one copy per half of the batch),
    poses / fixed poses / points / output poses each one array.  solve() refreshes the in/out points from the initial ones and makes the
    call; Handle.ba_solve_visual_batch(list of dicts) is the ad-hoc form that builds all of this per call."""

    def __init__(self, handle, windows, obs32=False):
        """obs32: carry the observations in the 16-byte form orbx_ba_obs32 (half the upload; bit-identical results).  Needs every pixel
        coordinate to be exactly an f32, as the reference's are; raises ValueError otherwise."""
        import torch
        self._handle = handle
        dt = BA_OBS32 if obs32 else BA_OBS
        if obs32:
            obs = [ba_obs_to_obs32(w["obs"], len(np.asarray(w["fixed_cw"]).reshape(-1, 7))) for w in windows]
            if any(a is None for a in obs):
                raise ValueError("BaBatch(obs32=True): a pixel coordinate is not exactly representable as f32")
        else:
            obs = [np.ascontiguousarray(w["obs"], BA_OBS) for w in windows]
        self.obs32 = bool(obs32)
        self._obs_buf = torch.empty(max(sum(len(a) for a in obs), 1) * dt.itemsize, dtype=torch.uint8).pin_memory()
        self.obs = self._obs_buf.numpy().view(dt)
        self.poses = [np.ascontiguousarray(w["poses_cw"], np.float64).reshape(-1, 7) for w in windows]
        self.fixed = [np.ascontiguousarray(w["fixed_cw"], np.float64).reshape(-1, 7) for w in windows]
        pts = [np.asarray(w["points"], np.float64).reshape(-1, 3) for w in windows]
        self.points0 = np.concatenate(pts) if pts else np.zeros((0, 3))
        self.points = self.points0.copy()
        self.out = np.zeros((sum(max(len(p), 1) for p in self.poses), 7))
        self.arr = (_BaWindow * max(len(windows), 1))()
        self._views = []
        o_obs = o_pts = o_out = 0
        for i, a_obs in enumerate(obs):
            n, M, K = len(a_obs), len(pts[i]), len(self.poses[i])
            self.obs[o_obs:o_obs + n] = a_obs
            a = self.arr[i]
            a.K, a.F, a.M, a.N = K, len(self.fixed[i]), M, n
            a.poses_cw = self.poses[i].ctypes.data; a.fixed_poses_cw = self.fixed[i].ctypes.data
            a.points = self.points.ctypes.data + 24 * o_pts
            if obs32:
                a.obs = None; a.obs32 = self.obs.ctypes.data + BA_OBS32.itemsize * o_obs
            else:
                a.obs = self.obs.ctypes.data + BA_OBS.itemsize * o_obs; a.obs32 = None
            a.poses_wc_out = self.out.ctypes.data + 56 * o_out
            self._views.append((self.out[o_out:o_out + K], self.points[o_pts:o_pts + M]))
            o_obs += n; o_pts += M; o_out += max(K, 1)
        self.n = len(windows)

    def solve(self, camera, cfg, should_stop=None):
        """One orbx_ba_solve_visual_batch call.  Returns one dict per window (None where the reference returns None); `poses_wc` and `points`
        are views of the batch's own arrays, valid until the next solve()."""
        h = self._handle
        np.copyto(self.points, self.points0)
        cb = _stop_callback(should_stop)
        cam = camera._c(); c = cfg._c()
        h._check(h._L.orbx_ba_solve_visual_batch(h._h, C.byref(cam), C.byref(c), C.c_int(self.n), self.arr, cb, None))
        res = []
        for i in range(self.n):
            a = self.arr[i]
            if a.status == ORBX_ERR_EMPTY:
                res.append(None)
            else:
                res.append(dict(poses_wc=self._views[i][0], points=self._views[i][1], iterations=a.iterations, initial_error=a.initial_error,
                                final_error=a.final_error))
        return res


def covisibility_lists(kf_ids, best, n_best):
    """The covisibility lists of MapSnapshot from the device result: kf_ids [nkf] (the ids of the keyframes handed to
    map_covisibility, in that order, every one of them a query in the same order), best [nkf,n] / n_best [nkf] as returned.
    -> (cov_start int32 [nkf+1], cov_kf_id uint64 [ncov]): per keyframe its neighbours' ids, weight descending then position
    ascending."""
    ids = np.asarray(kf_ids, np.uint64).reshape(-1)
    best = np.asarray(best, np.int64).reshape(len(ids), -1)
    cnt = np.asarray(n_best, np.int64).reshape(-1)
    if len(cnt) != len(ids):
        raise ValueError("one best row per keyframe")
    start = np.zeros(len(ids) + 1, np.int32); start[1:] = np.cumsum(cnt)
    rows = [ids[best[k, :cnt[k]]] for k in range(len(ids))]
    return start, (np.concatenate(rows) if rows else np.zeros(0, np.uint64)).astype(np.uint64)


class MapSnapshot:
    """The map as flat arrays (CSR) — what the host side of local BA reads and writes; the same layout and the same stated
    orders as include/orbx_map.hpp (see there for why the reference's HashMap orders are replaced by stated ones).

      keyframes:  kf_ids u64[nkf], kf_bad u8[nkf], kf_pose_wc f64[nkf,7] (T_wc), kf_n_keypoints i32[nkf],
                  kf_feat_start i32[nkf+1], feat_mp_id i64[nfeat] (-1 = None), feat_uv f32[nfeat,2],
                  cov_start i32[nkf+1], cov_kf_id u64[ncov] (covisibility neighbours in the stated order)
      map points: mp_ids u64[nmp], mp_bad u8[nmp], mp_pos f64[nmp,3], mp_obs_start i32[nmp+1], mp_obs_kf_id u64[nobs]
      inertial branch (optional, default "no IMU"): kf_prev_id i64[nkf] (-1 = None), kf_velocity f64[nkf,3], kf_bias f64[nkf,6] (gyro, accel),
                  kf_has_preint u8[nkf], kf_preint f64[nkf,11] (delta_rot qw,qx,qy,qz | delta_vel | delta_pos | dt, from prev_kf),
                  feat_stereo u8[nfeat] (points_cam[i].is_some()), mp_obs_feat_idx i32[nobs], imu_initialized (Map::is_imu_initialized())
    """
    FIELDS = (("kf_ids", np.uint64), ("kf_bad", np.uint8), ("kf_pose_wc", np.float64), ("kf_n_keypoints", np.int32),
              ("kf_feat_start", np.int32), ("feat_mp_id", np.int64), ("feat_uv", np.float32), ("cov_start", np.int32),
              ("cov_kf_id", np.uint64), ("mp_ids", np.uint64), ("mp_bad", np.uint8), ("mp_pos", np.float64),
              ("mp_obs_start", np.int32), ("mp_obs_kf_id", np.uint64))
    INERTIAL_FIELDS = (("kf_prev_id", np.int64), ("kf_velocity", np.float64), ("kf_bias", np.float64), ("kf_has_preint", np.uint8),
                       ("kf_preint", np.float64), ("feat_stereo", np.uint8), ("mp_obs_feat_idx", np.int32))

    def __init__(self, imu_initialized=False, **arrays):
        for name, dt in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays[name], dt))
        self.kf_pose_wc = self.kf_pose_wc.reshape(-1, 7)
        self.feat_uv = self.feat_uv.reshape(-1, 2)
        self.mp_pos = self.mp_pos.reshape(-1, 3)
        nkf, nfeat, nobs = len(self.kf_ids), len(self.feat_mp_id), len(self.mp_obs_kf_id)
        default = dict(kf_prev_id=np.full(nkf, -1, np.int64), kf_velocity=np.zeros((nkf, 3)), kf_bias=np.zeros((nkf, 6)), kf_has_preint=np.zeros(nkf, np.uint8),
                       kf_preint=np.zeros((nkf, 11)), feat_stereo=np.zeros(nfeat, np.uint8), mp_obs_feat_idx=np.full(nobs, -1, np.int32))
        for name, dt in self.INERTIAL_FIELDS:
            setattr(self, name, np.ascontiguousarray(arrays.get(name, default[name]), dt))
        self.kf_velocity = self.kf_velocity.reshape(-1, 3); self.kf_bias = self.kf_bias.reshape(-1, 6); self.kf_preint = self.kf_preint.reshape(-1, 11)
        self.imu_initialized = bool(imu_initialized)
        self.build_index()

    def build_index(self):
        self._kf = {int(k): i for i, k in enumerate(self.kf_ids)}
        self._mp = {int(k): i for i, k in enumerate(self.mp_ids)}

    def to_bytes(self):
        """[22 x u64: 21 element counts, imu_initialized] then the arrays in FIELDS + INERTIAL_FIELDS order (tests/cpp/local_mapper_driver.cpp reads this)."""
        arrs = [getattr(self, n).reshape(-1) for n, _ in self.FIELDS + self.INERTIAL_FIELDS]
        return np.array([len(a) for a in arrs] + [1 if self.imu_initialized else 0], np.uint64).tobytes() + b"".join(a.tobytes() for a in arrs)

    # ---- local_ba_lm.rs:665-726 --------------------------------------------------------------------------------
    def _local_keyframes(self, current, max_cov):
        local = [int(current)]
        k = self._kf.get(int(current), -1)
        if k >= 0:
            s, e = int(self.cov_start[k]), int(self.cov_start[k + 1])
            for nid in self.cov_kf_id[s:min(e, s + max_cov)]:        # take(max_covisible) before the filter (:675)
                nb = self._kf.get(int(nid), -1)
                if nb >= 0 and not self.kf_bad[nb]:
                    local.append(int(nid))
        return local

    def _local_map_points(self, local):
        seen = {}
        for kid in local:
            k = self._kf.get(kid, -1)
            if k < 0:
                continue
            for mp_id in self.feat_mp_id[int(self.kf_feat_start[k]):int(self.kf_feat_start[k + 1])]:
                if mp_id >= 0:
                    j = self._mp.get(int(mp_id), -1)
                    if j >= 0 and not self.mp_bad[j]:
                        seen.setdefault(int(mp_id), True)
        return list(seen)

    def _fixed_keyframes(self, local, mp_ids):
        loc = set(local)
        seen = {}
        for mid in mp_ids:
            j = self._mp.get(mid, -1)
            if j < 0:
                continue
            for kid in self.mp_obs_kf_id[int(self.mp_obs_start[j]):int(self.mp_obs_start[j + 1])]:
                if int(kid) not in loc:
                    seen.setdefault(int(kid), True)
        return list(seen)

    def collect_visual_ba_data(self, current_kf_id, config: "LocalBAConfigLM" = None) -> Optional["VisualBAProblemData"]:
        """PHASE 1 = collect_visual_ba_data, local_ba_lm.rs:800-897."""
        config = config or LocalBAConfigLM()
        local = self._local_keyframes(current_kf_id, config.max_covisible_keyframes)
        if not local:
            return None
        mp_ids = self._local_map_points(local)
        if not mp_ids:
            return None
        fixed = self._fixed_keyframes(local, mp_ids)
        anchor, optimized = local[0], local[1:]
        pose = lambda kid: se3_inverse(self.kf_pose_wc[self._kf[kid]])
        local_kf_poses = {k: pose(k) for k in optimized if k in self._kf}
        fixed_kf_poses = {}
        if anchor in self._kf:
            fixed_kf_poses[anchor] = pose(anchor)
        for k in fixed:
            if k in self._kf:
                fixed_kf_poses[k] = pose(k)
        local_mp_positions = {m: self.mp_pos[self._mp[m]].copy() for m in mp_ids if m in self._mp}
        opt_set, mp_set = set(optimized), set(mp_ids)
        obs = []
        for kid in local + fixed:
            k = self._kf.get(kid, -1)
            if k < 0:
                continue
            s, e = int(self.kf_feat_start[k]), int(self.kf_feat_start[k + 1])
            nkp = int(self.kf_n_keypoints[k])
            for f in range(s, e):
                mp_id = int(self.feat_mp_id[f])
                if mp_id >= 0 and mp_id in mp_set and f - s < nkp:
                    obs.append(VisualObservation(kid, mp_id, (float(self.feat_uv[f, 0]), float(self.feat_uv[f, 1])), kid in opt_set))
        if not obs:
            return None
        return VisualBAProblemData(local_kf_poses, local_mp_positions, fixed_kf_poses, anchor, obs, optimized, mp_ids)

    # ---- local_inertial_ba.rs:366-429, :933-1072, :1289-1330 ----------------------------------------------------
    def _temporal_keyframes(self, current, window_size):
        ids = [int(current)]
        prev = int(self.kf_prev_id[self._kf[int(current)]]) if int(current) in self._kf else -1
        while len(ids) < window_size and prev >= 0:
            ids.append(prev)
            prev = int(self.kf_prev_id[self._kf[prev]]) if prev in self._kf else -1
        ids.reverse()                                                 # oldest first: the anchor
        return ids

    def _fixed_keyframes_inertial(self, opt, mp_ids):
        o = set(opt)
        seen = {}
        for mid in mp_ids:
            j = self._mp.get(mid, -1)
            if j < 0:
                continue
            for kid in self.mp_obs_kf_id[int(self.mp_obs_start[j]):int(self.mp_obs_start[j + 1])]:
                kid = int(kid)
                if kid not in o:
                    k = self._kf.get(kid, -1)
                    if k >= 0 and not self.kf_bad[k]:                 # (:419-423: checked here, not in the visual collect)
                        seen.setdefault(kid, True)
        return list(seen)

    def collect_inertial_ba_data(self, current_kf_id, config: "LocalInertialBAConfig" = None) -> Optional["InertialBAProblemData"]:
        """PHASE 1 = collect_inertial_ba_data, local_inertial_ba.rs:933-1072."""
        config = config or LocalInertialBAConfig()
        opt = self._temporal_keyframes(current_kf_id, config.window_size)
        if len(opt) < 2:
            return None
        mp_ids = self._local_map_points(opt)
        if not mp_ids:
            return None
        fixed = self._fixed_keyframes_inertial(opt, mp_ids)
        kf_poses, kf_vel, kf_bias = {}, {}, {}
        for kid in opt:
            k = self._kf.get(kid, -1)
            if k >= 0:
                kf_poses[kid] = self.kf_pose_wc[k].copy(); kf_vel[kid] = self.kf_velocity[k].copy(); kf_bias[kid] = self.kf_bias[k].copy()
        fixed_poses = {kid: se3_inverse(self.kf_pose_wc[self._kf[kid]]) for kid in fixed if kid in self._kf}
        if opt[0] in self._kf:
            fixed_poses[opt[0]] = se3_inverse(self.kf_pose_wc[self._kf[opt[0]]])
        mp_positions = {m: self.mp_pos[self._mp[m]].copy() for m in mp_ids if m in self._mp}
        opt_set, all_kf = set(opt), set(opt) | set(fixed)
        obs = []
        for mid in mp_ids:
            j = self._mp.get(mid, -1)
            if j < 0:
                continue
            for o in range(int(self.mp_obs_start[j]), int(self.mp_obs_start[j + 1])):
                kid = int(self.mp_obs_kf_id[o])
                k = self._kf.get(kid, -1)
                if kid not in all_kf or k < 0:
                    continue
                fi = int(self.mp_obs_feat_idx[o])
                s, e = int(self.kf_feat_start[k]), int(self.kf_feat_start[k + 1])
                if fi < 0 or fi >= int(self.kf_n_keypoints[k]) or s + fi >= e:       # keypoints.get(feat_idx) is Err
                    continue
                f = s + fi
                obs.append(InertialVisualObs(kid, mid, (float(self.feat_uv[f, 0]), float(self.feat_uv[f, 1])), bool(self.feat_stereo[f]),
                                             kid in opt_set and kid != opt[0]))
        edges = []
        for i in range(len(opt) - 1):
            kj = self._kf.get(opt[i + 1], -1)
            if kj >= 0 and self.kf_has_preint[kj] and self.kf_preint[kj, 10] > 0.0:
                edges.append(ImuEdgeData(opt[i], opt[i + 1], self.kf_preint[kj].copy()))
        return InertialBAProblemData(kf_poses, kf_vel, kf_bias, mp_positions, fixed_poses, obs, edges, opt, mp_ids)

    def apply_inertial_ba_results(self, result: "InertialBAResultData") -> int:
        """PHASE 3 = apply_inertial_ba_results, local_inertial_ba.rs:1289-1330: poses and points count, velocities and biases do not."""
        updated = 0
        for kid, pose in result.optimized_poses.items():
            k = self._kf.get(int(kid), -1)
            if k >= 0 and not self.kf_bad[k]:
                self.kf_pose_wc[k] = pose
                updated += 1
        for kid, v in result.optimized_velocities.items():
            k = self._kf.get(int(kid), -1)
            if k >= 0 and not self.kf_bad[k]:
                self.kf_velocity[k] = v
        for kid, b in result.optimized_biases.items():
            k = self._kf.get(int(kid), -1)
            if k >= 0 and not self.kf_bad[k]:
                self.kf_bias[k] = b
        for mid, pos in result.optimized_points.items():
            j = self._mp.get(int(mid), -1)
            if j >= 0 and not self.mp_bad[j]:
                self.mp_pos[j] = pos
                updated += 1
        return updated

    # ---- global_ba.rs:100-181, :421-443 ----------------------------------------------------------------------------
    def collect_global_ba_data(self) -> Optional["GlobalBAProblemData"]:
        """PHASE 1 = collect_global_ba_data, global_ba.rs:100-181.  Keyframes: not bad, ids ascending (:121), the first one fixed; map points:
        not bad and seen by ANY collected keyframe (:137), in the snapshot's order (the reference's is its HashMap's); observations keyframe by
        keyframe in ascending id, features in order."""
        kf_ids = sorted(int(k) for k, bad in zip(self.kf_ids, self.kf_bad) if not bad)
        if not kf_ids:
            return None
        kf_poses = {k: se3_inverse(self.kf_pose_wc[self._kf[k]]) for k in kf_ids}
        kf_set = set(kf_ids)
        mp_ids, mp_positions = [], {}
        for j, mid in enumerate(self.mp_ids):
            if self.mp_bad[j]:
                continue
            s, e = int(self.mp_obs_start[j]), int(self.mp_obs_start[j + 1])
            if not any(int(k) in kf_set for k in self.mp_obs_kf_id[s:e]):
                continue
            mp_ids.append(int(mid))
            mp_positions[int(mid)] = self.mp_pos[j].copy()
        if not mp_ids:
            return None
        mp_set = set(mp_ids)
        obs = []
        for kid in kf_ids:
            k = self._kf[kid]
            s, e = int(self.kf_feat_start[k]), int(self.kf_feat_start[k + 1])
            nkp = int(self.kf_n_keypoints[k])
            for f in range(s, e):
                mp_id = int(self.feat_mp_id[f])
                if mp_id >= 0 and mp_id in mp_set and f - s < nkp:
                    obs.append(GlobalBAObservation(kid, mp_id, (float(self.feat_uv[f, 0]), float(self.feat_uv[f, 1]))))
        if not obs:
            return None
        return GlobalBAProblemData(kf_poses, mp_positions, obs, kf_ids, mp_ids, kf_ids[0])

    def apply_global_ba_results(self, result: "GlobalBAResult") -> int:
        """PHASE 3 = apply_global_ba_results, global_ba.rs:421-443: the same silent skips as the local one; the fixed keyframe's pose is in the
        result too and counts."""
        return self.apply_visual_ba_results(result)

    def apply_visual_ba_results(self, result: "VisualBAResultData") -> int:
        """PHASE 3 = apply_visual_ba_results, local_ba_lm.rs:1112-1138: gone or bad entities are skipped silently."""
        updated = 0
        for kid, pose in result.optimized_poses.items():
            k = self._kf.get(int(kid), -1)
            if k >= 0 and not self.kf_bad[k]:
                self.kf_pose_wc[k] = pose
                updated += 1
        for mid, pos in result.optimized_points.items():
            j = self._mp.get(int(mid), -1)
            if j >= 0 and not self.mp_bad[j]:
                self.mp_pos[j] = pos
                updated += 1
        return updated

    # ---- search_in_neighbors.rs:93-102, :116-120, :141-143 --------------------------------------------------------
    def search_in_neighbors_affected(self, current_kf_id, neighbour_ids) -> List[int]:
        """The map points phase 4 of search_in_neighbors refreshes: the current keyframe's (:93-102), then the neighbours' (:116-120),
        as a set in first-seen order (:141-143; the reference's HashSet order is unspecified).  A current keyframe the snapshot does
        not hold: none (:100); a neighbour it does not hold is skipped (:118).  The ids are not looked up: a point that is gone is
        left out by collect_map_point_refresh, as both reference functions do nothing for it."""
        if self._kf.get(int(current_kf_id), -1) < 0:
            return []
        seen = {}
        for kid in [int(current_kf_id)] + [int(n) for n in neighbour_ids]:
            k = self._kf.get(kid, -1)
            if k < 0:
                continue
            for mp_id in self.feat_mp_id[int(self.kf_feat_start[k]):int(self.kf_feat_start[k + 1])]:
                if mp_id >= 0:
                    seen.setdefault(int(mp_id), True)
        return list(seen)

    def collect_map_point_refresh(self, mp_ids) -> "MapPointRefreshData":
        """The arrays of refresh_map_points for the given map points (those the snapshot holds, in order): positions, the observation
        lists as they stand in mp_obs_start / mp_obs_kf_id / mp_obs_feat_idx, and the distinct observing keyframes in first-seen
        order, which obs_kf indexes (-1 for a keyframe the snapshot does not hold: keyframes.get -> None)."""
        kept, pos, start, okf, ofeat, kf_ids, kf_at = [], [], [0], [], [], [], {}
        for mid in mp_ids:
            j = self._mp.get(int(mid), -1)
            if j < 0:
                continue
            kept.append(int(mid)); pos.append(self.mp_pos[j])
            for o in range(int(self.mp_obs_start[j]), int(self.mp_obs_start[j + 1])):
                kid = int(self.mp_obs_kf_id[o])
                if kid not in self._kf:
                    okf.append(-1)
                else:
                    if kid not in kf_at:
                        kf_at[kid] = len(kf_ids); kf_ids.append(kid)
                    okf.append(kf_at[kid])
                ofeat.append(int(self.mp_obs_feat_idx[o]) if o < len(self.mp_obs_feat_idx) else -1)
            start.append(len(okf))
        return MapPointRefreshData(kept, np.array(pos, np.float64).reshape(-1, 3), np.array(start, np.int32), np.array(okf, np.int32),
                                   np.array(ofeat, np.int32), kf_ids)


def local_bundle_adjustment(snapshot: MapSnapshot, kf_id, camera: "CameraModel", should_stop: Callable[[], bool] = None,
                            handle: "Handle" = None):
    """LocalMapper::local_bundle_adjustment (local_mapper.rs:334-410): the inertial branch (:343-375) once the map's IMU is
    initialised, else the visual one (:378-408); each collect -> solve (GPU, no lock) -> apply only if the solve ran an iteration
    (:363, :396).  Returns (updated | None where the reference returns early, result)."""
    if snapshot.imu_initialized:
        iconfig = LocalInertialBAConfig()
        iproblem = snapshot.collect_inertial_ba_data(kf_id, iconfig)
        if iproblem is None:
            return None, None
        iresult = solve_inertial_ba(iproblem, camera, iconfig, should_stop or (lambda: False), handle=handle)
        if iresult is None:
            return None, None
        return (snapshot.apply_inertial_ba_results(iresult) if iresult.iterations > 0 else 0), iresult
    config = LocalBAConfigLM()
    problem = snapshot.collect_visual_ba_data(kf_id, config)
    if problem is None:
        return None, None
    result = solve_visual_ba(problem, camera, config, should_stop or (lambda: False), handle=handle)
    if result is None:
        return None, None
    return (snapshot.apply_visual_ba_results(result) if result.iterations > 0 else 0), result


@dataclass
class GlobalBAObservation:
    """global_ba.rs:70-80"""
    kf_id: int
    mp_id: int
    observed_uv: tuple


@dataclass
class GlobalBAProblemData:
    """global_ba.rs:49-67.  Poses are 7-vectors (qw,qx,qy,qz,tx,ty,tz), T_cw."""
    kf_poses: Dict[int, np.ndarray]
    mp_positions: Dict[int, np.ndarray]
    observations: List[GlobalBAObservation]
    kf_ids: List[int]
    mp_ids: List[int]
    fixed_kf_id: int


@dataclass
class GlobalBAResult:
    """global_ba.rs:83-98.  optimized_poses are T_wc and include the fixed keyframe."""
    optimized_poses: Dict[int, np.ndarray] = field(default_factory=dict)
    optimized_points: Dict[int, np.ndarray] = field(default_factory=dict)
    iterations: int = 0
    initial_error: float = 0.0
    final_error: float = 0.0


def se3_inverse(pose7):
    """se3.rs:56-63 with nalgebra's quaternion-vector product (v + w t + q x t, t = 2 q x v)."""
    p = np.asarray(pose7, np.float64)
    w, x, y, z = p[0], -p[1], -p[2], -p[3]
    v = p[4:]
    t = np.array([2.0 * (y * v[2] - z * v[1]), 2.0 * (z * v[0] - x * v[2]), 2.0 * (x * v[1] - y * v[0])])
    c = np.array([y * t[2] - z * t[1], z * t[0] - x * t[2], x * t[1] - y * t[0]])
    return np.concatenate([[w, x, y, z], -(t * w + c + v)])


def flatten_global_ba_problem(problem: GlobalBAProblemData):
    """The id -> index re-keying of global_ba.rs:198-261: the fixed keyframe is removed from the parameter order,
    a keyframe without a pose starts at the identity, an observation of an unknown keyframe uses the identity pose
    (:649).  Returns (opt_ids, poses_cw, fixed_pose_cw, points, obs) or None where the reference returns None."""
    if len(problem.kf_ids) < 2 or len(problem.mp_ids) == 0 or problem.fixed_kf_id not in problem.kf_ids:
        return None
    fixed_pos = problem.kf_ids.index(problem.fixed_kf_id)
    opt_ids = [k for i, k in enumerate(problem.kf_ids) if i != fixed_pos]
    kf_to_param = {k: i for i, k in enumerate(opt_ids)}
    mp_to_param = {m: i for i, m in enumerate(problem.mp_ids)}
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    poses = np.array([problem.kf_poses.get(k, ident) for k in opt_ids], np.float64).reshape(-1, 7)
    fixed = np.asarray(problem.kf_poses.get(problem.fixed_kf_id, ident), np.float64)
    pts = np.array([problem.mp_positions.get(m, np.zeros(3)) for m in problem.mp_ids], np.float64).reshape(-1, 3)
    rows = []
    for o in problem.observations:
        if o.mp_id not in mp_to_param:
            raise ValueError("solve_global_ba: observation of a map point that is not in mp_ids (never produced by collect_global_ba_data)")
        if o.kf_id == problem.fixed_kf_id:
            rows.append((-1, 0, mp_to_param[o.mp_id], 0, o.observed_uv[0], o.observed_uv[1]))
        elif o.kf_id in kf_to_param:
            rows.append((kf_to_param[o.kf_id], -1, mp_to_param[o.mp_id], 0, o.observed_uv[0], o.observed_uv[1]))
        else:
            rows.append((-1, -1, mp_to_param[o.mp_id], 0, o.observed_uv[0], o.observed_uv[1]))
    return opt_ids, poses, fixed, pts, np.array(rows, BA_OBS)


def solve_global_ba(problem: GlobalBAProblemData, camera: CameraModel, config: GlobalBAConfig,
                    should_stop: Callable[[], bool], handle: Handle = None) -> Optional[GlobalBAResult]:
    """global_ba.rs:184-418."""
    flat = flatten_global_ba_problem(problem)
    if flat is None:
        return None
    opt_ids, poses, fixed, pts, obs = flat
    r = (handle or _handle()).ba_solve_global(camera, config, poses, fixed, pts, obs, should_stop)
    if r is None:
        return None
    out = {problem.fixed_kf_id: se3_inverse(fixed)}
    out.update({k: r["poses_wc"][i] for i, k in enumerate(opt_ids)})
    return GlobalBAResult(out, {m: r["points"][i] for i, m in enumerate(problem.mp_ids)}, r["iterations"], r["initial_error"],
                          r["final_error"])


def run_global_ba(snapshot: MapSnapshot, camera: CameraModel, config: GlobalBAConfig = None, running: Optional[list] = None,
                  handle: Handle = None) -> Optional[GlobalBAResult]:
    """run_global_ba (global_ba.rs:450-500): collect -> solve (should_stop = the running flag cleared by stop_global_ba, loop_closer.rs:285) ->
    apply, unconditionally (unlike local BA, which applies only when an iteration ran).  `running`: a one-element list standing in for the
    reference's AtomicBool — set on entry, cleared on every way out."""
    running = running if running is not None else [False]
    running[0] = True
    try:
        problem = snapshot.collect_global_ba_data()
        if problem is None:
            return None
        result = solve_global_ba(problem, camera, config or GlobalBAConfig(), lambda: not running[0], handle=handle)
        if result is None:
            return None
        snapshot.apply_global_ba_results(result)
        return result
    finally:
        running[0] = False


class OrbVocabulary:
    """vocabulary/mod.rs:83-94: the tree lives in device memory; transform runs on the GPU."""

    def __init__(self, handle: Handle, ptr):
        self._handle = handle
        self._v = ptr
        L = handle._L
        k, l, nn, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.orbx_vocab_info(self._v, C.byref(k), C.byref(l), C.byref(nn), C.byref(nw))
        self.k, self.l, self._n_nodes, self._n_words = k.value, l.value, nn.value, nw.value

    @classmethod
    def load_from_text(cls, path, handle: Handle = None):
        """mod.rs:117-211.  Raises OrbxError where the reference returns VocabularyError."""
        h = handle or _handle()
        v = C.c_void_p()
        h._check(h._L.orbx_vocab_load_text(h._h, str(path).encode(), C.byref(v)))
        return cls(h, v)

    @classmethod
    def from_nodes(cls, parent, is_leaf, desc, weight, k=10, l=6, handle: Handle = None):
        h = handle or _handle()
        parent = np.ascontiguousarray(parent, np.uint32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); weight = np.ascontiguousarray(weight, np.float64)
        v = C.c_void_p()
        h._check(h._L.orbx_vocab_create(h._h, C.c_int(len(parent)), _vp(parent), _vp(is_leaf), _vp(desc), _vp(weight), C.c_int(k),
                                        C.c_int(l), C.byref(v)))
        return cls(h, v)

    def params(self):
        return self.k, self.l

    def num_words(self):
        return self._n_words

    def num_nodes(self):
        return self._n_nodes

    def nodes(self):
        parent = np.zeros(self._n_nodes, np.uint32); leaf = np.zeros(self._n_nodes, np.uint8)
        desc = np.zeros((self._n_nodes, 32), np.uint8); weight = np.zeros(self._n_nodes, np.float64)
        self._handle._L.orbx_vocab_nodes(self._v, _vp(parent), _vp(leaf), _vp(desc), _vp(weight))
        return parent, leaf, desc, weight

    def transform_arrays(self, descriptors, levels_up=4):
        """Per descriptor: (word id, leaf node, FeatureVector key, leaf weight)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        word = np.zeros(n, np.uint32); leaf = np.zeros(n, np.uint32); node = np.zeros(n, np.uint32); w = np.zeros(n, np.float64)
        h = self._handle
        h._check(h._L.orbx_bow_transform(h._h, self._v, _vp(d), C.c_int(n), C.c_int(levels_up), _vp(word), _vp(leaf), _vp(node), _vp(w)))
        return word, leaf, node, w

    def vectors_arrays(self, descriptors, levels_up=4):
        """orbx_bow_vectors: the two maps of OrbVocabulary::transform accumulated ON THE DEVICE ->
        (bow_word [nb] ascending, bow_weight [nb] L1-normalised, fv_node [nf] ascending, fv_start [nf+1], fv_index [n]).
        Up to BOW_VECTORS_MAX = 8192 descriptors per call on the device; more: device descent + host accumulation, same result."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        if n > BOW_VECTORS_MAX:
            # orbx_bow_vectors sorts one call's descriptors in one workgroup's LDS (at most 8192 of them: four frames' worth).  Beyond
            # that the tree descent still runs on the GPU (orbx_bow_transform) and the two maps are accumulated here with the device
            # kernel's own orders: weights of a word added in feature order, the L1 norm in ascending word id.
            word, _leaf, node, w = self.transform_arrays(d, levels_up)
            order = np.argsort(word, kind="stable")
            bw, first = np.unique(word[order], return_index=True)
            bv = np.array([_seq_sum(w[order[a:b]]) for a, b in zip(first, list(first[1:]) + [n])], np.float64)
            norm = _seq_sum(bv)
            if norm > 0.0:
                bv = bv / norm
            forder = np.argsort(node, kind="stable")
            fn, ffirst = np.unique(node[forder], return_index=True)
            fs = np.concatenate([ffirst, [n]]).astype(np.int32)
            return bw.astype(np.uint32), bv, fn.astype(np.uint32), fs, forder.astype(np.int32)
        bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64); fn = np.zeros(max(n, 1), np.uint32)
        fs = np.zeros(n + 1, np.int32); fi = np.zeros(max(n, 1), np.int32); nb = C.c_int(); nf = C.c_int()
        h = self._handle
        h._L.orbx_bow_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        h._check(h._L.orbx_bow_vectors(h._h, self._v, _vp(d), n, int(levels_up), _vp(bw), _vp(bv), C.byref(nb), _vp(fn), _vp(fs), _vp(fi), C.byref(nf)))
        return bw[:nb.value], bv[:nb.value], fn[:nf.value], fs[:nf.value + 1], fi[:n]

    def vectors_device(self, d_desc, n, levels_up=4):
        """orbx_bow_vectors_device on descriptors already in device memory (a torch uint8 tensor [n, 32] on the handle's device, n <=
        BOW_VECTORS_MAX) -> dict of torch tensors left on the device: bow_word (int32 storage of the u32 ids), bow_weight, fv_node,
        fv_start, fv_index, counts (n_bow, n_fv).  Asynchronous on the handle's stream: nothing is read on the host, so the result can go
        straight into KeyFrameDatabase.add_device(id, r["bow_word"], r["bow_weight"], r["counts"], n)."""
        import torch
        h = self._handle
        n = int(n)
        dev = torch.device("cuda", h.device)
        m = max(n, 1)
        r = dict(bow_word=torch.empty(m, dtype=torch.int32, device=dev), bow_weight=torch.empty(m, dtype=torch.float64, device=dev),
                 fv_node=torch.empty(m, dtype=torch.int32, device=dev), fv_start=torch.empty(m + 1, dtype=torch.int32, device=dev),
                 fv_index=torch.empty(m, dtype=torch.int32, device=dev), counts=torch.zeros(2, dtype=torch.int32, device=dev))
        h._after_torch(d_desc, *r.values())
        h._L.orbx_bow_vectors_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        h._check(h._L.orbx_bow_vectors_device(h._h, self._v, _vp(d_desc), n, int(levels_up), _vp(r["bow_word"]), _vp(r["bow_weight"]),
                                              _vp(r["fv_node"]), _vp(r["fv_start"]), _vp(r["fv_index"]), _vp(r["counts"])))
        return r

    def transform(self, descriptors, levels_up=4):
        """mod.rs:296-325 -> (BowVector dict word -> weight, FeatureVector dict node -> [feature indices]); descent, accumulation
        and L1 normalisation on the GPU (the norm is summed in ascending word id: the reference sums in HashMap order)."""
        bw, bv, fn, fs, fi = self.vectors_arrays(descriptors, levels_up)
        bow = {int(k): float(v) for k, v in zip(bw, bv)}
        feat = {int(fn[i]): [int(x) for x in fi[fs[i]:fs[i + 1]]] for i in range(len(fn))}
        return bow, feat

    def transform_bow_only(self, descriptors):
        """mod.rs:330-356"""
        return self.transform(descriptors, 0)[0]

    @staticmethod
    def score(v1, v2):
        """mod.rs:357-374: 1 - 0.5 * |v1 - v2|_1 (orbx_bow_score; terms added in ascending word id)"""
        k1 = np.array(sorted(v1), np.uint32); k2 = np.array(sorted(v2), np.uint32)
        w1 = np.array([v1[int(k)] for k in k1], np.float64); w2 = np.array([v2[int(k)] for k in k2], np.float64)
        out = C.c_double()
        L = load_library()
        L.orbx_bow_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        rc = L.orbx_bow_score(_vp(k1), _vp(w1), len(k1), _vp(k2), _vp(w2), len(k2), C.byref(out))
        if rc != 0:
            raise OrbxError(rc, "orbx_bow_score: bad argument")
        return out.value

    def close(self):
        if self._v:
            self._handle._L.orbx_vocab_destroy(self._v)
            self._v = None

    def __del__(self):
        try:
            if self._handle._h:
                self.close()
        except Exception:
            pass


@dataclass
class LoopDetectorConfig:
    """detector.rs:17-46"""
    min_score_ratio: float = 0.75
    consistency_threshold: int = 3
    min_covisibles_for_threshold: int = 5
    max_covisibles_to_check: int = 10
    min_temporal_gap: int = 30

    def _c(self):
        return _LoopDetectorConfig(self.min_score_ratio, self.consistency_threshold, self.min_covisibles_for_threshold,
                                   self.max_covisibles_to_check, self.min_temporal_gap)


@dataclass
class LoopCandidate:
    """detector.rs:49-62.  loop_covisibles is map bookkeeping: the caller fills it (the searches return ids and scores)."""
    current_kf_id: int
    loop_kf_id: int
    bow_score: float
    loop_covisibles: list = field(default_factory=list)


class ConsistencyChecker:
    """detector.rs:68-167: a loop candidate counts once it was detected for consistency_threshold keyframes in a row.  Host code."""

    def __init__(self, config: LoopDetectorConfig = None):
        self.config = config or LoopDetectorConfig()
        self.history = deque()              # (keyframe id, set of candidate ids)
        self.consistent_counts = {}

    def add_and_check(self, kf_id, candidates):
        """:94-146 -> the consistent candidate with the largest score (the first of equals), or None."""
        candidate_set = set()
        for c in candidates:
            candidate_set.add(c.loop_kf_id)
            candidate_set.update(c.loop_covisibles)
        new_counts = {cid: self._region_count(cid) + 1 for cid in candidate_set}
        best = None
        for c in candidates:
            if new_counts.get(c.loop_kf_id, 0) >= self.config.consistency_threshold and (best is None or c.bow_score > best.bow_score):
                best = c
        self.history.append((kf_id, candidate_set))
        if len(self.history) > self.config.consistency_threshold + 2:
            self.history.popleft()
        self.consistent_counts = new_counts
        if best is not None:
            self.clear()
            return best
        return None

    def _region_count(self, candidate_id):
        return sum(1 for _kf, cs in self.history if candidate_id in cs)      # :149-160

    def clear(self):
        self.history.clear()
        self.consistent_counts = {}


def _bow_arrays(bow):
    """A BowVector as (ascending u32 word ids, f64 weights): from a dict word -> weight, or a (words, weights) pair kept as given."""
    if isinstance(bow, dict):
        k = np.array(sorted(bow), np.uint32)
        return k, np.array([bow[int(x)] for x in k], np.float64)
    w, v = bow
    w = np.ascontiguousarray(w, np.uint32).reshape(-1); v = np.ascontiguousarray(v, np.float64).reshape(-1)
    if len(w) != len(v):
        raise ValueError("a BowVector needs as many weights as words")
    return w, v


class KeyFrameDatabase:
    """orbx_kfdb: KeyFrameDatabase (atlas/keyframe_db.rs:36-95) with the BowVectors in device memory, and detect_loop_candidates
    (loop_closing/detector.rs:185-368) over it.  Ids are keyframe ids (u64); an entry also carries its map index and is_bad."""

    def __init__(self, handle: Handle = None):
        h = handle or _handle()
        self._handle = h
        L = self._L = h._L
        vp, i, u64 = C.c_void_p, C.c_int, C.c_uint64
        L.orbx_kfdb_create.argtypes = [vp, vp]
        L.orbx_kfdb_destroy.argtypes = [vp]; L.orbx_kfdb_destroy.restype = None
        L.orbx_kfdb_add.argtypes = [vp, u64, i, i, vp, vp, i]
        L.orbx_kfdb_add_device.argtypes = [vp, u64, i, i, vp, vp, vp, i]
        L.orbx_kfdb_erase.argtypes = [vp, u64]
        L.orbx_kfdb_set_bad.argtypes = [vp, u64, i]
        L.orbx_kfdb_size.argtypes = [vp, vp, vp]
        L.orbx_kfdb_compact.argtypes = [vp]
        L.orbx_kfdb_download.argtypes = [vp, u64, vp, vp, i, vp, vp, vp]
        L.orbx_kfdb_score.argtypes = [vp, i, vp, vp, i, vp, vp, i, vp]
        L.orbx_kfdb_detect_candidates.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, vp]
        L.orbx_kfdb_detect_loop_candidates.argtypes = [vp, vp, i, u64, vp, i, i, vp, vp, vp]
        L.orbx_kfdb_detect_loop_candidates_batch.argtypes = [vp, vp, i, i, vp, vp, vp, i, vp, vp, vp]
        self._p = C.c_void_p()
        h._check(L.orbx_kfdb_create(h._h, C.byref(self._p)))

    def add(self, kf_id, bow, map_idx=0, is_bad=False):
        """keyframe_db.rs:45-47; bow: dict word -> weight, or (ascending words, weights)."""
        w, v = _bow_arrays(bow)
        self._handle._check(self._L.orbx_kfdb_add(self._p, int(kf_id), int(map_idx), int(bool(is_bad)), _vp(w), _vp(v), len(w)))

    def add_device(self, kf_id, d_word, d_weight, d_count, max_n, map_idx=0, is_bad=False):
        """The outputs of orbx_bow_vectors_device (torch tensors or device addresses) straight in; no host synchronisation."""
        h = self._handle
        h._after_torch(*[t for t in (d_word, d_weight, d_count) if not isinstance(t, int)])
        h._check(self._L.orbx_kfdb_add_device(self._p, int(kf_id), int(map_idx), int(bool(is_bad)), _vp(d_word), _vp(d_weight), _vp(d_count), int(max_n)))

    def erase(self, kf_id):
        self._handle._check(self._L.orbx_kfdb_erase(self._p, int(kf_id)))

    def set_bad(self, kf_id, is_bad=True):
        self._handle._check(self._L.orbx_kfdb_set_bad(self._p, int(kf_id), int(bool(is_bad))))

    def sizes(self):
        """(live entries, table rows including tombstones)"""
        n, s = C.c_int(), C.c_int()
        self._handle._check(self._L.orbx_kfdb_size(self._p, C.byref(n), C.byref(s)))
        return n.value, s.value

    def __len__(self):
        return self.sizes()[0]

    def compact(self):
        self._handle._check(self._L.orbx_kfdb_compact(self._p))

    def download(self, kf_id):
        """-> (words, weights, map index, is_bad) of one entry, read back from the device."""
        w = np.zeros(KFDB_MAX_WORDS, np.uint32); v = np.zeros(KFDB_MAX_WORDS, np.float64)
        n, m, b = C.c_int(), C.c_int(), C.c_int()
        self._handle._check(self._L.orbx_kfdb_download(self._p, int(kf_id), _vp(w), _vp(v), KFDB_MAX_WORDS, C.byref(n), C.byref(m), C.byref(b)))
        return w[:n.value].copy(), v[:n.value].copy(), m.value, bool(b.value)

    def score(self, query, scoring=KFDB_SCORE_L1):
        """-> (ids ascending, scores) of the query against every entry."""
        w, v = _bow_arrays(query)
        cap = max(len(self), 1)
        ids = np.zeros(cap, np.uint64); sc = np.zeros(cap, np.float64); n = C.c_int()
        self._handle._check(self._L.orbx_kfdb_score(self._p, int(scoring), _vp(w), _vp(v), len(w), _vp(ids), _vp(sc), cap, C.byref(n)))
        return ids[:n.value], sc[:n.value]

    def detect_candidates(self, query, exclude_map=None, max_results=10):
        """keyframe_db.rs:58-94 -> (ids, map indices, scores), score descending."""
        w, v = _bow_arrays(query)
        cap = max(int(max_results), 1)
        ids = np.zeros(cap, np.uint64); maps = np.zeros(cap, np.int32); sc = np.zeros(cap, np.float64); n = C.c_int()
        self._handle._check(self._L.orbx_kfdb_detect_candidates(self._p, _vp(w), _vp(v), len(w), -1 if exclude_map is None else int(exclude_map),
                                                                int(max_results), _vp(ids), _vp(maps), _vp(sc), C.byref(n)))
        return ids[:n.value], maps[:n.value], sc[:n.value]

    def detect_loop_candidates(self, kf_id, connected, config: LoopDetectorConfig = None, scoring=KFDB_SCORE_L1, cap=64):
        """detector.rs:185-368 -> (ids, scores, total): the first min(total, cap) candidates, score descending."""
        ids, sc, cnt = self.detect_loop_candidates_batch([kf_id], [connected], config, scoring, cap, _single=True)
        m = max(min(int(cnt[0]), cap), 0)
        return ids[0, :m], sc[0, :m], int(cnt[0])

    def detect_loop_candidates_batch(self, kf_ids, connected_lists, config: LoopDetectorConfig = None, scoring=KFDB_SCORE_L1, cap=64, _single=False):
        """Q current keyframes in one call -> (ids [Q][cap], scores [Q][cap], counts [Q]); row q holds min(counts[q], cap) candidates."""
        cfg = (config or LoopDetectorConfig())._c()
        Q = len(kf_ids)
        cur = np.array([int(k) for k in kf_ids], np.uint64)
        off = np.zeros(Q + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in connected_lists])
        conn = np.array([int(x) for c in connected_lists for x in c], np.uint64)
        ids = np.zeros((Q, max(cap, 0)), np.uint64); sc = np.zeros((Q, max(cap, 0)), np.float64); cnt = np.zeros(max(Q, 1), np.int32)
        h = self._handle
        if _single:
            c1 = C.c_int()
            h._check(self._L.orbx_kfdb_detect_loop_candidates(self._p, C.byref(cfg), int(scoring), int(cur[0]), _vp(conn), len(conn), int(cap), _vp(ids),
                                                              _vp(sc), C.byref(c1)))
            cnt[0] = c1.value
        else:
            h._check(self._L.orbx_kfdb_detect_loop_candidates_batch(self._p, C.byref(cfg), int(scoring), Q, _vp(cur), _vp(off), _vp(conn), int(cap),
                                                                    _vp(ids), _vp(sc), _vp(cnt)))
        return ids, sc, cnt[:Q]

    def close(self):
        if self._p:
            self._L.orbx_kfdb_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            if self._handle._h:
                self.close()
        except Exception:
            pass


def png_decode_gray8(data: bytes):
    """cv::imread(IMREAD_GRAYSCALE) for the PNG subset EuRoC uses (host code in the library, no GPU)."""
    L = load_library()
    buf = np.frombuffer(data, np.uint8)
    w, h = C.c_int(), C.c_int()
    rc = L.orbx_png_decode_gray8(_vp(buf), C.c_size_t(len(buf)), None, C.c_size_t(0), C.byref(w), C.byref(h))
    if rc != 0:
        raise OrbxError(rc, "not a supported greyscale PNG")
    out = np.empty((h.value, w.value), np.uint8)
    rc = L.orbx_png_decode_gray8(_vp(buf), C.c_size_t(len(buf)), _vp(out), C.c_size_t(w.value), None, None)
    if rc != 0:
        raise OrbxError(rc, "damaged PNG")
    return out


class EurocDataset:
    """io/euroc.rs:54-132, the image side: cam0/cam1 lists, calibration, stereo pairs (host code, no GPU)."""

    def __init__(self, root):
        L = load_library()
        self._L = L
        self._d = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = L.orbx_euroc_open(str(root).encode(), C.byref(self._d), err, C.c_size_t(512))
        if rc != 0:
            self._d = None
            raise OrbxError(rc, err.value.decode())
        cam = _Camera(); kr = (C.c_double * 4)(); w, h = C.c_int(), C.c_int()
        L.orbx_euroc_calibration(self._d, C.byref(cam), kr, C.byref(w), C.byref(h))
        self.camera = CameraModel(cam.fx, cam.fy, cam.cx, cam.cy, cam.baseline)
        self.k_right = tuple(kr)
        self.width, self.height = w.value, h.value

    @classmethod
    def new(cls, root):
        return cls(root)

    def __len__(self):
        return self._L.orbx_euroc_len(self._d)

    def len(self):
        return len(self)

    def frame_timestamp(self, idx):
        ts = C.c_uint64()
        return ts.value if self._L.orbx_euroc_frame_timestamp(self._d, C.c_int(idx), C.byref(ts)) == 0 else None

    def read_pairs(self, first, count, out=None, threads=8):
        """[count, 2, h, w] u8, decoded by `threads` host threads; `out` may be a pinned buffer of that shape."""
        if out is None:
            out = np.empty((count, 2, self.height, self.width), np.uint8)
        rc = self._L.orbx_euroc_read_pairs(self._d, C.c_int(first), C.c_int(count), _vp(out), C.c_int(threads))
        if rc != 0:
            raise OrbxError(rc, self._L.orbx_euroc_last_error(self._d).decode())
        return out

    def stereo_pair(self, idx):
        """euroc.rs:100-132 -> (left, right, timestamp_ns)"""
        p = self.read_pairs(idx, 1, threads=2)
        return p[0, 0], p[0, 1], self.frame_timestamp(idx)

    def close(self):
        if self._d:
            self._L.orbx_euroc_close(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class InertialVisualObs:
    """local_inertial_ba.rs:64-77"""
    kf_id: int
    mp_id: int
    observed_uv: tuple
    is_stereo: bool
    is_kf_in_window: bool


@dataclass
class ImuEdgeData:
    """local_inertial_ba.rs:79-88; preint = (delta_rot qw,qx,qy,qz, delta_vel, delta_pos, dt) of PreintegratedState"""
    kf_i_id: int
    kf_j_id: int
    preint: np.ndarray


@dataclass
class InertialBAProblemData:
    """local_inertial_ba.rs:40-62.  kf_poses are T_wc, fixed_kf_poses T_cw (7-vectors); biases 6-vectors (gyro, accel)."""
    kf_poses: Dict[int, np.ndarray]
    kf_velocities: Dict[int, np.ndarray]
    kf_biases: Dict[int, np.ndarray]
    mp_positions: Dict[int, np.ndarray]
    fixed_kf_poses: Dict[int, np.ndarray]
    visual_observations: List[InertialVisualObs]
    imu_edges: List[ImuEdgeData]
    opt_kf_ids: List[int]
    mp_ids: List[int]


@dataclass
class InertialBAResultData:
    """local_inertial_ba.rs:90-106: the first keyframe of the window is not reported (:1250)."""
    optimized_poses: Dict[int, np.ndarray] = field(default_factory=dict)
    optimized_velocities: Dict[int, np.ndarray] = field(default_factory=dict)
    optimized_biases: Dict[int, np.ndarray] = field(default_factory=dict)
    optimized_points: Dict[int, np.ndarray] = field(default_factory=dict)
    iterations: int = 0
    initial_error: float = 0.0
    final_error: float = 0.0


def flatten_inertial_ba_problem(problem: InertialBAProblemData):
    """The id -> index re-keying of local_inertial_ba.rs:1084-1185: observations of unknown map points and IMU edges
    with a keyframe outside the window are dropped (:1107, :1129-1130); an in-window flag whose keyframe is not in
    opt_kf_ids, or a fixed keyframe without a pose, falls back to the identity pose (:637); missing states start at 0."""
    kf_idx = {k: i for i, k in enumerate(problem.opt_kf_ids)}
    mp_idx = {m: i for i, m in enumerate(problem.mp_ids)}
    fixed_ids = list(problem.fixed_kf_poses.keys())
    fixed_idx = {k: i for i, k in enumerate(fixed_ids)}
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    poses = np.array([problem.kf_poses.get(k, ident) for k in problem.opt_kf_ids], np.float64).reshape(-1, 7)
    vel = np.array([problem.kf_velocities.get(k, np.zeros(3)) for k in problem.opt_kf_ids], np.float64).reshape(-1, 3)
    bias = np.array([problem.kf_biases.get(k, np.zeros(6)) for k in problem.opt_kf_ids], np.float64).reshape(-1, 6)
    fixed = np.array([problem.fixed_kf_poses[k] for k in fixed_ids], np.float64).reshape(-1, 7)
    pts = np.array([problem.mp_positions.get(m, np.zeros(3)) for m in problem.mp_ids], np.float64).reshape(-1, 3)
    rows = []
    for o in problem.visual_observations:
        if o.mp_id not in mp_idx:
            continue
        if o.is_kf_in_window and o.kf_id in kf_idx:
            rows.append((kf_idx[o.kf_id], -1, mp_idx[o.mp_id], int(o.is_stereo), o.observed_uv[0], o.observed_uv[1]))
        else:
            rows.append((-1, fixed_idx.get(o.kf_id, -1), mp_idx[o.mp_id], int(o.is_stereo), o.observed_uv[0], o.observed_uv[1]))
    edges = [(kf_idx[e.kf_i_id], kf_idx[e.kf_j_id], e.preint) for e in problem.imu_edges if e.kf_i_id in kf_idx and e.kf_j_id in kf_idx]
    ek = np.array([(a, b) for a, b, _ in edges], np.int32).reshape(-1, 2)
    pre = np.array([p for _, _, p in edges], np.float64).reshape(-1, 11)
    return poses, vel, bias, fixed, pts, np.array(rows, BA_OBS), ek, pre


def solve_inertial_ba(problem: InertialBAProblemData, camera: CameraModel, config: LocalInertialBAConfig,
                      should_stop: Callable[[], bool], handle: Handle = None) -> Optional[InertialBAResultData]:
    """local_inertial_ba.rs:1074-1275."""
    if len(problem.opt_kf_ids) < 2:
        return None
    poses, vel, bias, fixed, pts, obs, ek, pre = flatten_inertial_ba_problem(problem)
    r = (handle or _handle()).ba_solve_inertial(camera, config, poses, vel, bias, fixed, pts, obs, ek, pre, should_stop)
    if r is None:
        return None
    ids = problem.opt_kf_ids
    return InertialBAResultData({k: r["poses_wc"][i] for i, k in enumerate(ids) if i > 0}, {k: r["velocities"][i] for i, k in enumerate(ids) if i > 0},
                                {k: r["biases"][i] for i, k in enumerate(ids) if i > 0}, {m: r["points"][i] for i, m in enumerate(problem.mp_ids)},
                                r["iterations"], r["initial_error"], r["final_error"])
