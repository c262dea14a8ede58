"""ctypes binding of the C-ABI in include/orbfe.h (liborbfe_hip.so).

There is no fallback: if the HIP library is missing or no device is usable this module raises.
"""
from __future__ import annotations

import ctypes as C
import threading
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liborbfe_hip.so")

KP_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")]
)
assert KP_DTYPE.itemsize == 28

ORBFE_OK = 0
STATUS_NAMES = {0: "OK", 1: "EBADARG", 2: "EBADSIZE", 3: "EDEVICE", 4: "ECAPACITY", 5: "ENOMEM"}
STAGE_COUNT = 8


class OrbfeError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"orbfe {STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class ImageSizeError(OrbfeError):
    """Mirrors the reference's ImageSizeError (include/ORB_SLAM2/Error.h, thrown at ORBExtractor.cc:310-314)."""


class Config(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("n_features", C.c_int32), ("n_levels", C.c_int32),
        ("scale_factor", C.c_float), ("fast_hi", C.c_int32), ("fast_lo", C.c_int32), ("brief_pairs", C.c_void_p),
        ("blur_variant", C.c_int32), ("gray_variant", C.c_int32), ("device_id", C.c_int32), ("max_images", C.c_int32), ("stream", C.c_void_p),
    ]


class LevelInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_float), ("quota", C.c_int32),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("cell_w", C.c_int32), ("cell_h", C.c_int32)]


class BaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("poses", C.c_void_p),
                ("points", C.c_void_p), ("edge_pose", C.c_void_p), ("edge_point", C.c_void_p), ("meas", C.c_void_p),
                ("is_stereo", C.c_void_p), ("info", C.c_void_p), ("huber_delta", C.c_void_p), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double)]


class PoseGraph(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("estimates", C.c_void_p), ("fixed", C.c_void_p),
                ("edge_v0", C.c_void_p), ("edge_v1", C.c_void_p), ("meas", C.c_void_p)]


class PoseGraphOptions(C.Structure):
    _fields_ = [("solver", C.c_int32)]


class BaSystemOut(C.Structure):
    _fields_ = [("Hpp", C.c_void_p), ("bp", C.c_void_p), ("Hll", C.c_void_p), ("bl", C.c_void_p), ("Hpl", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("bf", C.c_float)]


class BaOptimizeOut(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("level", C.c_void_p), ("chi2", C.c_void_p), ("bad", C.c_void_p),
                ("iterations", C.c_void_p)]


class BaGlobalOptions(C.Structure):
    _fields_ = [("solver", C.c_int32), ("pcg_tol", C.c_double), ("pcg_max_iter", C.c_int32)]


class BaGlobalOut(C.Structure):
    _fields_ = [("poses", C.c_void_p), ("points", C.c_void_p), ("chi2", C.c_void_p), ("iterations", C.c_void_p), ("cg_stats", C.c_void_p)]


class FramePose(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("min_u", C.c_float), ("max_u", C.c_float), ("min_v", C.c_float),
                ("max_v", C.c_float)]


class TrackInput(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("pos", C.c_void_p), ("view_dir", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p),
                ("desc", C.c_void_p), ("flags", C.c_void_p), ("held", C.c_void_p), ("right_u", C.c_void_p), ("level_sigma2", C.c_void_p),
                ("level_inv_sigma2", C.c_void_p), ("pose_se3", C.c_void_p), ("th", C.c_float), ("ratio", C.c_float),
                ("min_threshold", C.c_int32), ("min_matches", C.c_int32)]


class TrackStoredInput(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("ids", C.c_void_p), ("flags", C.c_void_p), ("held", C.c_void_p), ("right_u", C.c_void_p),
                ("level_sigma2", C.c_void_p), ("level_inv_sigma2", C.c_void_p), ("pose_se3", C.c_void_p), ("th", C.c_float), ("ratio", C.c_float),
                ("min_threshold", C.c_int32), ("min_matches", C.c_int32)]


class MotionInput(C.Structure):
    _fields_ = [("n", C.c_int32), ("qxy", C.c_void_p), ("q_octave", C.c_void_p), ("q_min_level", C.c_void_p), ("q_max_level", C.c_void_p), ("desc", C.c_void_p),
                ("pos", C.c_void_p), ("held", C.c_void_p), ("right_u", C.c_void_p), ("level_sigma2", C.c_void_p), ("level_inv_sigma2", C.c_void_p),
                ("pose_se3", C.c_void_p), ("th", C.c_float), ("th_second", C.c_float), ("ratio", C.c_float), ("min_threshold", C.c_int32),
                ("min_matches", C.c_int32)]


class TrackOutput(C.Structure):
    _fields_ = [("assigned", C.c_void_p), ("edge_of", C.c_void_p), ("inlier", C.c_void_p), ("n_matches", C.c_void_p), ("n_edges", C.c_void_p),
                ("n_good", C.c_void_p), ("pose_out", C.c_void_p)]


class RelocInput(C.Structure):
    _fields_ = [("kf_id", C.c_uint64), ("n", C.c_int32), ("good", C.c_void_p), ("pos", C.c_void_p), ("kf_Rcw", C.c_float * 9),
                ("kf_tcw", C.c_float * 3), ("held", C.c_void_p), ("right_u", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("bounds", C.c_float * 4), ("level_sigma2", C.c_void_p), ("level_inv_sigma2", C.c_void_p), ("cam", C.POINTER(Camera)),
                ("baseline", C.c_float), ("th_first", C.c_float), ("th_second", C.c_float), ("ratio", C.c_float),
                ("min_threshold", C.c_int32), ("min_inliers", C.c_int32), ("enough", C.c_int32)]


class RelocOutput(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("verdict", "n_edges", "n_inliers", "n_added", "tlc_z", "pose_se3", "Tcw", "inlier", "assigned",
                                          "final_assigned", "excluded_hits", "query_accepted")]


RELOC_VERDICTS = {1: "REJECT_1", 2: "ACCEPT_1", 3: "REJECT_2", 4: "ACCEPT_2", 5: "REJECT_3", 6: "ACCEPT_3"}


class TrackRefInput(C.Structure):
    _fields_ = [("kf_id", C.c_uint64), ("n", C.c_int32), ("good", C.c_void_p), ("pos", C.c_void_p), ("frame_good", C.c_void_p),
                ("frame_pos", C.c_void_p), ("right_u", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("bounds", C.c_float * 4),
                ("level_sigma2", C.c_void_p), ("level_inv_sigma2", C.c_void_p), ("cam", C.POINTER(Camera)), ("levelsup", C.c_int32),
                ("ratio", C.c_float), ("dist_threshold", C.c_int32), ("check_orientation", C.c_int32), ("min_matches", C.c_int32),
                ("min_inliers", C.c_int32), ("n_nodes", C.c_int32), ("nodes", C.c_void_p), ("node_offsets", C.c_void_p), ("features", C.c_void_p)]


class TrackRefOutput(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("verdict", "n_matches", "matches", "assigned", "n_edges", "n_inliers", "inlier", "final_assigned",
                                          "pose_se3", "Tcw", "bow")]


TRACKREF_VERDICTS = {1: "REJECT_MATCHES", 2: "REJECT_INLIERS", 3: "ACCEPT"}
TRACKREF_OWN = -2


class MotionSlotsInput(C.Structure):
    _fields_ = [("last_flags", C.c_void_p), ("last_ids", C.c_void_p), ("last_pos", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("last_Rcw", C.c_float * 9), ("last_tcw", C.c_float * 3), ("last_Rwc", C.c_float * 9), ("last_twc", C.c_float * 3),
                ("bounds", C.c_float * 4), ("cam", C.POINTER(Camera)), ("baseline", C.c_float), ("level_sigma2", C.c_void_p),
                ("level_inv_sigma2", C.c_void_p), ("th", C.c_float), ("th_second", C.c_float), ("ratio", C.c_float),
                ("min_threshold", C.c_int32), ("min_matches", C.c_int32), ("min_inliers", C.c_int32)]


class MotionSlotsOutput(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("verdict", "passes", "n_matches", "n_edges", "n_inliers", "n_in_map", "assigned", "final_assigned",
                                          "inlier", "excluded_hits", "query_matches", "temp", "temp_pos", "pose_se3", "Tcw")]


MOTION_VERDICTS = {1: "REJECT_MATCHES", 2: "REJECT_INLIERS", 3: "ACCEPT"}


def motion_slots_outputs(nf, fill=None):
    """the raw output arrays of orbfe_track_motion_model_slots for nf features; fill: a byte every array is filled with (a sentinel)"""
    o = dict(verdict=np.zeros(1, np.int32), passes=np.zeros(1, np.int32), n_matches=np.zeros(1, np.int32), n_edges=np.zeros(1, np.int32),
             n_inliers=np.zeros(1, np.int32), n_in_map=np.zeros(1, np.int32), assigned=np.full(nf, -1, np.int32),
             final_assigned=np.full(nf, -1, np.int32), inlier=np.zeros(nf, np.uint8), excluded_hits=np.zeros(nf, np.int32),
             query_matches=np.zeros(nf, np.int32), temp=np.zeros(nf, np.uint8), temp_pos=np.zeros((nf, 3), np.float32), pose_se3=np.zeros(7),
             Tcw=np.zeros(12, np.float32))
    if fill is not None:
        for v in o.values():
            v.view(np.uint8)[...] = fill
    return o


class MapSummary(C.Structure):
    _fields_ = [("next_id", C.c_uint64), ("n_scale_factors", C.c_int32), ("n_keyframes", C.c_int32), ("n_mappoints", C.c_int32),
                ("n_keypoints", C.c_int64), ("n_observations", C.c_int64)]


class MapGraph(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("pose_kf_id", "pose_fixed", "poses", "point_id", "points", "edge_pose", "edge_point",
                                          "edge_feat", "meas", "is_stereo", "info", "huber_delta")]


class MapBaReport(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_poses", "n_group", "n_points", "n_edges", "n_outlier_edges", "n_keyframes_hit",
                                         "n_bad_keyframes", "written")] + [("iterations", C.c_int32 * 2),
                                                                           ("chi2_before", C.c_double), ("chi2_after", C.c_double)]


class BatchResults(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("kps", "desc", "counts", "right_u", "depth", "n_matches")]


class VocabInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("n_nodes", C.c_int32), ("n_words", C.c_int32)]


class BowOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("words", "values", "n_words", "nodes", "node_offsets", "features", "n_nodes")]


class KfdbQueryIn(C.Structure):
    _fields_ = [("words", C.c_void_p), ("values", C.c_void_p), ("n_words", C.c_int32), ("ignore", C.c_void_p), ("n_ignore", C.c_int32),
                ("min_score", C.c_void_p)]


class TriKf(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("n_nodes", C.c_int32), ("nodes", C.c_void_p),
                ("node_offsets", C.c_void_p), ("features", C.c_void_p), ("flags", C.c_void_p), ("depth", C.c_void_p), ("right_u", C.c_void_p),
                ("Tcw", C.c_float * 16), ("Twc", C.c_float * 16), ("Ow", C.c_float * 3), ("unproc", C.c_void_p), ("unproc_pos", C.c_void_p)]


class FuseKf(C.Structure):
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("bounds", C.c_float * 4)]


class FusePoints(C.Structure):
    _fields_ = [("has_point", C.c_void_p), ("pos", C.c_void_p), ("view_dir", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p)]


class KfstoreInfo(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_bow", C.c_int32), ("has_stereo", C.c_int32), ("n_nodes", C.c_int32), ("n_bow_features", C.c_int32), ("grid_rows", C.c_int32),
                ("grid_cols", C.c_int32), ("bounds", C.c_float * 4), ("bytes", C.c_int64)]


class FusePose(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3)]


class TriState(C.Structure):
    _fields_ = [("n", C.c_int32), ("flags", C.c_void_p), ("Tcw", C.c_float * 16), ("Twc", C.c_float * 16), ("Ow", C.c_float * 3),
                ("unproc", C.c_void_p), ("unproc_pos", C.c_void_p)]


class BowQuery(C.Structure):
    _fields_ = [("from_store", C.c_int32), ("id", C.c_uint64), ("n", C.c_int32), ("desc", C.c_void_p), ("angle", C.c_void_p),
                ("n_nodes", C.c_int32), ("nodes", C.c_void_p), ("node_offsets", C.c_void_p), ("features", C.c_void_p), ("flags", C.c_void_p)]


BOW_MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4")])
BOW_SEARCH_MAX_KF = 64
BOW_TRACK, BOW_LOOP, BOW_ADD = 0, 1, 2
FUSE_MAX_KF = 64
FUSE_POINTS_MAX_PAIRS = 1 << 22
TRI_REC_DTYPE = np.dtype([("nb", "<i4"), ("q", "<i4"), ("t", "<i4"), ("kind", "<i4"), ("xyz", "<f4", (3,))])
TRI_MAX_NB = 64


class Sim3Side(C.Structure):
    _fields_ = [("id", C.c_uint64), ("n", C.c_int32), ("flags", C.c_void_p), ("pos", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3)]


class Sim3Points(C.Structure):
    _fields_ = [("m", C.c_int32), ("usable", C.c_void_p), ("pos", C.c_void_p), ("view_dir", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("desc", C.c_void_p)]


class BaEdgeOut(C.Structure):
    _fields_ = [("error", C.c_void_p), ("chi2", C.c_void_p), ("rho", C.c_void_p), ("j_point", C.c_void_p),
                ("j_pose", C.c_void_p), ("depth_positive", C.c_void_p)]


EXPORTS = [
    "orbfe_abi_version", "orbfe_create", "orbfe_destroy", "orbfe_last_error", "orbfe_get_level_info", "orbfe_get_scale_factors",
    "orbfe_get_capacity",
    "orbfe_extract", "orbfe_extract_batch", "orbfe_extract_slot", "orbfe_extract_slot_begin", "orbfe_extract_slot_end", "orbfe_extract_slots", "orbfe_frame_stereo", "orbfe_frame_stereo_slots", "orbfe_frame_rgbd_image", "orbfe_track_motion_model", "orbfe_fetch_batch", "orbfe_fetch_stereo_batch", "orbfe_get_pyramid", "orbfe_stereo_match", "orbfe_stereo_batch_device", "orbfe_sync",
    "orbfe_host_alloc", "orbfe_host_alloc_on", "orbfe_host_free", "orbfe_recommended_hw_queues", "orbfe_stream_submit", "orbfe_stream_wait", "orbfe_stream_device_results", "orbfe_record_bytes", "orbfe_stream_pack_records",
    "orbfe_fetch_features", "orbfe_fetch_stereo", "orbfe_device_results", "orbfe_match_bruteforce", "orbfe_ba_eval_edges", "orbfe_ba_build_system", "orbfe_ba_local_optimize", "orbfe_ba_global_optimize", "orbfe_pose_only_optimize", "orbfe_search_in_area", "orbfe_search_in_area_features", "orbfe_search_in_area_features_ex", "orbfe_extract_color", "orbfe_frame_rgbd", "orbfe_project_map_points", "orbfe_track_local_map",
    "orbfe_map_pb_summary", "orbfe_map_pb_reencode", "orbfe_map_pb_to_txt", "orbfe_map_txt_to_pb", "orbfe_map_local_graph", "orbfe_map_local_ba",
    "orbfe_vocab_load_txt", "orbfe_vocab_info_get", "orbfe_vocab_export", "orbfe_vocab_destroy", "orbfe_bow_transform", "orbfe_bow_slots",
    "orbfe_kfdb_create", "orbfe_kfdb_destroy", "orbfe_kfdb_add", "orbfe_kfdb_set_bad", "orbfe_kfdb_erase", "orbfe_kfdb_size", "orbfe_kfdb_query",
    "orbfe_kfdb_score", "orbfe_kfdb_group_filter",
    "orbfe_pnp_create", "orbfe_pnp_destroy", "orbfe_pnp_iterate", "orbfe_pnp_engine", "orbfe_pnp_stats",
    "orbfe_sim3_create", "orbfe_sim3_destroy", "orbfe_sim3_iterate", "orbfe_sim3_engine", "orbfe_sim3_stats", "orbfe_sim3_profile",
    "orbfe_sim3_optimize", "orbfe_pose_graph_optimize", "orbfe_pose_graph_optimize_ex",
    "orbfe_create_new_map_points", "orbfe_fuse_into_keyframes",
    "orbfe_kfstore_create", "orbfe_kfstore_destroy", "orbfe_kfstore_add", "orbfe_kfstore_add_from_slot", "orbfe_kfstore_set_bow",
    "orbfe_kfstore_erase", "orbfe_kfstore_size", "orbfe_kfstore_info_get", "orbfe_kfstore_fetch", "orbfe_fuse_into_keyframes_stored",
    "orbfe_create_new_map_points_stored", "orbfe_search_by_bow_stored", "orbfe_search_by_sim3_stored", "orbfe_search_by_sim3_points_stored",
    "orbfe_fuse_points_into_keyframes_stored", "orbfe_debug_fuse_points_kernels", "orbfe_reloc_refine_stored",
    "orbfe_track_reference_stored",
    "orbfe_mpstore_create", "orbfe_mpstore_destroy", "orbfe_mpstore_upsert", "orbfe_mpstore_erase", "orbfe_mpstore_fetch", "orbfe_mpstore_size",
    "orbfe_track_local_map_stored", "orbfe_track_motion_model_slots",
    "orbfe_profile_enable", "orbfe_profile_read", "orbfe_stage_name", "orbfe_debug_candidates", "orbfe_debug_se3_oplus",
    "orbfe_debug_reduced_solve", "orbfe_debug_sim3_edges", "orbfe_debug_pose_graph_edges", "orbfe_debug_pose_graph_phases",
    "orbfe_debug_pg_sparse_solve", "orbfe_debug_ba_reduced_bsr", "orbfe_debug_bsr_pcg", "orbfe_debug_ba_global_phases",
]
BOW_MAX_FEATURES = 65535
PG_MAX_FREE = 1024          # ORBFE_PG_MAX_FREE: the dense pose-graph solver's bound on the non-fixed vertices
GBA_DENSE_MAX_FREE = 1000   # ORBFE_GBA_DENSE_MAX_FREE: solver 0 of ba_global_optimize is dense up to this many non-fixed keyframes

_lib = None


def load() -> C.CDLL:
    """Load liborbfe_hip.so (built by orb_slam2_ros2_amd/csrc/Makefile); raises if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: build it with `make -C orb_slam2_ros2_amd/csrc` "
                      "(there is no CPU fallback for the front end)")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7, and a process that
    # loads the system runtime first and torch's second ends up with two runtimes, the second of which sees no
    # GPU.  If torch is installed, let it load its runtime first; liborbfe_hip.so then binds to that same copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    L.orbfe_abi_version.restype = C.c_int
    L.orbfe_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.orbfe_destroy.argtypes = [vp]
    L.orbfe_destroy.restype = None
    L.orbfe_last_error.argtypes = [vp]
    L.orbfe_last_error.restype = C.c_char_p
    L.orbfe_get_level_info.argtypes = [vp, i32, C.POINTER(LevelInfo)]
    L.orbfe_get_scale_factors.argtypes = [vp, vp, i32]
    L.orbfe_get_capacity.argtypes = [vp]
    L.orbfe_get_capacity.restype = i32
    L.orbfe_extract.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    L.orbfe_extract_batch.argtypes = [vp, i32, vp, C.c_size_t, vp, vp, vp]
    if hasattr(L, "orbfe_extract_slot_begin"):   # (ABI 4; tools/exp compares against libraries of earlier rounds)
        L.orbfe_extract_slot_begin.argtypes = [vp, i32, vp, C.c_size_t]
        L.orbfe_extract_slot_end.argtypes = [vp, i32, vp, vp, vp]
    L.orbfe_extract_slot.argtypes = [vp, i32, vp, C.c_size_t, vp, vp, vp]
    L.orbfe_extract_slots.argtypes = [vp, i32, i32, vp, C.c_size_t, vp, vp, vp]
    L.orbfe_frame_rgbd_image.argtypes = [vp, i32, vp, C.c_size_t, i32, vp, vp, i32, C.c_size_t, C.c_float, vp, vp, vp, vp, vp]
    L.orbfe_track_motion_model.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_frame_stereo.argtypes = [vp, vp, vp, C.c_size_t, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp]
    L.orbfe_frame_stereo_slots.argtypes = [vp, i32, vp, vp, C.c_size_t, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp]
    L.orbfe_fetch_batch.argtypes = [vp, i32, i32, vp, vp, vp]
    L.orbfe_fetch_stereo_batch.argtypes = [vp, i32, i32, vp, vp, vp]
    L.orbfe_get_pyramid.argtypes = [vp, i32, i32, i32, vp]
    L.orbfe_stereo_match.argtypes = [vp, i32, i32, f32, f32, vp, vp, vp, vp, vp]
    L.orbfe_stereo_batch_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, i32, f32, f32]
    L.orbfe_sync.argtypes = [vp]
    L.orbfe_host_alloc.argtypes = [C.c_size_t]
    L.orbfe_host_alloc.restype = vp
    L.orbfe_host_alloc_on.argtypes = [i32, C.c_size_t]
    L.orbfe_host_alloc_on.restype = vp
    L.orbfe_host_free.argtypes = [vp]
    L.orbfe_host_free.restype = None
    L.orbfe_stream_submit.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, i32, f32, f32, C.POINTER(BatchResults), C.POINTER(C.c_int64)]
    L.orbfe_stream_wait.argtypes = [vp, C.c_int64]
    L.orbfe_stream_device_results.argtypes = [vp, C.c_int64, i32] + [C.POINTER(vp)] * 6
    L.orbfe_record_bytes.argtypes = [vp]
    L.orbfe_record_bytes.restype = C.c_size_t
    L.orbfe_stream_pack_records.argtypes = [vp, C.c_int64, i32, vp]
    L.orbfe_fetch_features.argtypes = [vp, i32, vp, vp, vp]
    L.orbfe_fetch_stereo.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.orbfe_device_results.argtypes = [vp] + [C.POINTER(vp)] * 6
    L.orbfe_match_bruteforce.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.orbfe_ba_eval_edges.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaEdgeOut)]
    L.orbfe_ba_build_system.argtypes = [vp, C.POINTER(BaProblem), vp, C.POINTER(BaSystemOut)]
    L.orbfe_ba_local_optimize.argtypes = [vp, C.POINTER(BaProblem), vp, i32, i32, vp, C.POINTER(BaOptimizeOut)]
    L.orbfe_pose_only_optimize.argtypes = [vp, i32, vp, vp, vp, vp, vp] + [C.c_double] * 5 + [vp, vp, vp]
    L.orbfe_search_in_area.argtypes = [vp, i32, i32] + [vp] * 10
    L.orbfe_search_in_area_features.argtypes = [vp, i32, vp, vp, i32] + [vp] * 10
    L.orbfe_search_in_area_features_ex.argtypes = [vp, i32, vp, vp, vp, i32] + [vp] * 11
    L.orbfe_extract_color.argtypes = [vp, vp, C.c_size_t, i32, vp, vp, vp]
    L.orbfe_frame_rgbd.argtypes = [vp, i32, C.POINTER(Camera), vp, i32, C.c_size_t, f32, vp, vp, vp]
    L.orbfe_project_map_points.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(FramePose), C.POINTER(Camera), vp, vp, vp, vp, vp]
    L.orbfe_track_local_map.argtypes = [vp, i32, C.POINTER(FramePose), C.POINTER(Camera), C.POINTER(TrackInput), C.POINTER(TrackOutput)]
    L.orbfe_map_pb_summary.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(MapSummary)]
    L.orbfe_map_pb_reencode.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.orbfe_map_pb_to_txt.argtypes = [C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.orbfe_map_txt_to_pb.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.orbfe_map_local_graph.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(i32 * 4), C.POINTER(MapGraph)]
    L.orbfe_map_local_ba.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(Camera), vp, vp, C.c_size_t,
                                     C.POINTER(C.c_size_t), C.POINTER(MapBaReport)]
    L.orbfe_vocab_load_txt.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.orbfe_vocab_info_get.argtypes = [vp, C.POINTER(VocabInfo)]
    L.orbfe_vocab_export.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbfe_vocab_destroy.argtypes = [vp]
    L.orbfe_vocab_destroy.restype = None
    L.orbfe_bow_transform.argtypes = [vp, vp, vp, i32, i32, C.POINTER(BowOut)]
    L.orbfe_bow_slots.argtypes = [vp, vp, i32, i32, i32, i32, C.POINTER(BowOut)]
    L.orbfe_kfdb_create.argtypes = [i32, i32, C.POINTER(vp)]
    L.orbfe_kfdb_destroy.argtypes = [vp]
    L.orbfe_kfdb_destroy.restype = None
    L.orbfe_kfdb_add.argtypes = [vp, i32, vp, vp, vp, vp]
    L.orbfe_kfdb_set_bad.argtypes = [vp, i32, vp, vp]
    L.orbfe_kfdb_erase.argtypes = [vp, i32, vp]
    L.orbfe_kfdb_size.argtypes = [vp, C.POINTER(C.c_int64)]
    L.orbfe_kfdb_query.argtypes = [vp, vp, C.POINTER(KfdbQueryIn), vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.orbfe_kfdb_score.argtypes = [vp, vp, C.POINTER(KfdbQueryIn), vp, i32, vp]
    L.orbfe_kfdb_group_filter.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.POINTER(C.c_int64)]
    L.orbfe_pnp_create.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, C.POINTER(Camera), C.POINTER(PnpParams), C.POINTER(vp)]
    L.orbfe_pnp_destroy.argtypes = [vp]
    L.orbfe_pnp_destroy.restype = None
    L.orbfe_pnp_iterate.argtypes = [vp, i32, i32, vp, C.POINTER(i32), vp, C.POINTER(C.c_int64), C.c_int64, C.POINTER(i32), C.POINTER(i32)]
    L.orbfe_pnp_engine.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.orbfe_pnp_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.orbfe_sim3_create.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(Camera), C.POINTER(Sim3Params), C.POINTER(vp)]
    L.orbfe_sim3_destroy.argtypes = [vp]
    L.orbfe_sim3_destroy.restype = None
    L.orbfe_sim3_iterate.argtypes = [vp, i32, i32, vp, C.POINTER(i32), vp, C.POINTER(C.c_int64), C.c_int64, C.POINTER(i32), C.POINTER(i32)]
    L.orbfe_sim3_engine.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.orbfe_sim3_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.orbfe_sim3_profile.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.orbfe_create_new_map_points.argtypes = [vp, C.POINTER(TriKf), i32, vp, C.POINTER(Camera), vp, f32, vp, i32, vp, C.c_int64,
                                              C.POINTER(C.c_int64), vp, C.c_int64, C.POINTER(C.c_int64), vp]
    L.orbfe_fuse_into_keyframes.argtypes = [vp, C.POINTER(FuseKf), C.POINTER(FusePoints), i32, vp, vp, C.POINTER(Camera), f32, vp, i32, f32, f32,
                                            i32, vp, vp, vp]
    u64, i64 = C.c_uint64, C.c_int64
    L.orbfe_kfstore_create.argtypes = [i32, i32, i32, i32, i64, C.POINTER(vp)]
    L.orbfe_kfstore_destroy.argtypes = [vp]
    L.orbfe_kfstore_destroy.restype = None
    L.orbfe_kfstore_add.argtypes = [vp, u64, i32, vp, vp, vp, vp, vp]
    L.orbfe_kfstore_add_from_slot.argtypes = [vp, vp, u64, i32, i32, vp, C.POINTER(i32)]
    L.orbfe_kfstore_set_bow.argtypes = [vp, u64, i32, vp, vp, vp]
    L.orbfe_kfstore_erase.argtypes = [vp, i32, vp]
    L.orbfe_kfstore_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.orbfe_kfstore_info_get.argtypes = [vp, u64, C.POINTER(KfstoreInfo)]
    L.orbfe_kfstore_fetch.argtypes = [vp, u64] + [vp] * 9
    L.orbfe_fuse_into_keyframes_stored.argtypes = [vp, vp, u64, i32, C.POINTER(FusePoints), i32, vp, vp, vp, C.POINTER(Camera), f32, vp, i32, f32,
                                                   f32, i32, vp, vp, vp]
    L.orbfe_create_new_map_points_stored.argtypes = [vp, vp, u64, C.POINTER(TriState), i32, vp, vp, C.POINTER(Camera), vp, f32, vp, i32, vp, i64,
                                                     C.POINTER(i64), vp, i64, C.POINTER(i64), vp]
    L.orbfe_search_by_bow_stored.argtypes = [vp, vp, C.POINTER(BowQuery), i32, vp, vp, i32, f32, i32, i32, vp, i64, vp]
    L.orbfe_search_by_sim3_stored.argtypes = [vp, vp, C.POINTER(Sim3Side), C.POINTER(Sim3Side), vp, f32, i32, vp, C.POINTER(Camera), vp, i32, f32,
                                              f32, i32, vp, i32, C.POINTER(i32)]
    L.orbfe_search_by_sim3_points_stored.argtypes = [vp, vp, u64, C.POINTER(Sim3Points), vp, f32, C.POINTER(Camera), vp, i32, f32, f32, i32, vp, vp]
    L.orbfe_fuse_points_into_keyframes_stored.argtypes = [vp, vp, i32, vp, vp, C.POINTER(Sim3Points), C.POINTER(Camera), vp, i32, f32, f32, i32, vp,
                                                          vp]
    L.orbfe_debug_fuse_points_kernels.argtypes = [vp]
    L.orbfe_reloc_refine_stored.argtypes = [vp, i32, vp, C.POINTER(RelocInput), C.POINTER(RelocOutput)]
    L.orbfe_track_reference_stored.argtypes = [vp, i32, vp, vp, C.POINTER(TrackRefInput), C.POINTER(TrackRefOutput)]
    L.orbfe_mpstore_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.orbfe_mpstore_destroy.argtypes = [vp]
    L.orbfe_mpstore_destroy.restype = None
    L.orbfe_mpstore_upsert.argtypes = [vp, i32, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.orbfe_mpstore_erase.argtypes = [vp, i32, vp]
    L.orbfe_mpstore_fetch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.orbfe_mpstore_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.orbfe_track_local_map_stored.argtypes = [vp, i32, vp, C.POINTER(FramePose), C.POINTER(Camera), C.POINTER(TrackStoredInput),
                                               C.POINTER(TrackOutput)]
    L.orbfe_track_motion_model_slots.argtypes = [vp, i32, i32, i32, i32, vp, C.POINTER(MotionSlotsInput), C.POINTER(MotionSlotsOutput)]
    L.orbfe_profile_enable.argtypes = [vp, i32]
    L.orbfe_profile_read.argtypes = [vp, vp, vp, i32]
    L.orbfe_stage_name.argtypes = [i32]
    L.orbfe_stage_name.restype = C.c_char_p
    L.orbfe_debug_candidates.argtypes = [vp, i32, i32, vp, i32, vp]
    L.orbfe_debug_se3_oplus.argtypes = [vp, i32, vp, vp, vp]
    L.orbfe_debug_reduced_solve.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.orbfe_ba_global_optimize.argtypes = [vp, C.POINTER(BaProblem), vp, i32, vp, C.POINTER(BaGlobalOptions), C.POINTER(BaGlobalOut)]
    L.orbfe_debug_ba_reduced_bsr.argtypes = [vp, C.POINTER(BaProblem), vp, C.c_double, i32, vp, vp, vp, vp, vp]
    L.orbfe_debug_bsr_pcg.argtypes = [vp, i32, vp, vp, vp, vp, C.c_double, i32, vp, vp, vp]
    L.orbfe_debug_ba_global_phases.argtypes = [vp]
    L.orbfe_sim3_optimize.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp] + [C.c_float] * 4 + [vp, vp, vp, vp]
    L.orbfe_debug_sim3_edges.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp] + [C.c_float] * 4 + [vp, vp, vp, vp]
    L.orbfe_pose_graph_optimize.argtypes = [vp, vp, i32, vp, vp, vp]
    L.orbfe_pose_graph_optimize_ex.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.orbfe_debug_pg_sparse_solve.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_debug_pose_graph_edges.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_debug_pose_graph_phases.argtypes = [vp]
    _lib = L
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _row_strided(a, dtypes):
    """a as the C ABI takes an image: rows `strides[0]` bytes apart, everything inside a row contiguous.  A view that already is one (a
    column range of a larger image, rows with padding) is passed through WITHOUT a copy, so its stride reaches the library; anything
    else is made contiguous."""
    a = np.asarray(a)
    inner = a.dtype.itemsize
    ok = a.dtype in dtypes and a.ndim >= 2 and a.strides[0] >= inner * int(np.prod(a.shape[1:]))
    for ax in range(a.ndim - 1, 0, -1):
        ok = ok and a.strides[ax] == inner
        inner *= a.shape[ax]
    return a if ok else np.ascontiguousarray(a, dtypes[0] if len(dtypes) == 1 else None)


class PinnedArray:
    """numpy view of page-locked host memory from orbfe_host_alloc (freed with the object)"""

    def __init__(self, shape, dtype, device_id=-1):
        """device_id: the HIP device whose NUMA node the pages go to (-1: the calling thread's current device)"""
        self.lib = load()
        self.dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * self.dtype.itemsize
        self.p = self.lib.orbfe_host_alloc_on(int(device_id), max(n, 1))
        if not self.p:
            raise MemoryError(f"orbfe_host_alloc({n}) failed")
        self.array = np.frombuffer((C.c_uint8 * max(n, 1)).from_address(self.p), dtype=self.dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, "p", None):
            self.array = None
            self.lib.orbfe_host_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- map.pb (host-only entry points: no context, no device) ------------------------------------------
def _status(st, what):
    if st != 0:
        raise RuntimeError(f"{what}: orbfe status {st}")


def map_pb_summary(pb: bytes) -> dict:
    """Counts of an `orbslam2.MapData` file as Map::loadFromProtobuf would read it (src/Map.cc:252-313)."""
    s = MapSummary()
    _status(load().orbfe_map_pb_summary(pb, len(pb), C.byref(s)), "map_pb_summary")
    return {k: getattr(s, k) for k, _ in MapSummary._fields_}


def map_pb_reencode(pb: bytes) -> bytes:
    """Parse + serialise: the canonical libprotobuf encoding of the same content."""
    L, n = load(), C.c_size_t(0)
    _status(L.orbfe_map_pb_reencode(pb, len(pb), None, 0, C.byref(n)), "map_pb_reencode")
    out = np.zeros(max(n.value, 1), np.uint8)
    _status(L.orbfe_map_pb_reencode(pb, len(pb), ptr(out), out.size, C.byref(n)), "map_pb_reencode")
    return out[:n.value].tobytes()


def map_pb_to_txt(pb: bytes):
    """map.pb -> (KeyFrames.txt, MapPoints.txt) as Map::saveToTxtFile writes them (src/Map.cc:82-110)"""
    L, nk, nm = load(), C.c_size_t(0), C.c_size_t(0)
    _status(L.orbfe_map_pb_to_txt(pb, len(pb), None, 0, C.byref(nk), None, 0, C.byref(nm)), "map_pb_to_txt")
    kf, mp = np.zeros(max(nk.value, 1), np.uint8), np.zeros(max(nm.value, 1), np.uint8)
    _status(L.orbfe_map_pb_to_txt(pb, len(pb), ptr(kf), kf.size, C.byref(nk), ptr(mp), mp.size, C.byref(nm)), "map_pb_to_txt")
    return kf[:nk.value].tobytes().decode(), mp[:nm.value].tobytes().decode()


def map_txt_to_pb(keyframes_txt: str, mappoints_txt: str) -> bytes:
    """(KeyFrames.txt, MapPoints.txt) -> map.pb: Map::loadFromTxtFile's readers (src/Map.cc:117-165), canonical protobuf encoding"""
    L, n = load(), C.c_size_t(0)
    k, m = keyframes_txt.encode(), mappoints_txt.encode()
    _status(L.orbfe_map_txt_to_pb(k, len(k), m, len(m), None, 0, C.byref(n)), "map_txt_to_pb")
    out = np.zeros(max(n.value, 1), np.uint8)
    _status(L.orbfe_map_txt_to_pb(k, len(k), m, len(m), ptr(out), out.size, C.byref(n)), "map_txt_to_pb")
    return out[:n.value].tobytes()


def map_local_graph(pb: bytes, kf_id: int) -> dict:
    """The graph Optimizer::OptimizeLocalMap builds around keyframe kf_id (src/Optimizer.cc:232-330)."""
    L, sizes = load(), (C.c_int32 * 4)()
    _status(L.orbfe_map_local_graph(pb, len(pb), kf_id, C.byref(sizes), None), "map_local_graph")
    n_poses, n_group, n_points, n_edges = list(sizes)
    g = dict(pose_kf_id=np.zeros(n_poses, np.uint64), pose_fixed=np.zeros(n_poses, np.uint8), poses=np.zeros((n_poses, 7)),
             point_id=np.zeros(n_points, np.uint64), points=np.zeros((n_points, 3)), edge_pose=np.zeros(n_edges, np.int32),
             edge_point=np.zeros(n_edges, np.int32), edge_feat=np.zeros(n_edges, np.int32), meas=np.zeros((n_edges, 3)),
             is_stereo=np.zeros(n_edges, np.uint8), info=np.zeros(n_edges), huber_delta=np.zeros(n_edges))
    mg = MapGraph(*[ptr(g[k]).value if g[k].size else None for k, _ in MapGraph._fields_])
    _status(L.orbfe_map_local_graph(pb, len(pb), kf_id, C.byref(sizes), C.byref(mg)), "map_local_graph")
    g["n_group"] = n_group
    return g


class Vocabulary:
    """A DBoW vocabulary tree in the ORB-SLAM2 text format (orbfe_vocab: host data + one device copy per HIP device, made on first use)."""

    def __init__(self, handle):
        self.lib = load()
        self.h = handle

    @classmethod
    def load_txt(cls, path):
        L, h = load(), C.c_void_p(None)
        st = L.orbfe_vocab_load_txt(os.fsencode(path), C.byref(h))
        if st != ORBFE_OK:
            raise OrbfeError(st, L.orbfe_last_error(None).decode())
        return cls(h)

    def info(self) -> dict:
        vi = VocabInfo()
        _status(self.lib.orbfe_vocab_info_get(self.h, C.byref(vi)), "vocab_info")
        return {k: getattr(vi, k) for k, _ in VocabInfo._fields_}

    def export(self) -> dict:
        """the parsed arrays in node-id order: parent (-1 root), is_leaf, desc [n][32], weight, word_id (-1 inner nodes)"""
        n = self.info()["n_nodes"]
        a = dict(parent=np.zeros(n, np.int32), is_leaf=np.zeros(n, np.uint8), desc=np.zeros((n, 32), np.uint8), weight=np.zeros(n),
                 word_id=np.zeros(n, np.int32))
        _status(self.lib.orbfe_vocab_export(self.h, *[ptr(a[k]) for k in ("parent", "is_leaf", "desc", "weight", "word_id")]), "vocab_export")
        return a

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbfe_vocab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RansacParams(C.Structure):
    """orbfe_pnp_params and orbfe_sim3_params: one layout under two names"""
    _fields_ = [("min_set", C.c_int32), ("max_iterations", C.c_int32), ("ratio", C.c_float), ("prob", C.c_float)]


PnpParams = Sim3Params = RansacParams


class _RansacSet:
    """What PnPSet and Sim3Set share: the handle of a set made by orbfe_<_name>_create, and iterate's marshalling.  A subclass's __init__
    calls _create; it has _cap (the room for the returned inliers) and shapes what iterate returns."""
    _name = None

    def _create(self, sizes, *args):
        self.lib = load()
        self.sizes = sizes
        self._fn = {k: getattr(self.lib, f"orbfe_{self._name}_{k}") for k in ("create", "destroy", "iterate", "stats")}
        h = C.c_void_p(None)
        st = self._fn["create"](*args, C.byref(h))
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())
        self.h = h

    def _check(self, st):
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self._fn["destroy"](self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _iterate(self, problem, n, model, inliers, cap):
        """-> (ret, no_more, the 12 floats or None, inliers int32); model: 12 floats or None, inliers: the entry list or None"""
        ent = () if inliers is None else np.ascontiguousarray(inliers, np.int32).reshape(-1)
        cap = self._cap(len(ent), int(n), problem) if cap is None else int(cap)
        buf = np.empty(max(cap, 1), np.int32)  # (the library writes [0, k), and only that is returned)
        if len(ent):
            buf[:len(ent)] = ent
        mz = np.zeros(12, np.float32)
        has = C.c_int32(0)
        if model is not None:
            mz[:] = model
            has.value = 1
        k = C.c_int64(len(ent))
        ret, nm = C.c_int32(0), C.c_int32(0)
        self._check(self._fn["iterate"](self.h, int(problem), int(n), ptr(mz), C.byref(has), ptr(buf), C.byref(k), cap, C.byref(ret), C.byref(nm)))
        return bool(ret.value), bool(nm.value), (mz if has.value else None), buf[:k.value].copy()

    def stats(self):
        """(launch sequences, hypotheses evaluated on the device)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._fn["stats"](self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _ransac_engine(name, state):
    L = load()
    g = C.c_uint32(0)
    s = None if state is None else C.c_uint32(int(state))
    st = getattr(L, f"orbfe_{name}_engine")(C.byref(g), None if s is None else C.byref(s))
    if st != ORBFE_OK:
        raise OrbfeError(st, L.orbfe_last_error(None).decode())
    return g.value


class PnPSet(_RansacSet):
    """The PnPSolvers of one relocalisation on one device (orbfe_pnp, include/orbfe.h): problem i has the points
    [offsets[i], offsets[i + 1]) of xyz (world) / uv (keypoints) / octave.  cam = (fx, fy, cx, cy); params = (min_set, max_iterations,
    ratio, prob) or None for setRansacParams()'s defaults."""
    _name = "pnp"

    def __init__(self, offsets, xyz, uv, octave, level_sigma2, cam, params=None, device_id=0):
        o = np.ascontiguousarray(offsets, np.int64)
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        oc = np.ascontiguousarray(octave, np.int32).reshape(-1)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        if len(o) < 1 or o[-1] != len(x) or len(u) != len(x) or len(oc) != len(x):
            raise ValueError("PnPSet: offsets must end at len(xyz) == len(uv) == len(octave)")
        cm = Camera(*(float(v) for v in cam), 0, 0, 0, 0, 0, 0)
        pp = None if params is None else C.byref(PnpParams(*params))
        self._create(np.diff(o), int(device_id), len(o) - 1, ptr(o), ptr(x), ptr(u), ptr(oc), ptr(s2), len(s2), C.byref(cm), pp)

    def _cap(self, n_entry, n, problem):  # P1: the list piles up every hypothesis's inliers
        return n_entry + (n + 2) * int(self.sizes[problem]) + 1

    def iterate(self, problem, n, pose=None, inliers=None):
        """Ransac::iterate(n, modelRet, bNoMore, vnInlierIndices) of one problem: (ret, no_more, Rcw (3, 3) float32 or None,
        tcw (3,) float32 or None, inliers int32).  pose: None (empty Mats) or (Rcw, tcw); inliers: the entry list (appended to)."""
        if pose is not None:
            pose = np.concatenate([np.asarray(pose[0], np.float32).reshape(9), np.asarray(pose[1], np.float32).reshape(3)])
        ret, nm, m, inl = self._iterate(problem, n, pose, inliers, None)
        return ret, nm, (None if m is None else m[:9].reshape(3, 3).copy()), (None if m is None else m[9:].copy()), inl


def pnp_engine(state=None):
    """the process-wide PnP sampling engine's state (minstd_rand0's x); with `state`, set it first and return the old one"""
    return _ransac_engine("pnp", state)


class Sim3Set(_RansacSet):
    """The Sim3Solvers of one LoopClosing::computeSim3 call on one device (orbfe_sim3, include/orbfe.h): problem i has the
    correspondences [offsets[i], offsets[i + 1]) of pos_p / pos_q (world positions of the two map points) and octave_p / octave_q, and
    the keyframe poses pose_p[i] / pose_q[i] (12 floats: R row-major, then t).  cam = (fx, fy, cx, cy); params = (min_set,
    max_iterations, ratio, prob) or None for Sim3Solver::create's defaults (min_set must be 3)."""
    _name = "sim3"

    def __init__(self, offsets, pos_p, pos_q, octave_p, octave_q, pose_p, pose_q, level_sigma2, cam, params=None, device_id=0):
        o = np.ascontiguousarray(offsets, np.int64)
        xp = np.ascontiguousarray(pos_p, np.float32).reshape(-1, 3)
        xq = np.ascontiguousarray(pos_q, np.float32).reshape(-1, 3)
        op = np.ascontiguousarray(octave_p, np.int32).reshape(-1)
        oq = np.ascontiguousarray(octave_q, np.int32).reshape(-1)
        tp = np.ascontiguousarray(pose_p, np.float32).reshape(-1, 12)
        tq = np.ascontiguousarray(pose_q, np.float32).reshape(-1, 12)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        if len(o) < 1 or o[-1] != len(xp) or len(xq) != len(xp) or len(op) != len(xp) or len(oq) != len(xp):
            raise ValueError("Sim3Set: offsets must end at len(pos_p) == len(pos_q) == len(octave_p) == len(octave_q)")
        if len(tp) != len(o) - 1 or len(tq) != len(o) - 1:
            raise ValueError("Sim3Set: one pose_p and one pose_q per problem")
        cm = Camera(*(float(v) for v in cam), 0, 0, 0, 0, 0, 0)
        pp = None if params is None else C.byref(Sim3Params(*params))
        self._create(np.diff(o), int(device_id), len(o) - 1, ptr(o), ptr(xp), ptr(xq), ptr(op), ptr(oq), ptr(tp), ptr(tq), ptr(s2), len(s2),
                     C.byref(cm), pp)

    def _cap(self, n_entry, n, problem):  # S2: a list is one hypothesis's inliers
        size = int(self.sizes[problem]) if 0 <= int(problem) < len(self.sizes) else 0  # out of range: the library refuses it
        return max(n_entry, size) + 1

    def iterate(self, problem, n, model=None, inliers=None, cap=None):
        """Ransac::iterate(n, modelRet, bNoMore, vnInlierIndices) of one problem: (ret, no_more, model float32[12] (Rqp row-major, then
        tqp; the scale is 1) or None, inliers int32).  model / inliers: the entry state, returned untouched when no hypothesis ran."""
        return self._iterate(problem, n, None if model is None else np.asarray(model, np.float32).reshape(12), inliers, cap)

    def profile(self, enable=None):
        """(device microseconds between the events around the launches, bytes uploaded by create and the speculations) so far;
        enable True / False first starts / stops recording the events (None: leave)"""
        t, b = C.c_double(0), C.c_int64(0)
        self._check(self.lib.orbfe_sim3_profile(self.h, -1 if enable is None else int(bool(enable)), C.byref(t), C.byref(b)))
        return t.value, b.value


def sim3_engine(state=None):
    """the process-wide Sim3 sampling engine's state (Ransac<Sim3Ret>'s own minstd_rand0, apart from pnp_engine's); with `state`, set
    it first and return the old one"""
    return _ransac_engine("sim3", state)


class KeyFrameDB:
    """KeyFrameDB's place-recognition index on one device (orbfe_kfdb, include/orbfe.h): keyframes keyed by uint64 id, each one's BowVector
    (the words / values that Context.bow_transform / bow_slots return).  Any Context on the same device queries it."""

    def __init__(self, n_words, device_id=0):
        self.lib = load()
        h = C.c_void_p(None)
        st = self.lib.orbfe_kfdb_create(int(device_id), int(n_words), C.byref(h))
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())
        self.h = h
        self.n_words = int(n_words)

    def _check(self, st):
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbfe_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, ids, words, values, offsets=None):
        """one keyframe (ids an int, words / values its BowVector) or many as a CSR: keyframe i has words[offsets[i]:offsets[i + 1]]"""
        if offsets is None:
            ids = [int(ids)]
            offsets = [0, len(words)]
        i = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        o = np.ascontiguousarray(offsets, np.int64)
        w = np.ascontiguousarray(words, np.uint32)
        v = np.ascontiguousarray(values, np.float64)
        if len(o) != len(i) + 1 or len(w) != len(v) or (len(o) and o[-1] != len(w)):
            raise ValueError("add: offsets must have len(ids) + 1 entries ending at len(words) == len(values)")
        self._check(self.lib.orbfe_kfdb_add(self.h, len(i), ptr(i), ptr(o), ptr(w), ptr(v)))

    def set_bad(self, ids, flags=True):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8), i.shape), np.uint8)
        self._check(self.lib.orbfe_kfdb_set_bad(self.h, len(i), ptr(i), ptr(f)))

    def erase(self, ids):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        self._check(self.lib.orbfe_kfdb_erase(self.h, len(i), ptr(i)))

    def __len__(self):
        n = C.c_int64(0)
        self._check(self.lib.orbfe_kfdb_size(self.h, C.byref(n)))
        return n.value

    @staticmethod
    def _query_in(words, values, ignore, min_score):
        w = np.ascontiguousarray(words, np.uint32)
        v = np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        ig = np.ascontiguousarray(np.asarray(list(ignore) if not isinstance(ignore, np.ndarray) else ignore, np.uint64).reshape(-1))
        ms = None if min_score is None else np.array([float(min_score)], np.float64)
        q = KfdbQueryIn(ptr(w).value if len(w) else None, ptr(v).value if len(v) else None, len(w), ptr(ig).value if len(ig) else None,
                        len(ig), None if ms is None else ptr(ms).value)
        return q, (w, v, ig, ms)   # the arrays stay alive with the structure

    def query(self, ctx, words, values, ignore=(), min_score=None):
        """(ids, counts, scores) of the survivors, ids ascending: relocalisation with min_score None, else loop mode"""
        q, keep = self._query_in(words, values, ignore, min_score)
        cap = max(len(self), 1)
        ids, counts, scores = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap)
        n = C.c_int64(0)
        ctx._check(self.lib.orbfe_kfdb_query(ctx.h, self.h, C.byref(q), ptr(ids), ptr(counts), ptr(scores), cap, C.byref(n)))
        k = n.value
        return ids[:k].copy(), counts[:k].copy(), scores[:k].copy()

    def score(self, ctx, words, values, ids):
        """DBoW's L1 score of the query against each of the keyframes `ids`"""
        q, keep = self._query_in(words, values, (), None)
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        out = np.zeros(len(i))
        ctx._check(self.lib.orbfe_kfdb_score(ctx.h, self.h, C.byref(q), ptr(i), len(i), ptr(out)))
        return out


class KeyframeStore:
    """Keyframes resident on one device, keyed by uint64 id (orbfe_kfstore, include/orbfe.h): features, stereo columns,
    frame bounds, the area grid and -- after set_bow -- the FeatureVector.  Poses and map points are not stored.  Any Context on the same
    device uses it through Context.fuse_into_keyframes_stored / create_new_map_points_stored."""

    def __init__(self, width, height, n_levels=8, device_id=0, slab_bytes=0):
        self.lib = load()
        h = C.c_void_p(None)
        st = self.lib.orbfe_kfstore_create(int(device_id), int(width), int(height), int(n_levels), int(slab_bytes), C.byref(h))
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())
        self.h = h

    def _check(self, st):
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbfe_kfstore_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _bounds(bounds):
        return None if bounds is None else np.ascontiguousarray(bounds, np.float32).reshape(4)

    def add(self, kf_id, kps, desc, depth=None, right_u=None, bounds=None):
        """from host arrays: kps [n] KP_DTYPE, desc [n, 32] uint8, depth / right_u [n] float64 (None: -1), bounds (minU, maxU, minV, maxV)
        (None: the image)"""
        k = np.ascontiguousarray(kps, KP_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if len(d) != len(k):
            raise ValueError("add: kps and desc differ in length")
        dp = None if depth is None else np.ascontiguousarray(depth, np.float64)
        ru = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        if any(a is not None and len(a) != len(k) for a in (dp, ru)):
            raise ValueError("add: depth / right_u must have one entry per feature")
        b = self._bounds(bounds)
        self._check(self.lib.orbfe_kfstore_add(self.h, int(kf_id), len(k), ptr(k), ptr(d), None if dp is None else ptr(dp), None if ru is None else ptr(ru),
                                               None if b is None else ptr(b)))

    def add_from_slot(self, ctx, kf_id, slot, pair=-1, bounds=None):
        """the features of extraction slot `slot` of `ctx` (pair >= 0: with that stereo pair's right_u and depth), device to device -> n"""
        b = self._bounds(bounds)
        n = C.c_int32(0)
        ctx._check(self.lib.orbfe_kfstore_add_from_slot(ctx.h, self.h, int(kf_id), int(slot), int(pair), None if b is None else ptr(b), C.byref(n)))
        return n.value

    def set_bow(self, kf_id, nodes, node_offsets, features):
        """the FeatureVector (bow_transform's last three outputs)"""
        nd = np.ascontiguousarray(nodes, np.uint32)
        of = np.ascontiguousarray(node_offsets, np.int32)
        ft = np.ascontiguousarray(features, np.uint32)
        if len(of) != len(nd) + 1 or (len(of) and 0 <= of[-1] and of[-1] > len(ft)):
            raise ValueError("set_bow: node_offsets must have len(nodes) + 1 entries ending inside features")
        self._check(self.lib.orbfe_kfstore_set_bow(self.h, int(kf_id), len(nd), ptr(nd), ptr(of), ptr(ft)))

    def erase(self, ids):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        self._check(self.lib.orbfe_kfstore_erase(self.h, len(i), ptr(i)))

    def __len__(self):
        n = C.c_int64(0)
        self._check(self.lib.orbfe_kfstore_size(self.h, C.byref(n), None, None))
        return n.value

    def bytes(self):
        """(bytes the entries occupy, bytes of device memory reserved in slabs)"""
        u, r = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.orbfe_kfstore_size(self.h, None, C.byref(u), C.byref(r)))
        return u.value, r.value

    def info(self, kf_id):
        o = KfstoreInfo()
        self._check(self.lib.orbfe_kfstore_info_get(self.h, int(kf_id), C.byref(o)))
        return dict(n=o.n, has_bow=bool(o.has_bow), has_stereo=bool(o.has_stereo), n_nodes=o.n_nodes, n_bow_features=o.n_bow_features, grid=(o.grid_rows, o.grid_cols),
                    bounds=np.array(list(o.bounds), np.float32), bytes=o.bytes)

    def fetch(self, kf_id):
        """the entry as dict(kps, desc, depth, right_u, bounds, cell_off, cell_feat, fv = (nodes, offsets, features) or None)"""
        i = self.info(kf_id)
        n = i["n"]
        out = dict(kps=np.zeros(n, KP_DTYPE), desc=np.zeros((n, 32), np.uint8), depth=np.zeros(n, np.float64), right_u=np.zeros(n, np.float64),
                   cell_off=np.zeros(i["grid"][0] * i["grid"][1] + 1, np.int32), cell_feat=np.zeros(n, np.int32))
        fv = (np.zeros(i["n_nodes"], np.uint32), np.zeros(i["n_nodes"] + 1, np.int32), np.zeros(i["n_bow_features"], np.uint32)) if i["has_bow"] else None
        p = lambda a: ptr(a) if a.size else None  # noqa: E731
        self._check(self.lib.orbfe_kfstore_fetch(self.h, int(kf_id), p(out["kps"]), p(out["desc"]), p(out["depth"]), p(out["right_u"]), p(out["cell_off"]),
                                                 p(out["cell_feat"]), *([None] * 3 if fv is None else [p(a) for a in fv])))
        out["bounds"], out["fv"] = i["bounds"], fv
        return out


MP_POS, MP_NORMAL_DEPTH, MP_DESC, MP_ALL = 1, 2, 4, 7


class MapPointStore:
    """Map points resident on one device, keyed by uint64 id (orbfe_mpstore, include/orbfe.h): a 64-byte row per point --
    pos, view_dir, max_dist, min_dist, desc -- in pages of rows_per_page rows, allocated on first use.  The host objects stay the truth:
    upsert a point when it changed.  Any Context on the same device reads it through Context.track_local_map_stored."""

    def __init__(self, device_id=0, rows_per_page=0, max_pages=0):
        self.lib = load()
        h = C.c_void_p(None)
        st = self.lib.orbfe_mpstore_create(int(device_id), int(rows_per_page), int(max_pages), C.byref(h))
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())
        self.h = h

    def _check(self, st):
        if st != ORBFE_OK:
            raise OrbfeError(st, self.lib.orbfe_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbfe_mpstore_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upsert(self, ids, pos=None, view_dir=None, max_dist=None, min_dist=None, desc=None, fields=None):
        """the arrays that are given (fields None: POS if pos, NORMAL_DEPTH if view_dir, max_dist and min_dist, DESC if desc) into the rows
        of `ids`; an id the store does not hold needs all of them"""
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        n = len(i)
        f32 = lambda a, w: None if a is None else np.ascontiguousarray(a, np.float32).reshape((n, w) if w > 1 else (n,))  # noqa: E731
        pos, view_dir, max_dist, min_dist = f32(pos, 3), f32(view_dir, 3), f32(max_dist, 1), f32(min_dist, 1)
        desc = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        if fields is None:
            fields = (MP_POS if pos is not None else 0) | (MP_NORMAL_DEPTH if all(a is not None for a in (view_dir, max_dist, min_dist)) else 0) | \
                (MP_DESC if desc is not None else 0)
        self._check(self.lib.orbfe_mpstore_upsert(self.h, n, ptr(i), int(fields), ptr(pos), ptr(view_dir), ptr(max_dist), ptr(min_dist), ptr(desc)))

    def erase(self, ids):
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        self._check(self.lib.orbfe_mpstore_erase(self.h, len(i), ptr(i)))

    def fetch(self, ids):
        """the rows of `ids` (an id may repeat) as dict(pos, view_dir, max_dist, min_dist, desc)"""
        i = np.ascontiguousarray(np.atleast_1d(ids), np.uint64)
        n = len(i)
        out = dict(pos=np.zeros((n, 3), np.float32), view_dir=np.zeros((n, 3), np.float32), max_dist=np.zeros(n, np.float32),
                   min_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8))
        self._check(self.lib.orbfe_mpstore_fetch(self.h, n, ptr(i), *[ptr(out[k]) for k in ("pos", "view_dir", "max_dist", "min_dist", "desc")]))
        return out

    def size(self):
        """dict(n_points, bytes_used, bytes_reserved)"""
        n, u, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.orbfe_mpstore_size(self.h, C.byref(n), C.byref(u), C.byref(r)))
        return dict(n_points=n.value, bytes_used=u.value, bytes_reserved=r.value)

    def __len__(self):
        return self.size()["n_points"]


def group_filter(ids, scores, connected):
    """KeyFrameDB::groupFilter on the host: ids / scores of the survivors, connected[i] the ordered covisible ids of survivor i.
    Returns the candidate ids, ascending."""
    i = np.ascontiguousarray(ids, np.uint64).reshape(-1)
    s = np.ascontiguousarray(scores, np.float64).reshape(-1)
    if len(connected) != len(i) or len(s) != len(i):
        raise ValueError("group_filter: ids, scores and connected differ in length")
    off = np.zeros(len(i) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in connected])
    conn = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint64).reshape(-1) for c in connected]) if len(connected) else np.zeros(0), np.uint64)
    out = np.zeros(max(len(i), 1), np.uint64)
    n = C.c_int64(0)
    L = load()
    st = L.orbfe_kfdb_group_filter(len(i), ptr(i), ptr(s), ptr(off), ptr(conn) if len(conn) else None, ptr(out), C.byref(n))
    if st != ORBFE_OK:
        raise OrbfeError(st, L.orbfe_last_error(None).decode())
    return out[:n.value].copy()


def _bow_arrays(n_img, cap):
    c = max(cap, 1)
    return dict(words=np.zeros((n_img, c), np.uint32), values=np.zeros((n_img, c)), n_words=np.zeros(n_img, np.int32),
                nodes=np.zeros((n_img, c), np.uint32), node_offsets=np.zeros((n_img, cap + 1), np.int32),
                features=np.zeros((n_img, c), np.uint32), n_nodes=np.zeros(n_img, np.int32))


def _bow_split(a, i):
    nw, nn = int(a["n_words"][i]), int(a["n_nodes"][i])
    off = a["node_offsets"][i, :nn + 1].copy()
    return (a["words"][i, :nw].copy(), a["values"][i, :nw].copy(), a["nodes"][i, :nn].copy(), off, a["features"][i, :off[-1]].copy())


class Context:
    """Owns one orbfe_ctx (device buffers for `max_images` image slots of one fixed geometry)."""

    def __init__(self, width, height, n_features=2000, n_levels=8, scale_factor=1.2, fast_hi=20, fast_lo=7, brief_pairs=None,
                 blur_variant=0, device_id=0, max_images=2, stream=None, gray_variant=0):
        self.lib = load()
        self._pairs = None
        if brief_pairs is not None:
            self._pairs = np.ascontiguousarray(brief_pairs, np.int8).reshape(256, 4)
        cfg = Config(width, height, n_features, n_levels, scale_factor, fast_hi, fast_lo, ptr(self._pairs), blur_variant,
                     gray_variant, device_id, max_images, stream)
        self.cfg = cfg
        h = C.c_void_p(None)
        st = self.lib.orbfe_create(C.byref(cfg), C.byref(h))
        if st != ORBFE_OK:
            msg = self.lib.orbfe_last_error(None).decode()
            raise (ImageSizeError if st == 2 else OrbfeError)(st, msg)
        self.h = h
        self.width, self.height, self.n_levels, self.max_images = width, height, n_levels, max_images
        self.requested_features = n_features
        self.n_features = int(self.lib.orbfe_get_capacity(h))   # stride of every per-image array (>= the requested count)

    def close(self):
        if getattr(self, "h", None):
            self.lib.orbfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != ORBFE_OK:
            msg = self.lib.orbfe_last_error(self.h).decode()
            raise (ImageSizeError if st == 2 else OrbfeError)(st, msg)

    # ---- geometry ---------------------------------------------------------------------------
    def level_info(self, level) -> LevelInfo:
        li = LevelInfo()
        self._check(self.lib.orbfe_get_level_info(self.h, level, C.byref(li)))
        return li

    def scale_factors(self) -> np.ndarray:
        out = np.zeros(self.n_levels, np.float32)
        self._check(self.lib.orbfe_get_scale_factors(self.h, ptr(out), self.n_levels))
        return out

    # ---- extraction -------------------------------------------------------------------------
    def _host_images(self, imgs):
        """the images as the library reads them (uint8 rows of one stride >= width) and that stride"""
        imgs = [np.asarray(im) for im in imgs]
        for im in imgs:
            if im.shape != (self.height, self.width):
                raise ValueError(f"image shape {im.shape} != context geometry {(self.height, self.width)}")
        # views with padded rows (a cv::Mat ROI / a row-padded camera buffer) go through as they are if they share one row stride
        strides = {im.strides[0] for im in imgs}
        if not (len(strides) == 1 and all(im.dtype == np.uint8 and im.strides[1] == 1 and im.strides[0] >= self.width for im in imgs)):
            imgs = [np.ascontiguousarray(im, np.uint8) for im in imgs]
            strides = {self.width}
        return imgs, (strides.pop() if imgs else self.width)

    def _result_arrays(self, n):
        """the [n][n_features] arrays a call's results land in: kept per context and image count (the first touch of a quarter of a
        megabyte of fresh pages was a fifth of a one-pair call); what the caller gets are copies of the filled parts"""
        cache = self.__dict__.setdefault("_res_cache", {})
        n = (threading.get_ident(), n)  # (a set per calling thread: the copies are taken after the library call has returned)
        if n not in cache:
            nf = max(self.n_features, 1)
            n_img = n[1]
            cache[n] = (np.zeros((max(n_img, 1), nf), KP_DTYPE), np.zeros((max(n_img, 1), nf, 32), np.uint8), np.zeros(max(n_img, 1), np.int32),
                        np.zeros(nf, np.float64), np.zeros(nf, np.float64))
        return cache[n]

    def extract_batch(self, imgs):
        imgs, stride = self._host_images(imgs)
        n = len(imgs)
        arr = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in imgs])
        if n <= 2:
            kps, desc, cnt = self._result_arrays(n)[:3]
        else:
            kps = np.zeros((n, max(self.n_features, 1)), KP_DTYPE)
            desc = np.zeros((n, max(self.n_features, 1), 32), np.uint8)
            cnt = np.zeros(n, np.int32)
        self._check(self.lib.orbfe_extract_batch(self.h, n, arr, stride, ptr(kps), ptr(desc), ptr(cnt)))
        return [(kps[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)]

    def frame_stereo(self, left, right, fx, bf, slot_left=None):
        """orbfe_frame_stereo: both extractions and the stereo match of one frame as one call (Frame::createStereo's device work).
        -> ((kpsL, descL), (kpsR, descR), n_matches, right_u, depth); slot_left (even): orbfe_frame_stereo_slots into that slot pair"""
        (left, right), stride = self._host_images([left, right])
        kps, desc, cnt, ru, dp = self._result_arrays(2)
        nm = C.c_int32(0)
        if slot_left is None:
            self._check(self.lib.orbfe_frame_stereo(self.h, left.ctypes.data, right.ctypes.data, stride, fx, bf, ptr(kps), ptr(desc), ptr(cnt),
                                                    ptr(ru), ptr(dp), C.byref(nm)))
        else:
            self._check(self.lib.orbfe_frame_stereo_slots(self.h, slot_left, left.ctypes.data, right.ctypes.data, stride, fx, bf, ptr(kps),
                                                          ptr(desc), ptr(cnt), ptr(ru), ptr(dp), C.byref(nm)))
        return ((kps[0, :cnt[0]].copy(), desc[0, :cnt[0]].copy()), (kps[1, :cnt[1]].copy(), desc[1, :cnt[1]].copy()), nm.value, ru.copy(), dp.copy())

    def extract(self, img):
        return self.extract_batch([img])[0]

    def extract_slot(self, slot, img):
        """one image -> slot `slot` on the slot's own stream (calls on different slots may run on different threads at once)"""
        img = np.asarray(img)
        if img.shape != (self.height, self.width):
            raise ValueError(f"image shape {img.shape} != context geometry {(self.height, self.width)}")
        if not (img.dtype == np.uint8 and img.strides[1] == 1 and img.strides[0] >= self.width):
            img = np.ascontiguousarray(img, np.uint8)
        nf = max(self.n_features, 1)
        kps = np.zeros(nf, KP_DTYPE)
        desc = np.zeros((nf, 32), np.uint8)
        n = C.c_int32(0)
        self._check(self.lib.orbfe_extract_slot(self.h, slot, img.ctypes.data, img.strides[0], ptr(kps), ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_slot_begin(self, slot, img):
        """orbfe_extract_slot in two halves: stage the image and enqueue the extraction on the slot's lane, return at once"""
        img = np.asarray(img)
        if img.shape != (self.height, self.width):
            raise ValueError(f"image shape {img.shape} != context geometry {(self.height, self.width)}")
        if not (img.dtype == np.uint8 and img.strides[1] == 1 and img.strides[0] >= self.width):
            img = np.ascontiguousarray(img, np.uint8)
        self._check(self.lib.orbfe_extract_slot_begin(self.h, slot, img.ctypes.data, img.strides[0]))

    def extract_slot_end(self, slot):
        """... wait for it and deliver what extract_slot delivers"""
        nf = max(self.n_features, 1)
        kps = np.zeros(nf, KP_DTYPE)
        desc = np.zeros((nf, 32), np.uint8)
        n = C.c_int32(0)
        self._check(self.lib.orbfe_extract_slot_end(self.h, slot, ptr(kps), ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_slots(self, slot0, imgs):
        """len(imgs) images -> the consecutive slots slot0 .. as ONE launch sequence on slot0's lane (orbfe_extract_slots)"""
        n_img = len(imgs)
        arrs = []
        for img in imgs:
            img = np.asarray(img)
            if img.shape != (self.height, self.width):
                raise ValueError(f"image shape {img.shape} != context geometry {(self.height, self.width)}")
            arrs.append(np.ascontiguousarray(img, np.uint8))
        nf = max(self.n_features, 1)
        ptrs = (C.c_void_p * n_img)(*[a.ctypes.data for a in arrs])
        kps = np.zeros((n_img, nf), KP_DTYPE)
        desc = np.zeros((n_img, nf, 32), np.uint8)
        n = np.zeros(n_img, np.int32)
        self._check(self.lib.orbfe_extract_slots(self.h, slot0, n_img, ptrs, self.width, ptr(kps), ptr(desc), ptr(n)))
        return [(kps[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(n_img)]

    def fetch_batch(self, slot0, n_slots):
        """packed results of slots [slot0, slot0 + n_slots): (kps [n][NF], desc [n][NF][32], counts [n])"""
        nf = max(self.n_features, 1)
        kps = np.zeros((n_slots, nf), KP_DTYPE)
        desc = np.zeros((n_slots, nf, 32), np.uint8)
        cnt = np.zeros(n_slots, np.int32)
        self._check(self.lib.orbfe_fetch_batch(self.h, slot0, n_slots, ptr(kps), ptr(desc), ptr(cnt)))
        return kps, desc, cnt

    def fetch_stereo_batch(self, pair0, n_pairs):
        """packed stereo results of pairs [pair0, pair0 + n_pairs): (right_u [n][NF], depth [n][NF], n_matches [n])"""
        nf = max(self.n_features, 1)
        ru = np.zeros((n_pairs, nf), np.float64)
        dp = np.zeros((n_pairs, nf), np.float64)
        nm = np.zeros(n_pairs, np.int32)
        self._check(self.lib.orbfe_fetch_stereo_batch(self.h, pair0, n_pairs, ptr(ru), ptr(dp), ptr(nm)))
        return ru, dp, nm

    def pyramid(self, slot, level, blurred=False) -> np.ndarray:
        li = self.level_info(level)
        out = np.zeros((li.height, li.width), np.uint8)
        self._check(self.lib.orbfe_get_pyramid(self.h, slot, level, int(blurred), ptr(out)))
        return out

    def debug_candidates(self, slot, level) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self.lib.orbfe_debug_candidates(self.h, slot, level, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        self._check(self.lib.orbfe_debug_candidates(self.h, slot, level, ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def debug_se3_oplus(self, poses, upd) -> np.ndarray:
        """exp(upd[i]) * poses[i] by the device's pose_oplus: poses (n, 7) = (q xyzw, t), upd (n, 6) = (omega, upsilon) -> (n, 7)"""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        upd = np.ascontiguousarray(upd, np.float64).reshape(-1, 6)
        if poses.shape[0] != upd.shape[0]:
            raise ValueError("poses / upd disagree in length")
        n = poses.shape[0]
        out = np.zeros((max(n, 1), 7))
        self._check(self.lib.orbfe_debug_se3_oplus(self.h, n, ptr(poses), ptr(upd), ptr(out)))
        return out[:n]

    def debug_reduced_solve(self, solver, S, rhs):
        """S x = rhs (S (6 nb, 6 nb) symmetric positive definite, only its lower triangle counts) by one of local BA's four reduced-system
        solvers: 0 registers (nb 1..42), 1 blocked (43..1000), 2 LDS (1..100), 3 panel (>= 101) -> (x, ok); ok == 0: bad pivot, x = 0"""
        S = np.ascontiguousarray(S, np.float64)
        rhs = np.ascontiguousarray(rhs, np.float64).reshape(-1)
        n = rhs.shape[0]
        if S.shape != (n, n) or n % 6:
            raise ValueError("S must be (6 nb, 6 nb) and rhs (6 nb,)")
        x = np.zeros(max(n, 1))
        ok = C.c_int32(-1)
        self._check(self.lib.orbfe_debug_reduced_solve(self.h, solver, n // 6, ptr(S), ptr(rhs), ptr(x), C.byref(ok)))
        return x[:n], ok.value

    # ---- stereo -------------------------------------------------------------------------------
    def stereo_match(self, slot_left, slot_right, fx, bf):
        nf = max(self.n_features, 1)
        ru = np.zeros(nf, np.float64)
        dp = np.zeros(nf, np.float64)
        br = np.zeros(nf, np.int32)
        bd = np.zeros(nf, np.int32)
        nm = C.c_int32(0)
        self._check(self.lib.orbfe_stereo_match(self.h, slot_left, slot_right, fx, bf, ptr(ru), ptr(dp), C.byref(nm), ptr(br), ptr(bd)))
        return nm.value, ru, dp, br, bd

    def stereo_batch_device(self, d_left_ptr, d_right_ptr, stride, image_pitch, n_pairs, fx, bf):
        self._check(self.lib.orbfe_stereo_batch_device(self.h, d_left_ptr, d_right_ptr, stride, image_pitch, n_pairs, fx, bf))

    def sync(self):
        self._check(self.lib.orbfe_sync(self.h))

    # ---- host-image stream -----------------------------------------------------------------------
    def alloc_batch_results(self, n_pairs, pinned=True):
        """result arrays of one batch for stream_submit: dict of numpy arrays (page-locked unless pinned=False)"""
        nf = max(self.n_features, 1)
        spec = dict(kps=((2 * n_pairs, nf), KP_DTYPE), desc=((2 * n_pairs, nf, 32), np.uint8), counts=((2 * n_pairs,), np.int32),
                    right_u=((n_pairs, nf), np.float64), depth=((n_pairs, nf), np.float64), n_matches=((n_pairs,), np.int32))
        out, keep = {}, []
        for k, (shape, dt) in spec.items():
            if pinned:
                pa = PinnedArray(shape, dt)
                keep.append(pa)
                out[k] = pa.array
            else:
                out[k] = np.zeros(shape, dt)
        out["_pinned"] = keep
        return out

    def stream_submit(self, left, right, n_pairs, fx, bf, out, stride=None, image_pitch=None):
        """left / right: uint8 arrays [n_pairs, H, W] (C-contiguous; page-locked for true overlap) -> ticket"""
        stride = stride or self.width
        image_pitch = image_pitch or stride * self.height
        out = out or {}
        res = BatchResults(*[out[k].ctypes.data if out.get(k) is not None else None
                             for k in ("kps", "desc", "counts", "right_u", "depth", "n_matches")])
        t = C.c_int64(-1)
        self._check(self.lib.orbfe_stream_submit(self.h, left.ctypes.data, right.ctypes.data, stride, image_pitch, n_pairs, fx, bf,
                                                 C.byref(res), C.byref(t)))
        return t.value

    def stream_wait(self, ticket):
        self._check(self.lib.orbfe_stream_wait(self.h, ticket))

    def record_bytes(self) -> int:
        return int(self.lib.orbfe_record_bytes(self.h))

    def stream_pack_records(self, ticket, n_pairs, d_records_ptr):
        """frame records of a live ticket -> device memory at d_records_ptr (n_pairs * record_bytes() bytes); returns when complete"""
        self._check(self.lib.orbfe_stream_pack_records(self.h, ticket, n_pairs, d_records_ptr))

    def stream_device_results(self, ticket, n_pairs):
        """device pointers (ints) of the packed results of a live ticket: dict kps, desc, counts, right_u, depth, n_match"""
        ps = [C.c_void_p(None) for _ in range(6)]
        self._check(self.lib.orbfe_stream_device_results(self.h, ticket, n_pairs, *[C.byref(p) for p in ps]))
        return dict(zip(["kps", "desc", "counts", "right_u", "depth", "n_match"], [p.value for p in ps]))

    def fetch_features(self, slot):
        nf = max(self.n_features, 1)
        kps = np.zeros(nf, KP_DTYPE)
        desc = np.zeros((nf, 32), np.uint8)
        n = C.c_int32(0)
        self._check(self.lib.orbfe_fetch_features(self.h, slot, ptr(kps), ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def fetch_stereo(self, pair):
        nf = max(self.n_features, 1)
        ru = np.zeros(nf, np.float64)
        dp = np.zeros(nf, np.float64)
        br = np.zeros(nf, np.int32)
        bd = np.zeros(nf, np.int32)
        nm = C.c_int32(0)
        self._check(self.lib.orbfe_fetch_stereo(self.h, pair, ptr(ru), ptr(dp), C.byref(nm), ptr(br), ptr(bd)))
        return nm.value, ru, dp, br, bd

    def device_results(self):
        ps = [C.c_void_p(None) for _ in range(6)]
        self._check(self.lib.orbfe_device_results(self.h, *[C.byref(p) for p in ps]))
        return dict(zip(["kps", "desc", "counts", "right_u", "depth", "n_match"], [p.value for p in ps]))

    # ---- matching -----------------------------------------------------------------------------
    def match_bruteforce(self, q, t, cand_offsets=None, cand_idx=None):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        nq, nt = q.shape[0], t.shape[0]
        if cand_offsets is not None:
            cand_offsets = np.ascontiguousarray(cand_offsets, np.uint32)
            cand_idx = np.ascontiguousarray(cand_idx if cand_idx is not None else np.zeros(0), np.uint32)
            assert cand_offsets.size == nq + 1
        bi = np.zeros(max(nq, 1), np.int32)
        bd = np.zeros(max(nq, 1), np.int32)
        sd = np.zeros(max(nq, 1), np.int32)
        self._check(self.lib.orbfe_match_bruteforce(self.h, ptr(q), nq, ptr(t), nt, ptr(cand_offsets), ptr(cand_idx), ptr(bi), ptr(bd), ptr(sd)))
        return bi[:nq], bd[:nq], sd[:nq]

    def search_in_area(self, slot, qxy, radius, min_level, max_level, q_desc, exclude=None):
        qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2)
        nq = qxy.shape[0]
        radius = np.ascontiguousarray(radius, np.float32)
        min_level = np.ascontiguousarray(min_level, np.int8)
        max_level = np.ascontiguousarray(max_level, np.int8)
        q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        ex = None
        if exclude is not None:
            ex = np.zeros(max(self.n_features, 1), np.uint8)
            ex[:len(exclude)] = np.asarray(exclude, np.uint8)
        out = [np.zeros(max(nq, 1), np.int32) for _ in range(4)]
        self._check(self.lib.orbfe_search_in_area(self.h, slot, nq, ptr(qxy), ptr(radius), ptr(min_level), ptr(max_level), ptr(q_desc),
                                                  ptr(ex), *[ptr(o) for o in out]))
        return tuple(o[:nq] for o in out)

    def search_in_area_features(self, t_kps, t_desc, qxy, radius, min_level, max_level, q_desc, exclude=None, bounds=None, want_hits=False):
        """orbfe_search_in_area against a caller-supplied feature set (a KeyFrame's keypoints [KP_DTYPE] and descriptors).
        bounds = (min_u, max_u, min_v, max_v) of the target frame (None: the image); want_hits: also return, per excluded feature, how many
        queries had it in their window (orbfe_search_in_area_features_ex)."""
        t_kps = np.ascontiguousarray(t_kps, KP_DTYPE)
        t_desc = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
        nt = t_kps.shape[0]
        qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2)
        nq = qxy.shape[0]
        radius = np.ascontiguousarray(radius, np.float32)
        min_level = np.ascontiguousarray(min_level, np.int8)
        max_level = np.ascontiguousarray(max_level, np.int8)
        q_desc = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        ex = None
        if exclude is not None:
            ex = np.zeros(max(nt, 1), np.uint8)
            ex[:len(exclude)] = np.asarray(exclude, np.uint8)
        out = [np.zeros(max(nq, 1), np.int32) for _ in range(4)]
        if bounds is None and not want_hits:
            self._check(self.lib.orbfe_search_in_area_features(self.h, nt, ptr(t_kps), ptr(t_desc), nq, ptr(qxy), ptr(radius), ptr(min_level),
                                                               ptr(max_level), ptr(q_desc), ptr(ex), *[ptr(o) for o in out]))
            return tuple(o[:nq] for o in out)
        bnd = None if bounds is None else np.ascontiguousarray(bounds, np.float32).reshape(4)
        hits = np.zeros(max(nt, 1), np.int32) if want_hits else None
        self._check(self.lib.orbfe_search_in_area_features_ex(self.h, nt, ptr(t_kps), ptr(t_desc), ptr(bnd), nq, ptr(qxy), ptr(radius),
                                                              ptr(min_level), ptr(max_level), ptr(q_desc), ptr(ex), *[ptr(o) for o in out], ptr(hits)))
        res = tuple(o[:nq] for o in out)
        return res + (hits[:nt],) if want_hits else res

    # ---- BA -------------------------------------------------------------------------------------
    def ba_eval_edges(self, poses, points, edge_pose, edge_point, meas, is_stereo, info, huber_delta, fx, fy, cx, cy, bf,
                      jacobians=True):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        edge_pose = np.ascontiguousarray(edge_pose, np.int32)
        edge_point = np.ascontiguousarray(edge_point, np.int32)
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
        is_stereo = np.ascontiguousarray(is_stereo, np.uint8)
        info = np.ascontiguousarray(info, np.float64)
        huber_delta = np.ascontiguousarray(huber_delta, np.float64)
        E = edge_pose.size
        prob = BaProblem(poses.shape[0], points.shape[0], E, ptr(poses).value, ptr(points).value, ptr(edge_pose).value,
                         ptr(edge_point).value, ptr(meas).value, ptr(is_stereo).value, ptr(info).value, ptr(huber_delta).value,
                         fx, fy, cx, cy, bf)
        out = dict(error=np.zeros((E, 3)), chi2=np.zeros(E), rho=np.zeros((E, 2)), depth_positive=np.zeros(E, np.uint8))
        if jacobians:
            out["j_point"] = np.zeros((E, 3, 3))
            out["j_pose"] = np.zeros((E, 3, 6))
        o = BaEdgeOut(ptr(out["error"]).value, ptr(out["chi2"]).value, ptr(out["rho"]).value,
                      ptr(out["j_point"]).value if jacobians else None, ptr(out["j_pose"]).value if jacobians else None,
                      ptr(out["depth_positive"]).value)
        self._check(self.lib.orbfe_ba_eval_edges(self.h, C.byref(prob), C.byref(o)))
        return out

    def ba_build_system(self, poses, points, edge_pose, edge_point, meas, is_stereo, info, huber_delta, fx, fy, cx, cy, bf,
                        pose_fixed=None, want_hpl=True):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        edge_pose = np.ascontiguousarray(edge_pose, np.int32)
        edge_point = np.ascontiguousarray(edge_point, np.int32)
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
        is_stereo = np.ascontiguousarray(is_stereo, np.uint8)
        info = np.ascontiguousarray(info, np.float64)
        huber_delta = np.ascontiguousarray(huber_delta, np.float64)
        fixed = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8)
        nk, npt, E = poses.shape[0], points.shape[0], edge_pose.size
        prob = BaProblem(nk, npt, E, ptr(poses).value, ptr(points).value, ptr(edge_pose).value, ptr(edge_point).value,
                         ptr(meas).value, ptr(is_stereo).value, ptr(info).value, ptr(huber_delta).value, fx, fy, cx, cy, bf)
        out = dict(Hpp=np.zeros((nk, 6, 6)), bp=np.zeros((nk, 6)), Hll=np.zeros((npt, 3, 3)), bl=np.zeros((npt, 3)))
        if want_hpl:
            out["Hpl"] = np.zeros((E, 6, 3))
        o = BaSystemOut(ptr(out["Hpp"]).value, ptr(out["bp"]).value, ptr(out["Hll"]).value, ptr(out["bl"]).value,
                        ptr(out["Hpl"]).value if want_hpl else None)
        self._check(self.lib.orbfe_ba_build_system(self.h, C.byref(prob), ptr(fixed), C.byref(o)))
        return out

    def ba_local_optimize(self, prob, pose_fixed=None, iters_first=5, iters_second=10, stop=None):
        """prob: dict with the orbfe_ba_problem arrays (see ba_synth.make_problem) -> dict(poses, points, level, chi2, bad, iters).
        stop: a numpy uint8 array of one element another thread may set to 1 while the call runs (the reference's `bool& isStop`)"""
        f64 = lambda a, shape: np.ascontiguousarray(a, np.float64).reshape(shape)
        poses, points, meas = f64(prob["poses"], (-1, 7)), f64(prob["points"], (-1, 3)), f64(prob["meas"], (-1, 3))
        info, delta = f64(prob["info"], -1), f64(prob["huber_delta"], -1)
        ek = np.ascontiguousarray(prob["edge_pose"], np.int32)
        ep = np.ascontiguousarray(prob["edge_point"], np.int32)
        st = np.ascontiguousarray(prob["is_stereo"], np.uint8)
        fixed = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8)
        nk, npt, E = poses.shape[0], points.shape[0], ek.size
        bp = BaProblem(nk, npt, E, ptr(poses).value, ptr(points).value, ptr(ek).value, ptr(ep).value, ptr(meas).value, ptr(st).value,
                       ptr(info).value, ptr(delta).value, prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
        out = dict(poses=np.zeros((nk, 7)), points=np.zeros((npt, 3)), level=np.zeros(max(E, 1), np.uint8), chi2=np.zeros(max(E, 1)),
                   bad=np.zeros(max(E, 1), np.uint8), iters=np.zeros(2, np.int32))
        o = BaOptimizeOut(ptr(out["poses"]).value, ptr(out["points"]).value, ptr(out["level"]).value, ptr(out["chi2"]).value,
                          ptr(out["bad"]).value, ptr(out["iters"]).value)
        if stop is not None:
            assert isinstance(stop, np.ndarray) and stop.dtype == np.uint8 and stop.size >= 1
        self._check(self.lib.orbfe_ba_local_optimize(self.h, C.byref(bp), ptr(fixed), iters_first, iters_second, ptr(stop), C.byref(o)))
        for k in ("level", "chi2", "bad"):
            out[k] = out[k][:E]
        return out

    def _ba_problem(self, prob):
        """the orbfe_ba_problem of a problem dict and the arrays it points into (keep them alive for the call)"""
        f64 = lambda a, shape: np.ascontiguousarray(a, np.float64).reshape(shape)
        keep = [f64(prob["poses"], (-1, 7)), f64(prob["points"], (-1, 3)), np.ascontiguousarray(prob["edge_pose"], np.int32),
                np.ascontiguousarray(prob["edge_point"], np.int32), f64(prob["meas"], (-1, 3)), np.ascontiguousarray(prob["is_stereo"], np.uint8),
                f64(prob["info"], -1), f64(prob["huber_delta"], -1)]
        nk, npt, E = keep[0].shape[0], keep[1].shape[0], keep[2].size
        bp = BaProblem(nk, npt, E, *[ptr(a).value for a in keep], prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"])
        return bp, keep, (nk, npt, E)

    def ba_global_optimize(self, prob, pose_fixed=None, iterations=10, solver=0, pcg_tol=None, pcg_max_iter=0, stop=None):
        """Optimizer::globalOptimization from the point where the graph is built (orbfe_ba_global_optimize): ONE optimize(iterations) on
        the graph `prob` describes (see ba_synth.make_trajectory_problem), then chi2 of every edge at the final estimates.  solver 0 auto
        (dense up to GBA_DENSE_MAX_FREE non-fixed keyframes), 1 dense, 2 block-sparse PCG -> dict(poses, points, chi2, iters,
        cg_stats = (trials, CG iterations in all, trials the solver rejected))."""
        bp, keep, (nk, npt, E) = self._ba_problem(prob)
        fixed = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8)
        out = dict(poses=np.zeros((nk, 7)), points=np.zeros((npt, 3)), chi2=np.zeros(max(E, 1)), iters=np.zeros(1, np.int32),
                   cg_stats=np.zeros(3, np.int64))
        opt = BaGlobalOptions(int(solver), 0.0 if pcg_tol is None else float(pcg_tol), int(pcg_max_iter))
        o = BaGlobalOut(ptr(out["poses"]).value, ptr(out["points"]).value, ptr(out["chi2"]).value, ptr(out["iters"]).value,
                        ptr(out["cg_stats"]).value)
        if stop is not None:
            assert isinstance(stop, np.ndarray) and stop.dtype == np.uint8 and stop.size >= 1
        self._check(self.lib.orbfe_ba_global_optimize(self.h, C.byref(bp), ptr(fixed), int(iterations), ptr(stop), C.byref(opt), C.byref(o)))
        out["chi2"] = out["chi2"][:E]
        out["iters"] = int(out["iters"][0])
        return out

    @staticmethod
    def ba_global_phases():
        """(build, Schur, PCG, evaluate) milliseconds and the launches of the last ba_global_optimize made with ORBFE_GBA_PHASES set"""
        ms = np.zeros(5)
        load().orbfe_debug_ba_global_phases(ptr(ms))
        return ms

    def debug_ba_reduced_bsr(self, prob, pose_fixed=None, lam=0.0):
        """the block-CSR reduced camera system of ONE linearisation of `prob` at its estimates and lambda `lam` ->
        dict(row_off (nf + 1,), col (nnzb,), blocks (nnzb, 6, 6), rhs (6 nf,))"""
        bp, keep, (nk, npt, E) = self._ba_problem(prob)
        fixed = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8)
        nf = nk if fixed is None else int((fixed == 0).sum())
        nnzb = C.c_int32(0)
        row_off = np.zeros(nf + 1, np.int32)
        self._check(self.lib.orbfe_debug_ba_reduced_bsr(self.h, C.byref(bp), ptr(fixed), float(lam), 0, C.byref(nnzb), ptr(row_off), None, None, None))
        nz = nnzb.value
        col, blocks, rhs = np.zeros(max(nz, 1), np.int32), np.zeros((max(nz, 1), 6, 6)), np.zeros(max(6 * nf, 1))
        self._check(self.lib.orbfe_debug_ba_reduced_bsr(self.h, C.byref(bp), ptr(fixed), float(lam), nz, C.byref(nnzb), ptr(row_off), ptr(col),
                                                        ptr(blocks), ptr(rhs)))
        return dict(row_off=row_off, col=col[:nz], blocks=blocks[:nz], rhs=rhs[:6 * nf])

    def debug_bsr_pcg(self, row_off, col, blocks, rhs, tol=0.0, max_iter=0):
        """one block-CSR system through the conjugate-gradient solver of ba_global_optimize -> (x, iterations, ok)"""
        row_off, col = np.ascontiguousarray(row_off, np.int32), np.ascontiguousarray(col, np.int32)
        blocks, rhs = np.ascontiguousarray(blocks, np.float64).reshape(-1, 36), np.ascontiguousarray(rhs, np.float64)
        nb = row_off.size - 1
        assert rhs.size == 6 * nb and blocks.shape[0] == col.size == row_off[-1]
        x, it, ok = np.zeros(6 * nb), C.c_int32(0), C.c_int32(0)
        self._check(self.lib.orbfe_debug_bsr_pcg(self.h, nb, ptr(row_off), ptr(col), ptr(blocks), ptr(rhs), float(tol), int(max_iter), ptr(x),
                                                 C.byref(it), C.byref(ok)))
        return x, it.value, ok.value

    def project_map_points(self, pos, view_dir, max_dist, min_dist, Rcw, tcw, cam, bounds):
        """MapPoint::isInVision + predictLevel for n map points (MapPoint.cc:141-201); cam = (fx, fy, cx, cy), bounds = (minU, maxU,
        minV, maxV) -> dict(uv, distance, cos_theta, level, visible)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, view_dir, max_dist, min_dist = f32(pos).reshape(-1, 3), f32(view_dir).reshape(-1, 3), f32(max_dist), f32(min_dist)
        n = pos.shape[0]
        m = max(n, 1)
        out = dict(uv=np.zeros((m, 2), np.float32), distance=np.zeros(m, np.float32), cos_theta=np.zeros(m, np.float32),
                   level=np.zeros(m, np.int8), visible=np.zeros(m, np.uint8))
        fp = FramePose((C.c_float * 9)(*f32(Rcw).reshape(9)), (C.c_float * 3)(*f32(tcw).reshape(3)), *[float(np.float32(b)) for b in bounds])
        cm = Camera(*[float(np.float32(v)) for v in cam], 0, 0, 0, 0, 0, 0)
        self._check(self.lib.orbfe_project_map_points(self.h, n, ptr(pos), ptr(view_dir), ptr(max_dist), ptr(min_dist), C.byref(fp),
                                                      C.byref(cm), ptr(out["uv"]), ptr(out["distance"]), ptr(out["cos_theta"]),
                                                      ptr(out["level"]), ptr(out["visible"])))
        return {k: v[:n] for k, v in out.items()}

    def track_local_map(self, slot, pos, view_dir, max_dist, min_dist, desc, flags, Rcw, tcw, cam, bounds, pose_se3, level_sigma2,
                        level_inv_sigma2, held=None, right_u=None, th=3.0, ratio=0.8, min_threshold=50, min_matches=30):
        """Tracking::trackLocalMap's device work as one call (orbfe_track_local_map): searchByProjection(frame, map points, th) against
        the features of `slot`, then OptimizePoseOnly on what the frame holds.  cam = (fx, fy, cx, cy, bf); bounds = (minU, maxU, minV,
        maxV) -> dict(assigned, edge_of, inlier, n_matches, n_edges, n_good, pose)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        pos, view_dir, max_dist, min_dist = f32(pos).reshape(-1, 3), f32(view_dir).reshape(-1, 3), f32(max_dist), f32(min_dist)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        flags = np.ascontiguousarray(flags, np.uint8)
        n, NF = pos.shape[0], self.n_features
        held = None if held is None else np.ascontiguousarray(held, np.int32)
        right_u = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        if (held is not None and held.size != NF) or (right_u is not None and right_u.size != NF):
            raise ValueError("held / right_u must have n_features entries")
        s2, is2, p0 = f32(level_sigma2), f32(level_inv_sigma2), np.ascontiguousarray(pose_se3, np.float64)
        fp = FramePose((C.c_float * 9)(*f32(Rcw).reshape(9)), (C.c_float * 3)(*f32(tcw).reshape(3)), *[float(np.float32(b)) for b in bounds])
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        out = dict(assigned=np.zeros(NF, np.int32), edge_of=np.zeros(NF, np.int32), inlier=np.zeros(NF, np.uint8), pose=np.zeros(7))
        nm, ne, ng = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        ti = TrackInput(n, *[ptr(a) for a in (pos, view_dir, max_dist, min_dist, desc, flags, held, right_u, s2, is2, p0)], th, ratio,
                        min_threshold, min_matches)
        to = TrackOutput(ptr(out["assigned"]), ptr(out["edge_of"]), ptr(out["inlier"]), C.cast(C.byref(nm), C.c_void_p),
                         C.cast(C.byref(ne), C.c_void_p), C.cast(C.byref(ng), C.c_void_p), ptr(out["pose"]))
        self._check(self.lib.orbfe_track_local_map(self.h, slot, C.byref(fp), C.byref(cm), C.byref(ti), C.byref(to)))
        out.update(n_matches=nm.value, n_edges=ne.value, n_good=ng.value)
        return out

    def track_local_map_stored(self, slot, store, ids, flags, Rcw, tcw, cam, bounds, pose_se3, level_sigma2, level_inv_sigma2, held=None,
                               right_u=None, th=3.0, ratio=0.8, min_threshold=50, min_matches=30):
        """track_local_map with the map points named by id in a MapPointStore (orbfe_track_local_map_stored): `ids` in place of pos,
        view_dir, max_dist, min_dist and desc; held indexes `ids`.  Returns what track_local_map returns for the arrays store.fetch(ids)
        gives; an id the store does not hold: OrbfeError(ORBFE_EBADARG)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        flags = np.ascontiguousarray(flags, np.uint8)
        n, NF = len(ids), self.n_features
        if flags.size != n:
            raise ValueError("flags must have one entry per id")
        held = None if held is None else np.ascontiguousarray(held, np.int32)
        right_u = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        if (held is not None and held.size != NF) or (right_u is not None and right_u.size != NF):
            raise ValueError("held / right_u must have n_features entries")
        s2, is2, p0 = f32(level_sigma2), f32(level_inv_sigma2), np.ascontiguousarray(pose_se3, np.float64)
        fp = FramePose((C.c_float * 9)(*f32(Rcw).reshape(9)), (C.c_float * 3)(*f32(tcw).reshape(3)), *[float(np.float32(b)) for b in bounds])
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        out = dict(assigned=np.zeros(NF, np.int32), edge_of=np.zeros(NF, np.int32), inlier=np.zeros(NF, np.uint8), pose=np.zeros(7))
        nm, ne, ng = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        ti = TrackStoredInput(n, *[ptr(a) for a in (ids, flags, held, right_u, s2, is2, p0)], th, ratio, min_threshold, min_matches)
        to = TrackOutput(ptr(out["assigned"]), ptr(out["edge_of"]), ptr(out["inlier"]), C.cast(C.byref(nm), C.c_void_p),
                         C.cast(C.byref(ne), C.c_void_p), C.cast(C.byref(ng), C.c_void_p), ptr(out["pose"]))
        self._check(self.lib.orbfe_track_local_map_stored(self.h, slot, store.h, C.byref(fp), C.byref(cm), C.byref(ti), C.byref(to)))
        out.update(n_matches=nm.value, n_edges=ne.value, n_good=ng.value)
        return out

    def track_motion_model(self, slot, qxy, q_octave, q_min_level, q_max_level, desc, pos, cam, bounds, pose_se3, level_sigma2, level_inv_sigma2,
                           held=None, right_u=None, th=15.0, th_second=30.0, ratio=0.9, min_threshold=50, min_matches=20):
        """The middle of Tracking::trackMotionModel as one call (orbfe_track_motion_model): searchByProjection(frame, lastFrame, th) around the
        last frame's feature positions (radius th * sigma2(octave)) against the features of `slot` (+ the th_second search when fewer than
        min_matches matched), then
        OptimizePoseOnly.  cam = (fx, fy, cx, cy, bf); bounds = (minU, maxU, minV, maxV)
        -> dict(assigned, edge_of, inlier, excluded_hits, query_matches, n_matches, n_edges, n_good, pose, passes)"""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        qxy, pos = f32(qxy).reshape(-1, 2), f32(pos).reshape(-1, 3)
        lo, hi = np.ascontiguousarray(q_min_level, np.int8), np.ascontiguousarray(q_max_level, np.int8)
        octv = np.ascontiguousarray(q_octave, np.int8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n, NF = qxy.shape[0], self.n_features
        if not (pos.shape[0] == n and lo.size == n and hi.size == n and octv.size == n and desc.shape[0] == n):
            raise ValueError("qxy / levels / desc / pos disagree in length")
        held = None if held is None else np.ascontiguousarray(held, np.int32)
        right_u = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        if (held is not None and held.size != NF) or (right_u is not None and right_u.size != NF):
            raise ValueError("held / right_u must have n_features entries")
        s2, is2, p0 = f32(level_sigma2), f32(level_inv_sigma2), np.ascontiguousarray(pose_se3, np.float64)
        b4 = f32(bounds)
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        out = dict(assigned=np.zeros(NF, np.int32), edge_of=np.zeros(NF, np.int32), inlier=np.zeros(NF, np.uint8), pose=np.zeros(7),
                   excluded_hits=np.zeros(NF, np.int32), query_matches=np.zeros(max(n, 1), np.int32))
        nm, ne, ng, np_ = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        mi = MotionInput(n, *[ptr(a) for a in (qxy, octv, lo, hi, desc, pos, held, right_u, s2, is2, p0)], th, th_second, ratio, min_threshold, min_matches)
        to = TrackOutput(ptr(out["assigned"]), ptr(out["edge_of"]), ptr(out["inlier"]), C.cast(C.byref(nm), C.c_void_p),
                         C.cast(C.byref(ne), C.c_void_p), C.cast(C.byref(ng), C.c_void_p), ptr(out["pose"]))
        self._check(self.lib.orbfe_track_motion_model(self.h, slot, ptr(b4), C.byref(cm), C.byref(mi), C.byref(to), ptr(out["excluded_hits"]),
                                                      ptr(out["query_matches"]), C.byref(np_)))
        out.update(n_matches=nm.value, n_edges=ne.value, n_good=ng.value, passes=np_.value, query_matches=out["query_matches"][:n])
        return out

    def map_local_ba(self, pb: bytes, kf_id: int, fx, fy, cx, cy, bf):
        """Optimizer::OptimizeLocalMap around keyframe kf_id of a map.pb -> (updated map.pb bytes, report dict)"""
        cam = Camera(fx, fy, cx, cy, 0, 0, 0, 0, 0, bf)
        n, rep = C.c_size_t(0), MapBaReport()
        out = np.zeros(len(pb) + 4096, np.uint8)  # the result never grows: observations are only erased (-1 takes more bytes than an id, hence the slack)
        st = self.lib.orbfe_map_local_ba(self.h, pb, len(pb), kf_id, C.byref(cam), None, ptr(out), out.size, C.byref(n), C.byref(rep))
        if st == 4:  # ORBFE_ECAPACITY
            out = np.zeros(n.value, np.uint8)
            st = self.lib.orbfe_map_local_ba(self.h, pb, len(pb), kf_id, C.byref(cam), None, ptr(out), out.size, C.byref(n), C.byref(rep))
        self._check(st)
        r = {k: getattr(rep, k) for k, _ in MapBaReport._fields_ if k != "iterations"}
        r["iterations"] = list(rep.iterations)
        return out[:n.value].tobytes(), r

    def pose_only_optimize(self, Xw, meas, info, sigma2, pose, fx, fy, cx, cy, bf):
        Xw = np.ascontiguousarray(Xw, np.float64).reshape(-1, 3)
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
        info = np.ascontiguousarray(info, np.float64)
        sigma2 = np.ascontiguousarray(sigma2, np.float32)
        pose = np.ascontiguousarray(pose, np.float64)
        n = Xw.shape[0]
        out = np.zeros(7)
        inl = np.zeros(max(n, 1), np.uint8)
        ng = C.c_int32(0)
        self._check(self.lib.orbfe_pose_only_optimize(self.h, n, ptr(Xw), ptr(meas), ptr(info), ptr(sigma2), ptr(pose), fx, fy, cx, cy,
                                                      bf, ptr(out), ptr(inl), C.byref(ng)))
        return ng.value, out, inl[:n].astype(bool)

    @staticmethod
    def _sim3_pairs(pc, pm, uv_c, uv_m, info_c, info_m):
        pc = np.ascontiguousarray(pc, np.float32).reshape(-1, 3)
        pm = np.ascontiguousarray(pm, np.float32).reshape(-1, 3)
        uv_c = np.ascontiguousarray(uv_c, np.float32).reshape(-1, 2)
        uv_m = np.ascontiguousarray(uv_m, np.float32).reshape(-1, 2)
        info_c = np.ascontiguousarray(info_c, np.float64).reshape(-1)
        info_m = np.ascontiguousarray(info_m, np.float64).reshape(-1)
        n = pc.shape[0]
        if not all(a.shape[0] == n for a in (pm, uv_c, uv_m, info_c, info_m)):
            raise ValueError("the pair arrays disagree in length")
        return n, (pc, pm, uv_c, uv_m, info_c, info_m)

    def sim3_optimize(self, pc, pm, uv_c, uv_m, info_c, info_m, cam, model):
        """Optimizer::OptimizeSim3 on n matches (orbfe_sim3_optimize): pc = cPc, pm = mPc (n, 3), uv_c, uv_m (n, 2) the key points,
        info_c, info_m (n,) the edges' information, cam = (fx, fy, cx, cy), model float32[12] (R row-major, t: sim3_iterate's layout)
        -> (n_inliers, model float32[12], flags bool (n,), est float64[8] = qx qy qz qw tx ty tz s).  n_inliers == 0 with fewer than 20
        pairs left: the model comes back untouched and every flag set."""
        n, arrs = self._sim3_pairs(pc, pm, uv_c, uv_m, info_c, info_m)
        model = np.array(model, np.float32).reshape(12)
        flags = np.zeros(max(n, 1), np.uint8)
        est = np.zeros(8)
        ni = C.c_int32(-1)
        self._check(self.lib.orbfe_sim3_optimize(self.h, n, *(ptr(a) for a in arrs), *(float(v) for v in cam), ptr(model), ptr(flags),
                                                 C.byref(ni), ptr(est)))
        return ni.value, model, flags[:n].astype(bool), est

    def debug_sim3_edges(self, pc, pm, uv_c, uv_m, info_c, info_m, cam, est):
        """the edges of sim3_optimize at the estimate est (8 doubles) -> (err (n, 4), chi2 (n, 2), jac (n, 2, 2, 6))"""
        n, arrs = self._sim3_pairs(pc, pm, uv_c, uv_m, info_c, info_m)
        est = np.ascontiguousarray(est, np.float64).reshape(8)
        err, chi2, jac = np.zeros((max(n, 1), 4)), np.zeros((max(n, 1), 2)), np.zeros((max(n, 1), 2, 2, 6))
        self._check(self.lib.orbfe_debug_sim3_edges(self.h, n, *(ptr(a) for a in arrs), *(float(v) for v in cam), ptr(est), ptr(err),
                                                    ptr(chi2), ptr(jac)))
        return err[:n], chi2[:n], jac[:n]

    @staticmethod
    def _pose_graph(estimates, fixed, edges, meas):
        est = np.ascontiguousarray(estimates, np.float64).reshape(-1, 8)
        fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
        edges = np.asarray(edges, np.int32).reshape(-1, 2)
        v0, v1 = np.ascontiguousarray(edges[:, 0]), np.ascontiguousarray(edges[:, 1])
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 8)
        if fixed.shape[0] != est.shape[0] or meas.shape[0] != edges.shape[0]:
            raise ValueError("the graph's arrays disagree in length")
        g = PoseGraph(est.shape[0], edges.shape[0], ptr(est), ptr(fixed), ptr(v0), ptr(v1), ptr(meas))
        return g, (est, fixed, v0, v1, meas)  # (the arrays must outlive the call)

    def pose_graph_optimize(self, estimates, fixed, edges, meas, iterations=20, solver=None):
        """Optimizer::optimizeEssentialGraph from the point where the graph is built (orbfe_pose_graph_optimize): estimates (nv, 8) =
        qx qy qz qw tx ty tz s with s == 1, fixed (nv,), edges (ne, 2) = (vertex 0, vertex 1), meas (ne, 8)
        -> (estimates (nv, 8), chi2 (ne,) at them, (iterations run, trials run)).
        solver 0 (auto), 1 (dense) or 2 (block-sparse Cholesky) goes through orbfe_pose_graph_optimize_ex and the third value becomes
        (iterations run, trials run, solver used, blocks of the factor)."""
        g, keep = self._pose_graph(estimates, fixed, edges, meas)
        out = keep[0].copy()
        chi2 = np.zeros(max(g.n_edges, 1))
        if solver is not None:
            stats = np.zeros(4, np.int32)
            opt = PoseGraphOptions(int(solver))
            self._check(self.lib.orbfe_pose_graph_optimize_ex(self.h, C.byref(g), int(iterations), C.byref(opt), ptr(out), ptr(chi2), ptr(stats)))
            return out, chi2[:g.n_edges], tuple(int(v) for v in stats)
        stats = np.zeros(2, np.int32)
        self._check(self.lib.orbfe_pose_graph_optimize(self.h, C.byref(g), int(iterations), ptr(out), ptr(chi2), ptr(stats)))
        return out, chi2[:g.n_edges], (int(stats[0]), int(stats[1]))

    def debug_pg_sparse_solve(self, nb, low_row, low_col, blocks, rhs):
        """one block-sparse SPD system (its lower 6x6 blocks, row-major) through the symbolic phase and the factor-and-solve kernel of
        pose_graph_optimize's solver 2 -> (x (6 nb,), ok, blocks of the factor)"""
        low_row, low_col = np.ascontiguousarray(low_row, np.int32), np.ascontiguousarray(low_col, np.int32)
        blocks, rhs = np.ascontiguousarray(blocks, np.float64).reshape(-1, 36), np.ascontiguousarray(rhs, np.float64)
        assert rhs.size == 6 * nb and blocks.shape[0] == low_row.size == low_col.size
        x, ok, lb = np.zeros(6 * nb), C.c_int32(-1), C.c_int64(0)
        self._check(self.lib.orbfe_debug_pg_sparse_solve(self.h, int(nb), low_row.size, ptr(low_row), ptr(low_col), ptr(blocks), ptr(rhs), ptr(x),
                                                         C.byref(ok), C.byref(lb)))
        return x, ok.value, lb.value

    def debug_pose_graph_phases(self):
        """(build, assemble, solve, evaluate) milliseconds of the last pose_graph_optimize made with ORBFE_PG_PHASES set"""
        ms = np.zeros(4)
        self._check(self.lib.orbfe_debug_pose_graph_phases(ptr(ms)))
        return tuple(float(v) for v in ms)

    def debug_pose_graph_edges(self, estimates, fixed, edges, meas):
        """the edges of pose_graph_optimize at the given estimates -> (err (ne, 6), chi2 (ne,), jac (ne, 2, 6, 6) = [vertex][row][d])"""
        g, keep = self._pose_graph(estimates, fixed, edges, meas)
        n = g.n_edges
        err, chi2, jac = np.zeros((max(n, 1), 6)), np.zeros(max(n, 1)), np.zeros((max(n, 1), 2, 6, 6))
        self._check(self.lib.orbfe_debug_pose_graph_edges(self.h, C.byref(g), ptr(err), ptr(chi2), ptr(jac)))
        return err[:n], chi2[:n], jac[:n]

    # ---- frame glue ------------------------------------------------------------------------------
    def extract_color(self, img: np.ndarray, order: int):
        """img: (h, w, 3) uint8, order 1 = RGB / 2 = BGR -> (keypoints, descriptors) of slot 0.  A view whose rows are further apart
        than 3 w bytes (its last two axes contiguous) is passed as it is, with its row stride."""
        img = _row_strided(img, (np.uint8,))
        assert img.shape == (self.height, self.width, 3)
        kps = np.zeros(max(self.n_features, 1), KP_DTYPE)
        desc = np.zeros((max(self.n_features, 1), 32), np.uint8)
        n = C.c_int32(0)
        self._check(self.lib.orbfe_extract_color(self.h, ptr(img), img.strides[0], order, ptr(kps), ptr(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def frame_rgbd(self, slot, cam: dict, depth=None, depth_scale=1.0):
        """cam: dict(fx fy cx cy k1 k2 p1 p2 k3 bf) -> (undistorted keypoints, depth, right_u); depth None: undistortion only.
        depth: (h, w) uint16 / float32; a column range of a larger image is passed as it is, with the larger image's row stride."""
        cm = Camera(*[float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf")])
        nf = max(self.n_features, 1)
        kps = np.zeros(nf, KP_DTYPE)
        d, ru = np.zeros(nf), np.zeros(nf)
        dtype, stride = 0, 0
        if depth is not None:
            depth = _row_strided(depth, (np.uint16, np.float32))
            assert depth.dtype in (np.uint16, np.float32) and depth.shape == (self.height, self.width)
            dtype, stride = (0 if depth.dtype == np.uint16 else 1), depth.strides[0]
        self._check(self.lib.orbfe_frame_rgbd(self.h, slot, C.byref(cm), ptr(depth), dtype, stride, depth_scale, ptr(kps), ptr(d), ptr(ru)))
        return kps, d, ru   # [n_features] each; entries past the slot's keypoint count are zero (kps) / -1

    def frame_rgbd_image(self, img, cam: dict, depth=None, depth_scale=1.0, color_order=0, slot=0):
        """orbfe_frame_rgbd_image: (colour -> gray,) extraction, undistortion and the depth / rightU lookup of one RGB-D frame as one call
        (Frame::createRGBD's device work).  img: (h, w) uint8, or (h, w, 3) with color_order 1 (RGB) / 2 (BGR).
        -> (undistorted keypoints [n], descriptors [n], depth [n_features], right_u [n_features])"""
        img = np.asarray(img)
        want = (self.height, self.width, 3) if color_order else (self.height, self.width)
        if img.shape != want:
            raise ValueError(f"image shape {img.shape} != {want}")
        img = _row_strided(img, (np.uint8,))    # (row-strided views of the image and of the depth go through with their strides)
        cm = Camera(*[float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf")])
        nf = max(self.n_features, 1)
        kps, desc = np.zeros(nf, KP_DTYPE), np.zeros((nf, 32), np.uint8)
        d, ru = np.zeros(nf), np.zeros(nf)
        n = C.c_int32(0)
        dtype, stride = 0, 0
        if depth is not None:
            depth = _row_strided(depth, (np.uint16, np.float32))
            assert depth.dtype in (np.uint16, np.float32) and depth.shape == (self.height, self.width)
            dtype, stride = (0 if depth.dtype == np.uint16 else 1), depth.strides[0]
        self._check(self.lib.orbfe_frame_rgbd_image(self.h, slot, img.ctypes.data, img.strides[0], color_order, C.byref(cm), ptr(depth), dtype,
                                                    stride, depth_scale, ptr(kps), ptr(desc), C.byref(n), ptr(d), ptr(ru)))
        return kps[:n.value].copy(), desc[:n.value].copy(), d, ru

    # ---- bag of words (DBoW3 Vocabulary::transform) ------------------------------------------------------
    def bow_transform(self, vocab: Vocabulary, desc, levelsup=4):
        """(words, values, nodes, offsets, features) of n host descriptors [n][32]: BowVector words / values, FeatureVector nodes and
        their feature lists features[offsets[i]:offsets[i + 1]]"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        a = _bow_arrays(1, n)
        o = BowOut(*[ptr(a[k]).value for k, _ in BowOut._fields_])
        self._check(self.lib.orbfe_bow_transform(self.h, vocab.h, ptr(d), n, int(levelsup), C.byref(o)))
        return _bow_split(a, 0)

    def bow_slots(self, vocab: Vocabulary, slot0, n, levelsup=4, step=1):
        """bow_transform of the descriptors the last extraction left in slots slot0, slot0 + step, .. (n slots), read on the device: a list
        of n tuples (step 2: the left images of a batch of stereo pairs)"""
        a = _bow_arrays(n, self.n_features)
        o = BowOut(*[ptr(a[k]).value for k, _ in BowOut._fields_])
        self._check(self.lib.orbfe_bow_slots(self.h, vocab.h, slot0, n, step, int(levelsup), C.byref(o)))
        return [_bow_split(a, i) for i in range(n)]

    # ---- new map points of a keyframe ------------------------------------------------------------------------------------------
    def create_new_map_points(self, cur, nbs, cam, k_inv, bl, scale_factors, cap=None, tail_cap=None):
        """LocalMapping::createNewMapPoints' loops 1 and 2 (orbfe_create_new_map_points, include/orbfe.h) for the current keyframe `cur`
        against the neighbours `nbs` in the given order.  A keyframe is a dict: kps [n] KP_DTYPE, desc [n, 32] uint8, fv = (nodes,
        offsets, features) -- bow_transform's last three outputs --, flags [n] uint8 (1: map point good, 2: in map), depth [n], right_u
        [n] (float64), Tcw, Twc (4x4 float32), Ow [3]; cur also unproc [n] (bool) and unproc_pos [n, 3] (float32).  cam = (fx, fy, cx,
        cy).  Returns (records TRI_REC_DTYPE in processing order, tail int32, consumed [n] bool: the features whose unprocessed point
        an own-stereo candidate took, which loop 2 erases from mmUnprocessMps)."""
        keep = []

        def arr(a, dt, shape=None):
            a = np.ascontiguousarray(a, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        def kf(d, with_unproc):
            n = len(d["kps"])
            nodes, offs, feats = d["fv"]
            k = TriKf()
            k.n = n
            k.kps = ptr(arr(d["kps"], KP_DTYPE)).value
            k.desc = ptr(arr(d["desc"], np.uint8, (-1, 32))).value
            nodes = arr(nodes, np.uint32)
            k.n_nodes = len(nodes)
            k.nodes = ptr(nodes).value
            k.node_offsets = ptr(arr(offs, np.int32)).value
            k.features = ptr(arr(feats, np.uint32)).value
            k.flags = ptr(arr(d["flags"], np.uint8)).value
            k.depth = ptr(arr(d["depth"], np.float64)).value
            k.right_u = ptr(arr(d["right_u"], np.float64)).value
            k.Tcw[:] = [float(v) for v in np.asarray(d["Tcw"], np.float32).reshape(16)]
            k.Twc[:] = [float(v) for v in np.asarray(d["Twc"], np.float32).reshape(16)]
            k.Ow[:] = [float(v) for v in np.asarray(d["Ow"], np.float32).reshape(3)]
            if with_unproc:
                k.unproc = ptr(arr(np.asarray(d["unproc"]).astype(bool), np.uint8)).value
                k.unproc_pos = ptr(arr(d["unproc_pos"], np.float32, (-1, 3))).value
            return k

        c = kf(cur, True)
        nb = (TriKf * max(len(nbs), 1))(*[kf(d, False) for d in nbs])
        n = len(cur["kps"])
        cap = n if cap is None else int(cap)
        tail_cap = n if tail_cap is None else int(tail_cap)
        recs = np.zeros(max(cap, 1), TRI_REC_DTYPE)
        tail = np.zeros(max(tail_cap, 1), np.int32)
        consumed = np.zeros(max(n, 1), np.uint8)
        cm = Camera(*[float(v) for v in cam[:4]])
        ki = arr(k_inv, np.float32, (9,))
        sf = arr(scale_factors, np.float32)
        nr, nt = C.c_int64(0), C.c_int64(0)
        st = self.lib.orbfe_create_new_map_points(self.h, C.byref(c), len(nbs), C.cast(nb, C.c_void_p), C.byref(cm), ptr(ki), float(bl),
                                                  ptr(sf), len(sf), ptr(recs), cap, C.byref(nr), ptr(tail), tail_cap, C.byref(nt),
                                                  ptr(consumed))
        self.last_counts = (nr.value, nt.value)
        self._check(st)
        return recs[:nr.value].copy(), tail[:nt.value].copy(), consumed[:n].astype(bool)

    # ---- the inverse fuses of a new keyframe -------------------------------------------------------------------------------------
    def fuse_into_keyframes(self, cur, pts, targets, z, cam, bl, scale_factors, th=3.0, ratio=0.6, dist_threshold=50, out=None):
        """The K inverse fuses of LocalMapping::fuseMapPoints as one call (orbfe_fuse_into_keyframes, include/orbfe.h).  cur and every
        target: dict(kps [n] KP_DTYPE, desc [n, 32] uint8, Rcw [3, 3], tcw [3], bounds = (minU, maxU, minV, maxV)); pts: dict(has_point
        [n], pos [n, 3], view_dir [n, 3], max_dist [n], min_dist [n]) per feature of cur; z [K]: tlc.z of every target
        (ORBMatcher.cc:274-276); cam = (fx, fy, cx, cy).  Returns (best_idx int32, best_dist int32, visible uint8), each [K, n].
        out: the three arrays to write into (C-contiguous, [K, n]) instead of fresh ones."""
        keep = []

        def arr(a, dt, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        def vptr(a):
            return None if a is None else ptr(a).value

        def kf(d):
            k = FuseKf()
            k.n = len(d["kps"])
            k.kps = vptr(arr(d["kps"], KP_DTYPE))
            k.desc = vptr(arr(d["desc"], np.uint8, (-1, 32)))
            k.Rcw[:] = [float(v) for v in np.asarray(d["Rcw"], np.float32).reshape(9)]
            k.tcw[:] = [float(v) for v in np.asarray(d["tcw"], np.float32).reshape(3)]
            k.bounds[:] = [float(np.float32(v)) for v in d["bounds"]]
            return k

        c = kf(cur)
        n, K = c.n, len(targets)
        tg = (FuseKf * max(K, 1))(*[kf(d) for d in targets])
        p = FusePoints()
        has = pts.get("has_point")
        p.has_point = vptr(arr(None if has is None else np.asarray(has).astype(bool), np.uint8))
        p.pos = vptr(arr(pts.get("pos"), np.float32, (-1, 3)))
        p.view_dir = vptr(arr(pts.get("view_dir"), np.float32, (-1, 3)))
        p.max_dist = vptr(arr(pts.get("max_dist"), np.float32))
        p.min_dist = vptr(arr(pts.get("min_dist"), np.float32))
        zz = arr(z, np.float32)
        sf = arr(scale_factors, np.float32)
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]])
        if out is None:
            out = (np.zeros((K, n), np.int32), np.zeros((K, n), np.int32), np.zeros((K, n), np.uint8))
        bi, bd, vis = out
        # (kept with the arrays behind them: tools/fuse_bench.py times the bare C call with the same arguments)
        self._fuse_args = (self.h, C.byref(c), C.byref(p), K, C.cast(tg, C.c_void_p), ptr(zz), C.byref(cm), float(np.float32(bl)), ptr(sf), len(sf),
                           float(np.float32(th)), float(np.float32(ratio)), int(dist_threshold), ptr(bi), ptr(bd), ptr(vis))
        self._fuse_keep = (keep, c, p, tg, cm, bi, bd, vis)
        self._check(self.lib.orbfe_fuse_into_keyframes(*self._fuse_args))
        return bi, bd, vis

    # ---- the same two calls over keyframes resident in a KeyframeStore ------------------------------------------------------------------
    def fuse_into_keyframes_stored(self, store, cur_id, pts, target_ids, poses, z, cam, bl, scale_factors, th=3.0, ratio=0.6, dist_threshold=50,
                                   out=None):
        """fuse_into_keyframes with the keyframes named by id in `store` (orbfe_fuse_into_keyframes_stored): poses = [(Rcw, tcw)] per target
        (or dicts with those keys); everything else, and the result, as fuse_into_keyframes."""
        keep = []

        def arr(a, dt, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        def vptr(a):
            return None if a is None else ptr(a).value

        K = len(target_ids)
        n = store.info(cur_id)["n"]
        ids = arr(target_ids, np.uint64)
        ps = (FusePose * max(K, 1))()
        for k, pz in enumerate(poses):
            R, t = (pz["Rcw"], pz["tcw"]) if isinstance(pz, dict) else pz
            ps[k].Rcw[:] = [float(v) for v in np.asarray(R, np.float32).reshape(9)]
            ps[k].tcw[:] = [float(v) for v in np.asarray(t, np.float32).reshape(3)]
        p = FusePoints()
        has = pts.get("has_point")
        rows = [arr(None if has is None else np.asarray(has).astype(bool), np.uint8), arr(pts.get("pos"), np.float32, (-1, 3)),
                arr(pts.get("view_dir"), np.float32, (-1, 3)), arr(pts.get("max_dist"), np.float32), arr(pts.get("min_dist"), np.float32)]
        p.has_point, p.pos, p.view_dir, p.max_dist, p.min_dist = [vptr(x) for x in rows]
        zz = arr(z, np.float32)
        sf = arr(scale_factors, np.float32)
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]])
        # the library sizes every row array by the STORED feature count: arrays of another length would be read or written past their end
        if any(x is not None and len(x) != n for x in rows) or len(poses) != K or (zz is not None and len(zz) != K):
            raise ValueError(f"fuse_into_keyframes_stored: keyframe {cur_id} has {n} features and there are {K} targets; pts / poses / z do not match")
        if out is None:
            out = (np.zeros((K, n), np.int32), np.zeros((K, n), np.int32), np.zeros((K, n), np.uint8))
        bi, bd, vis = out
        if any(x.size < K * n or not x.flags.c_contiguous for x in out) or (bi.dtype, bd.dtype, vis.dtype) != (np.int32, np.int32, np.uint8):
            raise ValueError("fuse_into_keyframes_stored: out must be C-contiguous int32, int32, uint8 arrays of at least [K, n]")
        # (kept with the arrays behind them: tools/kfstore_bench.py times the bare C call with the same arguments)
        self._fuse_stored_args = (self.h, store.h, int(cur_id), n, C.byref(p), K, vptr(ids), C.cast(ps, C.c_void_p), vptr(zz), C.byref(cm),
                                  float(np.float32(bl)), ptr(sf), len(sf), float(np.float32(th)), float(np.float32(ratio)), int(dist_threshold),
                                  ptr(bi), ptr(bd), ptr(vis))
        self._fuse_stored_keep = (keep, p, ps, cm, bi, bd, vis)
        self._check(self.lib.orbfe_fuse_into_keyframes_stored(*self._fuse_stored_args))
        return bi, bd, vis

    def create_new_map_points_stored(self, store, cur_id, cur, nb_ids, nbs, cam, k_inv, bl, scale_factors, cap=None, tail_cap=None):
        """create_new_map_points with the keyframes named by id in `store` (orbfe_create_new_map_points_stored).  cur and every entry of nbs
        carry only the map state: flags [n], Tcw, Twc, Ow; cur also unproc and unproc_pos (other keys are ignored, so the dicts of
        create_new_map_points pass).  Returns what create_new_map_points returns."""
        keep = []

        def arr(a, dt, shape=None):
            a = np.ascontiguousarray(a, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        def state(d, with_unproc):
            k = TriState()
            fl = arr(d["flags"], np.uint8)
            k.n = len(fl)
            k.flags = ptr(fl).value
            k.Tcw[:] = [float(v) for v in np.asarray(d["Tcw"], np.float32).reshape(16)]
            k.Twc[:] = [float(v) for v in np.asarray(d["Twc"], np.float32).reshape(16)]
            k.Ow[:] = [float(v) for v in np.asarray(d["Ow"], np.float32).reshape(3)]
            if with_unproc:
                k.unproc = ptr(arr(np.asarray(d["unproc"]).astype(bool), np.uint8)).value
                k.unproc_pos = ptr(arr(d["unproc_pos"], np.float32, (-1, 3))).value
            return k

        c = state(cur, True)
        nb = (TriState * max(len(nbs), 1))(*[state(d, False) for d in nbs])
        ids = arr(nb_ids, np.uint64)
        n = c.n
        unproc, unproc_pos = np.asarray(cur["unproc"]), np.asarray(cur["unproc_pos"], np.float32).reshape(-1, 3)
        if len(ids) != len(nbs) or len(unproc) != n or len(unproc_pos) != n:
            raise ValueError("create_new_map_points_stored: one id per neighbour state, unproc / unproc_pos of cur's length")
        cap = n if cap is None else int(cap)
        tail_cap = n if tail_cap is None else int(tail_cap)
        recs = np.zeros(max(cap, 1), TRI_REC_DTYPE)
        tail = np.zeros(max(tail_cap, 1), np.int32)
        consumed = np.zeros(max(n, 1), np.uint8)
        cm = Camera(*[float(v) for v in cam[:4]])
        ki = arr(k_inv, np.float32, (9,))
        sf = arr(scale_factors, np.float32)
        nr, nt = C.c_int64(0), C.c_int64(0)
        self._tri_stored_args = (self.h, store.h, int(cur_id), C.byref(c), len(nbs), ptr(ids), C.cast(nb, C.c_void_p), C.byref(cm), ptr(ki), float(bl),
                                 ptr(sf), len(sf), ptr(recs), cap, C.byref(nr), ptr(tail), tail_cap, C.byref(nt), ptr(consumed))
        self._tri_stored_keep = (keep, c, nb, cm, recs, tail, consumed, nr, nt)
        st = self.lib.orbfe_create_new_map_points_stored(*self._tri_stored_args)
        self.last_counts = (nr.value, nt.value)
        self._check(st)
        return recs[:nr.value].copy(), tail[:nt.value].copy(), consumed[:n].astype(bool)

    def search_by_bow_stored(self, store, query, kf_ids, kf_flags, mode, ratio, dist_threshold, check_orientation, cap=None):
        """ORBMatcher::searchByBow of one query against the keyframes kf_ids of `store` in one call (orbfe_search_by_bow_stored).
        query: an int (the id of a stored keyframe) or a dict(id=..., flags=...) for a stored query, else dict(desc [n, 32], fv = (nodes,
        offsets, features), angle [n] (needed with check_orientation), flags [n] or None).  kf_flags: None or one entry per candidate
        ([n_k] uint8 ORBFE_TRI_GOOD | ORBFE_TRI_INMAP, or None = all 0).  mode: BOW_TRACK / BOW_LOOP / BOW_ADD.  cap None: room for
        every FeatureVector entry of the candidates.  Returns a list of per-candidate BOW_MATCH_DTYPE arrays; self.last_bow_offsets
        holds match_offsets (also after an ECAPACITY failure)."""
        keep = []

        def arr(a, dt, shape=None):
            a = np.ascontiguousarray(a, dt)
            if shape is not None:
                a = a.reshape(shape)
            keep.append(a)
            return a

        q = BowQuery()
        if not isinstance(query, dict):
            query = dict(id=int(query))
        fl = None if query.get("flags") is None else arr(query["flags"], np.uint8)
        if "desc" not in query:
            q.from_store, q.id = 1, int(query["id"])
            q.n = len(fl) if fl is not None else store.info(q.id)["n"]
        else:
            d = arr(query["desc"], np.uint8, (-1, 32))
            nodes, offs, feats = query["fv"]
            nd, of, ft = arr(nodes, np.uint32), arr(offs, np.int32), arr(feats, np.uint32)
            if len(of) != len(nd) + 1 or (0 <= of[-1] and of[-1] > len(ft)):
                raise ValueError("search_by_bow_stored: node_offsets must have len(nodes) + 1 entries ending inside features")
            q.from_store, q.n, q.desc = 0, len(d), ptr(d).value
            if query.get("angle") is not None:
                an = arr(query["angle"], np.float32)
                if len(an) != len(d):
                    raise ValueError("search_by_bow_stored: one angle per query feature")
                q.angle = ptr(an).value
            q.n_nodes, q.nodes, q.node_offsets, q.features = len(nd), ptr(nd).value, ptr(of).value, ptr(ft).value
            if fl is not None and len(fl) != len(d):
                raise ValueError("search_by_bow_stored: one flag per query feature")
        if fl is not None:
            q.flags = ptr(fl).value
        ids = arr(kf_ids, np.uint64).reshape(-1)
        K = len(ids)
        kf_flags = [None] * K if kf_flags is None else list(kf_flags)
        if len(kf_flags) != K:
            raise ValueError("search_by_bow_stored: one flags entry (or None) per candidate")
        fp = (C.c_void_p * max(K, 1))()
        for i, f in enumerate(kf_flags):
            fp[i] = None if f is None else ptr(arr(f, np.uint8)).value
        if cap is None:
            cap = 0
            if K <= BOW_SEARCH_MAX_KF:                       # (more: the call refuses; nothing to size)
                sizes = {}
                for i in ids.tolist():
                    if i not in sizes:
                        o = KfstoreInfo()
                        sizes[i] = o.n_bow_features if self.lib.orbfe_kfstore_info_get(store.h, i, C.byref(o)) == ORBFE_OK else 0
                cap = sum(sizes[i] for i in ids.tolist())
        cap = int(cap)
        out = np.zeros(max(cap, 1), BOW_MATCH_DTYPE)
        offs = np.full(K + 1, -1, np.int64)
        self._bow_search_args = (self.h, store.h, C.byref(q), K, ptr(ids), C.cast(fp, C.c_void_p), int(mode), float(ratio), int(dist_threshold),
                                 int(bool(check_orientation)), ptr(out), cap, ptr(offs))
        self._bow_search_keep = (keep, q, ids, fp, out, offs)
        st = self.lib.orbfe_search_by_bow_stored(*self._bow_search_args)
        self.last_bow_offsets, self.last_bow_matches = offs, out
        self._check(st)
        return [out[offs[k]:offs[k + 1]].copy() for k in range(K)]

    @staticmethod
    def _sim3_side(side, keep):
        """dict(id, flags [n] or None, pos [n, 3], max_dist, min_dist, Rcw, tcw; n: the count when flags is None) -> Sim3Side"""
        o = Sim3Side()
        o.id = int(side["id"])
        if side.get("flags") is None:
            o.n = int(side["n"])
        else:
            fl = np.ascontiguousarray(side["flags"], np.uint8).reshape(-1)
            pos = np.ascontiguousarray(side["pos"], np.float32).reshape(-1, 3)
            mx, mn = np.ascontiguousarray(side["max_dist"], np.float32), np.ascontiguousarray(side["min_dist"], np.float32)
            if not len(fl) == len(pos) == len(mx) == len(mn):
                raise ValueError("search_by_sim3_stored: the arrays of a side differ in length")
            keep += [fl, pos, mx, mn]
            o.n, o.flags, o.pos, o.max_dist, o.min_dist = len(fl), ptr(fl).value, ptr(pos).value, ptr(mx).value, ptr(mn).value
        o.Rcw[:] = np.asarray(side["Rcw"], np.float32).reshape(9).tolist()
        o.tcw[:] = np.asarray(side["tcw"], np.float32).reshape(3).tolist()
        return o

    @staticmethod
    def _sim3_model(model, s):
        """(R [3, 3], t [3]) or 12 floats -> the [12] array of the C call"""
        if isinstance(model, (tuple, list)) and len(model) == 2:
            model = np.concatenate([np.asarray(model[0], np.float32).reshape(9), np.asarray(model[1], np.float32).reshape(3)])
        return np.ascontiguousarray(model, np.float32).reshape(12), float(np.float32(s))

    def search_by_sim3_stored(self, store, cur, match, model, s, matches, cam, scale_factors, th, ratio, dist_threshold, cap=None):
        """ORBMatcher::searchBySim3(mpCurr, mpMatch, matches, g2oScm, th) over two stored keyframes in one call
        (orbfe_search_by_sim3_stored).  cur / match: dict(id, flags [n] uint8 ORBFE_TRI_GOOD | ORBFE_TRI_INMAP or None (then n), pos [n, 3],
        max_dist [n], min_dist [n], Rcw, tcw); model: (R, t) or 12 floats, p_c = s R p_m + t; matches: [(query in cur, train in match)];
        cam: (fx, fy, cx, cy).  Returns the NEW pairs [(query, train)] in ascending query; self.last_sim3_new holds *n_new (also after an
        ECAPACITY failure)."""
        keep = []
        c_side, m_side = self._sim3_side(cur, keep), self._sim3_side(match, keep)
        mdl, s = self._sim3_model(model, s)
        pairs = np.asarray([(m[0], m[1]) for m in matches], np.int32).reshape(-1, 2)
        mt = np.zeros(len(pairs), BOW_MATCH_DTYPE)
        mt["query"], mt["train"] = pairs[:, 0], pairs[:, 1]
        sf = np.ascontiguousarray(scale_factors, np.float32)
        cm = Camera(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), 0.0)
        cap = min(c_side.n, 1 << 30) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), BOW_MATCH_DTYPE)
        n_new = C.c_int32(-1)
        self._sim3_search_args = (self.h, store.h, C.byref(c_side), C.byref(m_side), ptr(mdl), s, len(mt), ptr(mt) if len(mt) else None, C.byref(cm),
                                  ptr(sf), len(sf), float(th), float(ratio), int(dist_threshold), ptr(out), cap, C.byref(n_new))
        self._sim3_search_keep = (keep, c_side, m_side, mdl, mt, cm, sf, out, n_new)
        st = self.lib.orbfe_search_by_sim3_stored(*self._sim3_search_args)
        self.last_sim3_new, self.last_sim3_out = n_new.value, out
        self._check(st)
        return list(zip(out["query"][:n_new.value].tolist(), out["train"][:n_new.value].tolist()))

    def search_by_sim3_points_stored(self, store, kf_id, pts, model, s, cam, scale_factors, th, ratio, dist_threshold):
        """ORBMatcher::searchBySim3(pCurr, vLoopGroupMps, vMatchedMps, g2oScw, th) against the stored keyframe kf_id in one call
        (orbfe_search_by_sim3_points_stored).  pts: dict(usable [m], pos [m, 3], view_dir [m, 3], max_dist [m], min_dist [m], desc [m, 32]);
        model: (R, t) or 12 floats, p_c = s R p_w + t.  Returns (best_idx [m] (-1: none), best_dist [m])."""
        us = np.ascontiguousarray(pts["usable"], np.uint8).reshape(-1)
        pos = np.ascontiguousarray(pts["pos"], np.float32).reshape(-1, 3)
        vd = np.ascontiguousarray(pts["view_dir"], np.float32).reshape(-1, 3)
        mx, mn = np.ascontiguousarray(pts["max_dist"], np.float32), np.ascontiguousarray(pts["min_dist"], np.float32)
        d = np.ascontiguousarray(pts["desc"], np.uint8).reshape(-1, 32)
        m = len(us)
        if not m == len(pos) == len(vd) == len(mx) == len(mn) == len(d):
            raise ValueError("search_by_sim3_points_stored: the point arrays differ in length")
        p = Sim3Points(m, *[ptr(a).value if m else None for a in (us, pos, vd, mx, mn, d)])
        mdl, s = self._sim3_model(model, s)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        cm = Camera(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), 0.0)
        bi, bd = np.full(max(m, 1), -1, np.int32), np.zeros(max(m, 1), np.int32)
        self._check(self.lib.orbfe_search_by_sim3_points_stored(self.h, store.h, int(kf_id), C.byref(p), ptr(mdl), s, C.byref(cm), ptr(sf), len(sf),
                                                                float(th), float(ratio), int(dist_threshold), ptr(bi), ptr(bd)))
        return bi[:m], bd[:m]

    def fuse_points_into_keyframes_stored(self, store, kf_ids, poses, pts, cam, scale_factors, th, ratio, dist_threshold, out=None):
        """The forward fuse ORBMatcher::fuse(pkf, mapPoints, map, bLoop, th) of ONE list of map points into the stored keyframes kf_ids in
        one call (orbfe_fuse_points_into_keyframes_stored).  poses: [(Rcw, tcw)] per keyframe (or dicts with those keys); pts: dict(usable
        [m], pos [m, 3], view_dir [m, 3], max_dist [m], min_dist [m], desc [m, 32]).  Returns (best_idx [K, m] (-1: none), best_dist [K, m]);
        out = (best_idx, best_dist) supplies the arrays (a call that fails or has nothing to do leaves them as they are)."""
        us = np.ascontiguousarray(pts["usable"], np.uint8).reshape(-1)
        pos = np.ascontiguousarray(pts["pos"], np.float32).reshape(-1, 3)
        vd = np.ascontiguousarray(pts["view_dir"], np.float32).reshape(-1, 3)
        mx, mn = np.ascontiguousarray(pts["max_dist"], np.float32), np.ascontiguousarray(pts["min_dist"], np.float32)
        d = np.ascontiguousarray(pts["desc"], np.uint8).reshape(-1, 32)
        m = len(us)
        if not m == len(pos) == len(vd) == len(mx) == len(mn) == len(d):
            raise ValueError("fuse_points_into_keyframes_stored: the point arrays differ in length")
        ids = np.ascontiguousarray(kf_ids, np.uint64).reshape(-1)
        K = len(ids)
        if len(poses) != K:
            raise ValueError("fuse_points_into_keyframes_stored: one pose per keyframe")
        ps = (FusePose * max(K, 1))()
        for k, pz in enumerate(poses):
            R, t = (pz["Rcw"], pz["tcw"]) if isinstance(pz, dict) else pz
            ps[k].Rcw[:] = np.asarray(R, np.float32).reshape(9).tolist()
            ps[k].tcw[:] = np.asarray(t, np.float32).reshape(3).tolist()
        p = Sim3Points(m, *[ptr(a).value if m else None for a in (us, pos, vd, mx, mn, d)])
        sf = np.ascontiguousarray(scale_factors, np.float32)
        cm = Camera(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), 0.0)
        if out is None:
            out = (np.full((K, m), -1, np.int32), np.zeros((K, m), np.int32))
        bi, bd = out
        if any(x.size < K * m or not x.flags.c_contiguous or x.dtype != np.int32 for x in out):
            raise ValueError("fuse_points_into_keyframes_stored: out must be C-contiguous int32 arrays of at least [K, m]")
        # (kept with the arrays behind them: tools/fuse_points_bench.py times the bare C call with the same arguments)
        self._fuse_points_args = (self.h, store.h, K, ptr(ids) if K else None, C.cast(ps, C.c_void_p), C.byref(p), C.byref(cm), ptr(sf), len(sf),
                                  float(np.float32(th)), float(np.float32(ratio)), int(dist_threshold), ptr(bi) if bi.size else None,
                                  ptr(bd) if bd.size else None)
        self._fuse_points_keep = (us, pos, vd, mx, mn, d, ids, ps, p, sf, cm, bi, bd)
        self._check(self.lib.orbfe_fuse_points_into_keyframes_stored(*self._fuse_points_args))
        return bi, bd

    def fuse_points_kernel_ms(self):
        """(projection, search): device milliseconds of the two kernels of the last fuse_points_into_keyframes_stored made with the MATCH
        stage timed (profile_enable)"""
        ms = np.zeros(2, np.float64)
        self._check(self.lib.orbfe_debug_fuse_points_kernels(ptr(ms)))
        return float(ms[0]), float(ms[1])

    def reloc_refine_stored(self, slot, store, kf_id, good, pos, kf_Rcw, kf_tcw, held, Rcw, tcw, cam, bounds, level_sigma2, level_inv_sigma2,
                            baseline, right_u=None, th_first=10.0, th_second=3.0, ratio=0.9, min_threshold=50, min_inliers=10, enough=50,
                            out=None):
        """What Tracking::trackReLocalize does with one PnP hypothesis (Rcw, tcw) against the stored keyframe kf_id, as one call
        (orbfe_reloc_refine_stored): setCurrFrameAttrib's points (held), OptimizePoseOnly with its post-check, the 10 / 50 decisions, the
        two searchByProjection(frame, keyframe) and the second optimisation.  The frame is the extraction in `slot`; good [n], pos [n, 3]:
        the keyframe's map state; cam = (fx, fy, cx, cy, bf); bounds = (minU, maxU, minV, maxV).
        -> dict(verdict, verdict_name, n_edges [2], n_inliers [2], n_added [2], tlc_z [2], pose_se3 [2, 7], Tcw [2, 12], inlier [2, NF],
        assigned [2, NF], final_assigned [NF], excluded_hits [2, NF], query_accepted [2, n]); out: such a dict to fill (a call that fails
        leaves it as it is)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        good = np.ascontiguousarray(good, np.uint8).reshape(-1)
        pos = f32(pos).reshape(-1, 3)
        n, NF = len(good), self.n_features
        if len(pos) != n:
            raise ValueError("reloc_refine_stored: good and pos differ in length")
        held = np.ascontiguousarray(held, np.int32).reshape(-1)
        right_u = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        if held.size != NF or (right_u is not None and right_u.size != NF):
            raise ValueError("reloc_refine_stored: held / right_u must have n_features entries")
        s2, is2 = f32(level_sigma2), f32(level_inv_sigma2)
        if s2.size < self.n_levels or is2.size < self.n_levels:
            raise ValueError("reloc_refine_stored: one sigma2 / inv_sigma2 per level of the context")
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        ri = RelocInput()
        ri.kf_id, ri.n = int(kf_id), n
        ri.good, ri.pos = (ptr(good).value, ptr(pos).value) if n else (None, None)
        ri.kf_Rcw[:] = f32(kf_Rcw).reshape(9).tolist()
        ri.kf_tcw[:] = f32(kf_tcw).reshape(3).tolist()
        ri.held = ptr(held).value
        ri.right_u = None if right_u is None else ptr(right_u).value
        ri.Rcw[:] = f32(Rcw).reshape(9).tolist()
        ri.tcw[:] = f32(tcw).reshape(3).tolist()
        ri.bounds[:] = f32(bounds).reshape(4).tolist()
        ri.level_sigma2, ri.level_inv_sigma2, ri.cam = ptr(s2).value, ptr(is2).value, C.pointer(cm)
        ri.baseline, ri.th_first, ri.th_second, ri.ratio = float(baseline), float(th_first), float(th_second), float(ratio)
        ri.min_threshold, ri.min_inliers, ri.enough = int(min_threshold), int(min_inliers), int(enough)
        if out is None:
            out = dict(verdict=np.zeros(1, np.int32), n_edges=np.zeros(2, np.int32), n_inliers=np.zeros(2, np.int32), n_added=np.zeros(2, np.int32),
                       tlc_z=np.zeros(2, np.float32), pose_se3=np.zeros((2, 7)), Tcw=np.zeros((2, 12), np.float32), inlier=np.zeros((2, NF), np.uint8),
                       assigned=np.full((2, NF), -1, np.int32), final_assigned=np.full(NF, -1, np.int32),
                       excluded_hits=np.zeros((2, NF), np.int32), query_accepted=np.zeros((2, max(n, 1)), np.uint8))
        ro = RelocOutput(*[ptr(out[k]).value for k, _ in RelocOutput._fields_])
        # (kept with the arrays behind them: tools/reloc_refine_bench.py times the bare C call with the same arguments)
        self._reloc_args = (self.h, int(slot), store.h, C.byref(ri), C.byref(ro))
        self._reloc_keep = (good, pos, held, right_u, s2, is2, cm, ri, ro, out)
        self._check(self.lib.orbfe_reloc_refine_stored(*self._reloc_args))
        res = dict(out)
        res["query_accepted"] = out["query_accepted"].reshape(2, -1)[:, :n] if n else np.zeros((2, 0), np.uint8)
        res["verdict"] = int(out["verdict"][0])
        res["verdict_name"] = RELOC_VERDICTS.get(res["verdict"], "?")
        return res

    def track_reference_stored(self, slot, vocab, store, kf_id, good, pos, Rcw, tcw, cam, bounds, level_sigma2, level_inv_sigma2,
                               frame_good=None, frame_pos=None, right_u=None, feature_vector=None, want_bow=False, levelsup=4, ratio=0.7,
                               dist_threshold=50, check_orientation=True, min_matches=10, min_inliers=10, out=None):
        """Tracking::trackReference against the stored keyframe kf_id as one call (orbfe_track_reference_stored); the parameters and the
        returned dict are described at track_reference_call, which builds the C arguments."""
        args, keep = self.track_reference_call(slot, vocab, store, kf_id, good, pos, Rcw, tcw, cam, bounds, level_sigma2, level_inv_sigma2,
                                               frame_good=frame_good, frame_pos=frame_pos, right_u=right_u, feature_vector=feature_vector,
                                               want_bow=want_bow, levelsup=levelsup, ratio=ratio, dist_threshold=dist_threshold,
                                               check_orientation=check_orientation, min_matches=min_matches, min_inliers=min_inliers, out=out)
        self._check(self.lib.orbfe_track_reference_stored(*args))
        out, bow_arrays = keep[-1], keep[-2]
        res = {k: out[k] for k in ("assigned", "inlier", "final_assigned", "pose_se3", "Tcw")}
        for k in ("verdict", "n_matches", "n_edges", "n_inliers"):
            res[k] = int(out[k][0])
        res["matches"] = out["matches"][:res["n_matches"]].copy()
        res["verdict_name"] = TRACKREF_VERDICTS.get(res["verdict"], "?")
        if want_bow and vocab is not None:
            res["bow"] = _bow_split(bow_arrays, 0)
        return res

    def track_reference_call(self, slot, vocab, store, kf_id, good, pos, Rcw, tcw, cam, bounds, level_sigma2, level_inv_sigma2,
                             frame_good=None, frame_pos=None, right_u=None, feature_vector=None, want_bow=False, levelsup=4, ratio=0.7,
                             dist_threshold=50, check_orientation=True, min_matches=10, min_inliers=10, out=None):
        """The ctypes arguments of orbfe_track_reference_stored for track_reference_stored's parameters -> (args, keep): the bare C call
        is self.lib.orbfe_track_reference_stored(*args); keep holds the arrays behind the pointers (its last entry the output arrays)
        and must live as long as args is used.  Nothing is kept on the context.
        Tracking::trackReference against the stored keyframe kf_id as one call (orbfe_track_reference_stored): computeBow of the
        extraction in `slot` (vocab: a Vocabulary) or the frame's FeatureVector given as feature_vector = (nodes, offsets, features) with
        vocab None, searchByBow with setMapPoints, the 10-match decision, OptimizePoseOnly with its post-check, the 10-inlier decision.
        good [n], pos [n, 3]: the keyframe's map state; frame_good [NF], frame_pos [NF, 3]: the points the frame came with (None: none);
        (Rcw, tcw): the pose the frame has; cam = (fx, fy, cx, cy, bf); bounds = (minU, maxU, minV, maxV).
        -> dict(verdict, verdict_name, n_matches, matches [n_matches] BOW_MATCH_DTYPE, assigned [NF] (TRACKREF_OWN: the point the feature
        came with), n_edges, n_inliers, inlier [NF], final_assigned [NF], pose_se3 [7], Tcw [12]; with want_bow: bow = (words, values, nodes,
        offsets, features) as bow_slots returns them); out: a dict of the raw output arrays to fill (a call that fails leaves it as it is)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        good = np.ascontiguousarray(good, np.uint8).reshape(-1)
        pos = f32(pos).reshape(-1, 3)
        n, NF = len(good), self.n_features
        if len(pos) != n:
            raise ValueError("track_reference_stored: good and pos differ in length")
        right_u = None if right_u is None else np.ascontiguousarray(right_u, np.float64)
        frame_good = None if frame_good is None else np.ascontiguousarray(frame_good, np.uint8).reshape(-1)
        frame_pos = None if frame_pos is None else f32(frame_pos).reshape(-1, 3)
        if (right_u is not None and right_u.size != NF) or (frame_good is not None and (frame_good.size != NF or frame_pos is None or len(frame_pos) != NF)):
            raise ValueError("track_reference_stored: frame_good / frame_pos / right_u must have n_features entries")
        s2, is2 = f32(level_sigma2), f32(level_inv_sigma2)
        if s2.size < self.n_levels or is2.size < self.n_levels:
            raise ValueError("track_reference_stored: one sigma2 / inv_sigma2 per level of the context")
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        ti = TrackRefInput()
        ti.kf_id, ti.n = int(kf_id), n
        ti.good, ti.pos = (ptr(good).value, ptr(pos).value) if n else (None, None)
        if frame_good is not None:
            ti.frame_good, ti.frame_pos = ptr(frame_good).value, ptr(frame_pos).value
        ti.right_u = None if right_u is None else ptr(right_u).value
        ti.Rcw[:] = f32(Rcw).reshape(9).tolist()
        ti.tcw[:] = f32(tcw).reshape(3).tolist()
        ti.bounds[:] = f32(bounds).reshape(4).tolist()
        ti.level_sigma2, ti.level_inv_sigma2, ti.cam = ptr(s2).value, ptr(is2).value, C.pointer(cm)
        ti.levelsup, ti.ratio, ti.dist_threshold = int(levelsup), float(ratio), int(dist_threshold)
        ti.check_orientation, ti.min_matches, ti.min_inliers = int(bool(check_orientation)), int(min_matches), int(min_inliers)
        fv = None
        if feature_vector is not None:
            nodes, offs, feats = feature_vector
            fv = (np.ascontiguousarray(nodes, np.uint32), np.ascontiguousarray(offs, np.int32), np.ascontiguousarray(feats, np.uint32))
            if len(fv[1]) != len(fv[0]) + 1 or (0 <= fv[1][-1] and fv[1][-1] > len(fv[2])):
                raise ValueError("track_reference_stored: node_offsets must have len(nodes) + 1 entries ending inside features")
            ti.n_nodes, ti.nodes, ti.node_offsets, ti.features = len(fv[0]), ptr(fv[0]).value, ptr(fv[1]).value, ptr(fv[2]).value
        if out is None:
            out = dict(verdict=np.zeros(1, np.int32), n_matches=np.zeros(1, np.int32), matches=np.zeros(max(n, 1), BOW_MATCH_DTYPE),
                       assigned=np.full(NF, -1, np.int32), n_edges=np.zeros(1, np.int32), n_inliers=np.zeros(1, np.int32),
                       inlier=np.zeros(NF, np.uint8), final_assigned=np.full(NF, -1, np.int32), pose_se3=np.zeros(7), Tcw=np.zeros(12, np.float32))
        bow_arrays = bo = None
        if want_bow:
            bow_arrays = out.get("bow_arrays") or _bow_arrays(1, NF)
            bo = BowOut(*[ptr(bow_arrays[k]).value for k, _ in BowOut._fields_])
        to = TrackRefOutput(*[ptr(out[k]).value for k, _ in TrackRefOutput._fields_[:-1]], C.addressof(bo) if bo is not None else None)
        args = (self.h, int(slot), None if vocab is None else vocab.h, store.h, C.byref(ti), C.byref(to))
        return args, (good, pos, frame_good, frame_pos, right_u, s2, is2, cm, fv, ti, to, bo, bow_arrays, out)

    def track_motion_model_slots(self, slot, pair, last_slot, last_pair, last_flags, pose, last_pose, cam, bounds, baseline, level_sigma2,
                                 level_inv_sigma2, store=None, last_ids=None, last_pos=None, th=15.0, th_second=30.0, ratio=0.9,
                                 min_threshold=50, min_matches=20, min_inliers=10, out=None):
        """Tracking::trackMotionModel from processLastFrame's unProject to its return as one call (orbfe_track_motion_model_slots); the
        parameters and the returned dict are described at track_motion_slots_call, which builds the C arguments."""
        args, keep = self.track_motion_slots_call(slot, pair, last_slot, last_pair, last_flags, pose, last_pose, cam, bounds, baseline,
                                                  level_sigma2, level_inv_sigma2, store=store, last_ids=last_ids, last_pos=last_pos, th=th,
                                                  th_second=th_second, ratio=ratio, min_threshold=min_threshold, min_matches=min_matches,
                                                  min_inliers=min_inliers, out=out)
        self._check(self.lib.orbfe_track_motion_model_slots(*args))
        out = keep[-1]
        res = {k: out[k] for k in ("assigned", "final_assigned", "inlier", "excluded_hits", "query_matches", "temp", "temp_pos", "pose_se3", "Tcw")}
        for k in ("verdict", "passes", "n_matches", "n_edges", "n_inliers", "n_in_map"):
            res[k] = int(out[k][0])
        res["verdict_name"] = MOTION_VERDICTS.get(res["verdict"], "?")
        return res

    def track_motion_slots_call(self, slot, pair, last_slot, last_pair, last_flags, pose, last_pose, cam, bounds, baseline, level_sigma2,
                                level_inv_sigma2, store=None, last_ids=None, last_pos=None, th=15.0, th_second=30.0, ratio=0.9,
                                min_threshold=50, min_matches=20, min_inliers=10, out=None):
        """The ctypes arguments of orbfe_track_motion_model_slots -> (args, keep): the bare C call is
        self.lib.orbfe_track_motion_model_slots(*args); keep holds the arrays behind the pointers (its last entry the output arrays).
        slot / last_slot: the extraction slots of the current and the last frame's left image; pair / last_pair: the stereo pairs that hold
        the current frame's right_u and the last frame's depth (-1: mono edges / no temporary points).  last_flags [NF]: bit 0 the
        last-frame feature holds a good point, bit 1 that point is in the map; its points by id in a MapPointStore (store, last_ids [NF])
        or by position (last_pos [NF, 3]).  pose = (Rcw, tcw): the predicted pose the frame has; last_pose = (Rcw, tcw, Rwc, twc) of the
        last frame; cam = (fx, fy, cx, cy, bf); bounds = (minU, maxU, minV, maxV); baseline = Camera::mfBl.
        -> dict(verdict, verdict_name, passes, n_matches, n_edges, n_inliers, n_in_map, assigned [NF] (the last-frame feature whose point
        frame feature f holds), final_assigned [NF], inlier [NF], excluded_hits [NF], query_matches [NF], temp [NF], temp_pos [NF, 3],
        pose_se3 [7], Tcw [12]); out: a dict of the raw output arrays to fill (a call that fails leaves it as it is)."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        NF = self.n_features
        last_flags = np.ascontiguousarray(last_flags, np.uint8).reshape(-1)
        last_ids = None if last_ids is None else np.ascontiguousarray(last_ids, np.uint64).reshape(-1)
        last_pos = None if last_pos is None else f32(last_pos).reshape(-1, 3)
        if last_flags.size != NF or (last_ids is not None and last_ids.size != NF) or (last_pos is not None and len(last_pos) != NF):
            raise ValueError("track_motion_model_slots: last_flags / last_ids / last_pos must have n_features entries")
        s2, is2 = f32(level_sigma2), f32(level_inv_sigma2)
        if s2.size < self.n_levels or is2.size < self.n_levels:
            raise ValueError("track_motion_model_slots: one sigma2 / inv_sigma2 per level of the context")
        cm = Camera(*[float(np.float32(v)) for v in cam[:4]], 0, 0, 0, 0, 0, float(np.float32(cam[4])))
        mi = MotionSlotsInput()
        mi.last_flags = ptr(last_flags).value
        mi.last_ids = None if last_ids is None else ptr(last_ids).value
        mi.last_pos = None if last_pos is None else ptr(last_pos).value
        mi.Rcw[:] = f32(pose[0]).reshape(9).tolist()
        mi.tcw[:] = f32(pose[1]).reshape(3).tolist()
        mi.last_Rcw[:] = f32(last_pose[0]).reshape(9).tolist()
        mi.last_tcw[:] = f32(last_pose[1]).reshape(3).tolist()
        mi.last_Rwc[:] = f32(last_pose[2]).reshape(9).tolist()
        mi.last_twc[:] = f32(last_pose[3]).reshape(3).tolist()
        mi.bounds[:] = f32(bounds).reshape(4).tolist()
        mi.cam, mi.baseline = C.pointer(cm), float(np.float32(baseline))
        mi.level_sigma2, mi.level_inv_sigma2 = ptr(s2).value, ptr(is2).value
        mi.th, mi.th_second, mi.ratio = float(th), float(th_second), float(ratio)
        mi.min_threshold, mi.min_matches, mi.min_inliers = int(min_threshold), int(min_matches), int(min_inliers)
        if out is None:
            out = motion_slots_outputs(NF)
        mo = MotionSlotsOutput(*[ptr(out[k]).value for k, _ in MotionSlotsOutput._fields_])
        args = (self.h, int(slot), int(pair), int(last_slot), int(last_pair), None if store is None else store.h, C.byref(mi), C.byref(mo))
        return args, (last_flags, last_ids, last_pos, s2, is2, cm, mi, mo, out)

    # ---- instrumentation ------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """False / 0: off, True / 1: every stage timed alone, 2 + stage id: that stage only, in the production schedule"""
        self._check(self.lib.orbfe_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        ms = np.zeros(STAGE_COUNT, np.float64)
        n = np.zeros(STAGE_COUNT, np.int64)
        self._check(self.lib.orbfe_profile_read(self.h, ptr(ms), ptr(n), int(reset)))
        names = [self.lib.orbfe_stage_name(i).decode() for i in range(STAGE_COUNT)]
        return {names[i]: (float(ms[i]), int(n[i])) for i in range(STAGE_COUNT)}
