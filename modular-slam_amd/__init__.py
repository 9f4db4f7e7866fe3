"""modular-slam_amd — MI355X-native ORB / Hamming-match / BoW front end for modular-slam.

This package is the thin Python harness over the C ABI (include/mslam_hip.h) implemented by
libmslam_hip.so (HIP kernels for gfx950, modular-slam_amd/csrc/).  It mirrors the reference's plugin
interfaces for this path (feature_interface.hpp:50-70, relocalizer.hpp:11-20,
loop_detection.hpp:10-15) with the same names and argument meaning:

    HipOrbDetector.detect(rgb_frame)          ~ IFeatureDetector<RgbFrame,uint8_t,32>::detect
    HipOrbMatcher.match(first, second)        ~ IFeatureMatcher<uint8_t,32>::match
    HipOrbRelocalizer.addKeyframe/relocalize  ~ IRelocalizer<...>
    HipLoopDetector.detectLoop()              ~ ILoopDetector<...>

There is NO CPU fallback: if the shared library is missing, or no HIP device is present, calls
raise.  (The directory name has a hyphen, so import it through `__graft_entry__.load_package()`,
which registers it as module `modular_slam_amd`.)
"""
import contextlib
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmslam_hip.so")

OK, E_INVALID, E_RUNTIME, E_CAPACITY, E_NO_VOCABULARY, E_FORMAT, E_NO_MODEL = range(7)
DBG_PYRAMID, DBG_BLURRED, DBG_CANDIDATES, DBG_SELECTED, DBG_CELLS, DBG_FORMS, DBG_QUAD_DIRECT = range(7)
QUAD_DIRECT_MAX_CANDIDATES = 1024    # k_quadtree_direct: pairs with more candidates run the list passes
MATCHER_AUTO, MATCHER_POPCOUNT = 0, 1
DETECTOR_DISTRIBUTED, DETECTOR_CV_ORB = 0, 1
BOW_ASSIGN_TREE, BOW_ASSIGN_FLAT = 0, 1
CV_ORDER_LIBSTDCXX, CV_ORDER_RASTER = 0, 1
POSE_GRAPH_MAX_KEYFRAMES, POSE_GRAPH_MAX_EDGES = 1024, 65536    # mslam_hip_pose_graph's bounds (include/mslam_hip.h)
POSE_GRAPH_MAX_KEYFRAMES_SPARSE, POSE_GRAPH_MAX_ENVELOPE_BLOCKS = 16384, 1048576    # with the SPARSE solver
PG_SOLVER_DENSE, PG_SOLVER_SPARSE = 0, 1    # mslam_hip_set_pose_graph_solver's kinds
_PG_SOLVER_NAMES = {"dense": PG_SOLVER_DENSE, "sparse": PG_SOLVER_SPARSE}
PG_ORDER_NATURAL, PG_ORDER_RCM = 0, 1    # mslam_hip_pose_graph_analyze's orderings
BA_GLOBAL_MAX_KEYFRAMES, BA_GLOBAL_MAX_KEYFRAMES_SPARSE = 1024, 16384    # mslam_hip_bundle_adjust_global's bounds, DENSE / SPARSE
BA_GLOBAL_SOLVER_DENSE, BA_GLOBAL_SOLVER_SPARSE = 0, 1    # mslam_hip_set_ba_global_solver's kinds
BA_GLOBAL_PCG_MAX_ITERATIONS, BA_GLOBAL_PCG_TOLERANCE = 500, 1e-6    # mslam_hip_set_ba_global_pcg's defaults
POSE_GRAPH_PCG_MAX_ITERATIONS, POSE_GRAPH_PCG_TOLERANCE = 500, 1e-6    # mslam_hip_set_pose_graph_pcg's defaults
CULL_MAX_ENTRIES = 4096   # mslam_hip_kf_observers / _cull_search / _cull: the listed entries of one call
BA_LOSS_NONE, BA_LOSS_HUBER, BA_LOSS_CAUCHY = 0, 1, 2    # mslam_hip_set_ba_loss's kinds
_BA_LOSS_NAMES = {"none": BA_LOSS_NONE, "huber": BA_LOSS_HUBER, "cauchy": BA_LOSS_CAUCHY}
UNION_DESC_RECENT, UNION_DESC_DISTINCTIVE = 0, 1    # mslam_hip_set_union_descriptor's modes
_UNION_DESC_NAMES = {"recent": UNION_DESC_RECENT, "distinctive": UNION_DESC_DISTINCTIVE}
TRACK_POSE_PNP, TRACK_POSE_ALIGN = 0, 1    # mslam_hip_set_track_pose's kinds
_TRACK_POSE_NAMES = {"pnp": TRACK_POSE_PNP, "align": TRACK_POSE_ALIGN}
TSDF_CHUNK, TSDF_MAX_VOXELS, TSDF_MAX_FRAMES = 64, 1 << 30, 32768    # MSLAM_HIP_TSDF_*: (frame, sign) entries per sweep, limits

# every symbol include/mslam_hip.h declares (tests/test_cabi.py checks the .so exports them all)
ABI_SYMBOLS = [
    "mslam_hip_default_params", "mslam_hip_abi_version", "mslam_hip_create", "mslam_hip_destroy",
    "mslam_hip_last_error", "mslam_hip_sync", "mslam_hip_detect", "mslam_hip_detect_batch_dev",
    "mslam_hip_get_batch_view", "mslam_hip_match", "mslam_hip_match_knn2", "mslam_hip_match_batch_dev",
    "mslam_hip_bow_load", "mslam_hip_bow_info", "mslam_hip_bow_words", "mslam_hip_bow_transform",
    "mslam_hip_bow_score", "mslam_hip_bow_db_add", "mslam_hip_bow_db_query", "mslam_hip_bow_db_clear",
    "mslam_hip_bow_batch_dev", "mslam_hip_get_bow_view", "mslam_hip_bow_cross_score_dev", "mslam_hip_level_geometry", "mslam_hip_debug_read",
    "mslam_hip_set_profiling", "mslam_hip_get_stage_times", "mslam_hip_copy_to_host", "mslam_hip_backproject", "mslam_hip_backproject_batch_dev",
    "mslam_hip_get_points_view", "mslam_hip_set_matcher", "mslam_hip_get_matcher",
    "mslam_hip_bow_pack_dev", "mslam_hip_bow_cross_score_packed_dev", "mslam_hip_debug_counts",
    "mslam_hip_last_match_kernel",
    "mslam_hip_join_matcher", "mslam_hip_bow_db_remove", "mslam_hip_bow_set_assignment",
    "mslam_hip_bow_db_reserve", "mslam_hip_bow_db_size", "mslam_hip_qlz_decompress",
    "mslam_hip_pnp_ransac", "mslam_hip_pnp_batch_dev", "mslam_hip_get_pnp_view", "mslam_hip_pnp_set_confidence", "mslam_hip_pack_batch_dev", "mslam_hip_packed_capacity",
    "mslam_hip_set_cv_keypoint_order", "mslam_hip_pnp_min_mse", "mslam_hip_pnp_min_mse_batch_dev",
    "mslam_hip_kf_add", "mslam_hip_kf_add_from_batch_dev", "mslam_hip_kf_remove", "mslam_hip_kf_clear", "mslam_hip_kf_size",
    "mslam_hip_kf_reserve", "mslam_hip_kf_read", "mslam_hip_relocalize",
    "mslam_hip_kf_visible", "mslam_hip_track", "mslam_hip_track_window", "mslam_hip_track_window_dev",
    "mslam_hip_kf_add_ids", "mslam_hip_kf_read_ids", "mslam_hip_kf_covisible", "mslam_hip_kf_union", "mslam_hip_kf_union_dev",
    "mslam_hip_match_guided_knn2", "mslam_hip_match_guided", "mslam_hip_set_guided_match", "mslam_hip_get_guided_match",
    "mslam_hip_bundle_adjust", "mslam_hip_bundle_adjust_global", "mslam_hip_kf_update_world", "mslam_hip_pose_graph",
    "mslam_hip_kf_fuse_search", "mslam_hip_kf_replace_ids", "mslam_hip_kf_fuse",
    "mslam_hip_kf_fuse_search_multi", "mslam_hip_kf_fuse_multi",
    "mslam_hip_kf_remove_observations",
    "mslam_hip_kf_observers", "mslam_hip_kf_cull_search", "mslam_hip_kf_cull",
    "mslam_hip_kf_remove_landmarks", "mslam_hip_kf_cull_landmarks_search", "mslam_hip_kf_cull_landmarks",
    "mslam_hip_set_ba_loss", "mslam_hip_get_ba_loss",
    "mslam_hip_set_union_descriptor", "mslam_hip_get_union_descriptor",
    "mslam_hip_set_pose_graph_solver", "mslam_hip_get_pose_graph_solver", "mslam_hip_pose_graph_analyze",
    "mslam_hip_set_ba_global_solver", "mslam_hip_get_ba_global_solver", "mslam_hip_bundle_adjust_global_analyze",
    "mslam_hip_set_pose_graph_loss", "mslam_hip_get_pose_graph_loss", "mslam_hip_pose_graph_edge_weights",
    "mslam_hip_set_pnp_mse_loss", "mslam_hip_get_pnp_mse_loss",
    "mslam_hip_pose_graph_covariance",
    "mslam_hip_set_ba_global_pcg", "mslam_hip_get_ba_global_pcg", "mslam_hip_get_ba_global_pcg_stats",
    "mslam_hip_set_pose_graph_pcg", "mslam_hip_get_pose_graph_pcg", "mslam_hip_get_pose_graph_pcg_stats",
    "mslam_hip_align_ransac", "mslam_hip_align_batch_dev", "mslam_hip_get_align_view",
    "mslam_hip_set_track_pose", "mslam_hip_get_track_pose",
    "mslam_hip_tsdf_create", "mslam_hip_tsdf_destroy", "mslam_hip_tsdf_info", "mslam_hip_tsdf_add_frame",
    "mslam_hip_tsdf_add_frame_dev", "mslam_hip_tsdf_get_frame", "mslam_hip_tsdf_update_poses", "mslam_hip_tsdf_remove_frame",
    "mslam_hip_tsdf_read", "mslam_hip_tsdf_extract", "mslam_hip_tsdf_raycast", "mslam_hip_tsdf_raycast_dev",
    "mslam_hip_icp_point_plane", "mslam_hip_icp_point_plane_dev", "mslam_hip_icp_linearize", "mslam_hip_tsdf_icp",
    "mslam_hip_tsdf_icp_dev",
]


class MslamHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mslam_hip error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_batch", C.c_int32), ("n_levels", C.c_int32),
                ("scale_factor", C.c_float), ("ini_fast_thr", C.c_int32), ("min_fast_thr", C.c_int32),
                ("min_node_area", C.c_uint32), ("max_keypoints", C.c_int32), ("max_candidates", C.c_int32),
                ("device", C.c_int32), ("stream", C.c_void_p), ("detector", C.c_int32), ("n_features", C.c_int32),
                ("edge_threshold", C.c_int32)]


class BatchView(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("capacity", C.c_int32), ("xy", C.c_void_p), ("desc", C.c_void_p),
                ("octave", C.c_void_p), ("angle", C.c_void_p), ("response", C.c_void_p), ("count", C.c_void_p),
                ("match_from", C.c_void_p), ("match_to", C.c_void_p), ("match_count", C.c_void_p)]


class PointsView(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("xyz", C.c_void_p), ("valid", C.c_void_p)]


class PackedHeader(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("total_keypoints", C.c_int32), ("total_matches", C.c_int32), ("with_points", C.c_int32),
                ("off_kp_offset", C.c_uint64), ("off_match_offset", C.c_uint64), ("off_xy", C.c_uint64), ("off_desc", C.c_uint64),
                ("off_octave", C.c_uint64), ("off_angle", C.c_uint64), ("off_response", C.c_uint64), ("off_xyz", C.c_uint64),
                ("off_valid", C.c_uint64), ("off_match_from", C.c_uint64), ("off_match_to", C.c_uint64), ("bytes", C.c_uint64),
                ("fits", C.c_int32), ("pad", C.c_int32)]


def unpack_batch(buf):
    """numpy views of a buffer written by mslam_hip_pack_batch_dev (buf: 1-D uint8 array holding at least header.bytes)"""
    h = PackedHeader.from_buffer_copy(bytes(buf[:C.sizeof(PackedHeader)]))
    if not h.fits:
        raise MslamHipError(E_CAPACITY, "packed results need %d bytes" % h.bytes)
    nk, nm, nf = h.total_keypoints, h.total_matches, h.n_frames

    def arr(off, dt, n, *shape):
        return np.frombuffer(buf, dt, n, int(off)).reshape((-1,) + shape) if shape else np.frombuffer(buf, dt, n, int(off))
    out = {"n_frames": nf, "bytes": int(h.bytes),
           "kp_offset": arr(h.off_kp_offset, np.int32, nf + 1), "match_offset": arr(h.off_match_offset, np.int32, nf + 1),
           "xy": arr(h.off_xy, np.float32, 2 * nk, 2), "desc": arr(h.off_desc, np.uint8, 32 * nk, 32),
           "octave": arr(h.off_octave, np.int32, nk), "angle": arr(h.off_angle, np.float32, nk),
           "response": arr(h.off_response, np.float32, nk),
           "match_from": arr(h.off_match_from, np.int32, nm), "match_to": arr(h.off_match_to, np.int32, nm)}
    if h.with_points:
        out["xyz"] = arr(h.off_xyz, np.float64, 3 * nk, 3)
        out["valid"] = arr(h.off_valid, np.uint8, nk)
    return out


class PnpView(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("pose", C.c_void_p), ("n_points", C.c_void_p), ("object_points", C.c_void_p),
                ("image_points", C.c_void_p), ("inliers", C.c_void_p)]


class AlignView(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("pose", C.c_void_p), ("n_points", C.c_void_p), ("src_points", C.c_void_p),
                ("dst_points", C.c_void_p), ("inliers", C.c_void_p), ("single_pose", C.c_void_p)]


class TsdfParams(C.Structure):
    """mslam_hip_tsdf_params: the volume (nx, ny, nz voxels of edge `voxel` from the corner `origin`), its truncation and depth
    cut, the number of frames it may retain and its one camera"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("max_frames", C.c_int32), ("voxel", C.c_double),
                ("origin", C.c_double * 3), ("trunc", C.c_double), ("max_depth", C.c_double), ("width", C.c_int32),
                ("height", C.c_int32), ("factor", C.c_float), ("reserved", C.c_int32), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class TsdfRaycastParams(C.Structure):
    """mslam_hip_tsdf_raycast_params: the render camera, the sample range and spacing in metres of camera depth, the coarse
    stride in samples and the observation count a voxel needs"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("z_near", C.c_double), ("z_far", C.c_double), ("step", C.c_double), ("coarse", C.c_int32),
                ("min_weight", C.c_int32)]


class IcpParams(C.Structure):
    """mslam_hip_icp_params: the frame camera, the model camera, the levels (stride, iterations), the gates, min_pairs and the
    step tolerances of frame-to-model alignment"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("factor", C.c_float), ("n_levels", C.c_int32), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("max_depth", C.c_double), ("model_width", C.c_int32),
                ("model_height", C.c_int32), ("mfx", C.c_double), ("mfy", C.c_double), ("mcx", C.c_double), ("mcy", C.c_double),
                ("stride", C.c_int32 * 4), ("iterations", C.c_int32 * 4), ("dist_max", C.c_double), ("cos_min", C.c_double),
                ("min_pairs", C.c_int32), ("reserved", C.c_int32), ("rot_tol", C.c_double), ("trans_tol", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("count", C.c_int32), ("level", C.c_int32),
                ("cost", C.c_double), ("pivots", C.c_double * 6)]


ICP_CONVERGED, ICP_ITERATIONS, ICP_DEGENERATE = range(3)
ICP_LEVELS = ((4, 4), (2, 5), (1, 10))
ICP_DIST_MAX, ICP_COS_MIN, ICP_MIN_PAIRS = 0.1, math.cos(0.6), 64
ICP_RECORD = np.dtype([("level", "<i4"), ("count", "<i4"), ("cost", "<f8"), ("rot2", "<f8"), ("trans2", "<f8")])


class RelocCandidate(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("n_correspondences", C.c_int32), ("n_inliers", C.c_int32), ("status", C.c_int32),
                ("rvec", C.c_double * 3), ("tvec", C.c_double * 3)]


class TrackResult(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("n_correspondences", C.c_int32), ("n_inliers", C.c_int32), ("status", C.c_int32),
                ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("R", C.c_double * 9), ("tracked", C.c_int32),
                ("keyframe_required", C.c_int32), ("keyframe_added", C.c_int32), ("n_entry", C.c_int32),
                ("n_inherited", C.c_int32), ("vote_best", C.c_int32), ("vote_best_count", C.c_int32)]


class BaSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("rejected_steps", C.c_int32),
                ("invalid_steps", C.c_int32), ("n_outliers", C.c_int32), ("reserved", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


class PcgStats(C.Structure):
    _fields_ = [("solves", C.c_int64), ("iterations", C.c_int64), ("longest", C.c_int64), ("at_cap", C.c_int64),
                ("breakdowns", C.c_int64)]


class BowView(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("words", C.c_void_p), ("values", C.c_void_p), ("n_words", C.c_void_p),
                ("best_entry", C.c_void_p), ("best_score", C.c_void_p)]


def build(verbose=False):
    """Compile every HIP source for gfx950 into libmslam_hip.so (in-tree)."""
    subprocess.check_call(["make", "-j8", "-C", _HERE] + ([] if verbose else ["-s"]))


_lib = None


def lib():
    """Load the HIP library.  Fails loudly when it has not been built — there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MslamHipError(E_RUNTIME, "libmslam_hip.so is not built (run __graft_entry__.build()); "
                                           "the product path has no CPU fallback")
        # PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7).  Two HIP runtimes in one
        # process cannot both open the GPU, so when torch is available load it FIRST: our NEEDED
        # libamdhip64.so.7 then binds to the runtime torch already mapped.  Without torch (pure C/C++
        # hosts) the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.mslam_hip_last_error.restype = C.c_char_p
        L.mslam_hip_last_error.argtypes = [C.c_void_p]
        L.mslam_hip_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
        L.mslam_hip_destroy.argtypes = [C.c_void_p]
        L.mslam_hip_destroy.restype = None
        L.mslam_hip_packed_capacity.restype = C.c_size_t
        L.mslam_hip_packed_capacity.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.mslam_hip_pack_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _loss_kind(kind, who):
    """a loss kind given by name ("none" / "huber" / "cauchy") or as BA_LOSS_* -> the number the C ABI takes"""
    if isinstance(kind, str):
        if kind.lower() not in _BA_LOSS_NAMES:
            raise MslamHipError(E_INVALID, "%s: kind %r is not none / huber / cauchy" % (who, kind))
        return _BA_LOSS_NAMES[kind.lower()]
    return int(kind)


def _pg_solver_kind(kind, who):
    if isinstance(kind, str):
        if kind.lower() not in _PG_SOLVER_NAMES:
            raise MslamHipError(E_INVALID, "%s: solver %r is not dense / sparse" % (who, kind))
        return _PG_SOLVER_NAMES[kind.lower()]
    return int(kind)


def _pcg_flag(enable):
    """True / False / 0 / 1 -> 0 / 1; anything else goes to the C ABI as a number it rejects"""
    return int(enable) if isinstance(enable, (bool, int, np.integer)) else -1


def _pcg_int(v):
    """an int32 for the C ABI; what does not fit becomes a number it rejects"""
    return int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 < int(v) < 2 ** 31 else 0


def _pcg_setting(pcg, who, what="global_pcg"):
    """HipBackend's global_pcg / pose_graph_pcg: None, True (the defaults) or (max_iterations, tolerance) -> None or the
    checked pair"""
    if pcg is None or pcg is False:
        return None
    if pcg is True:
        return ((POSE_GRAPH_PCG_MAX_ITERATIONS, POSE_GRAPH_PCG_TOLERANCE) if what == "pose_graph_pcg"
                else (BA_GLOBAL_PCG_MAX_ITERATIONS, BA_GLOBAL_PCG_TOLERANCE))
    try:
        it, tol = pcg
        ok = isinstance(it, (int, np.integer)) and not isinstance(it, bool) and 1 <= int(it) < 2 ** 31 and 0.0 < float(tol) < 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise MslamHipError(E_INVALID, "%s: %s %r is not (max_iterations >= 1, 0 < tolerance < 1)" % (who, what, pcg))
    return int(it), float(tol)


def pose_graph_analyze(fixed, K, edge_a, edge_b):
    """The symbolic phase of Context.pose_graph's SPARSE solver (mslam_hip_pose_graph_analyze): host only, no context, no GPU.
    fixed: [K] flags or None; edges (a, b) as indices below K.  Nodes are the free poses that have an edge.  -> dict(order =
    pose index per position [n_free], first = the least position among a row's neighbours and itself [n_free], n_free,
    ordering = PG_ORDER_NATURAL or PG_ORDER_RCM, envelope_blocks, fits = the envelope is within
    POSE_GRAPH_MAX_ENVELOPE_BLOCKS (the library's E_CAPACITY is fits = False here: the analysis itself is complete)).
    MslamHipError(E_INVALID): K above 16384, more than 65536 edges, an index out of range, an edge from a pose to itself."""
    K = int(K)
    ea = np.ascontiguousarray(edge_a, np.int32).reshape(-1)
    eb = np.ascontiguousarray(edge_b, np.int32).reshape(-1)
    if len(ea) != len(eb):
        raise MslamHipError(E_INVALID, "pose_graph_analyze: %d / %d edge ends" % (len(ea), len(eb)))
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
    if fx is not None and len(fx) != K:
        raise MslamHipError(E_INVALID, "pose_graph_analyze: %d poses, %d fixed flags" % (K, len(fx)))
    order, first = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32)
    n, kind, blocks = C.c_int(0), C.c_int(0), C.c_int64(0)
    rc = lib().mslam_hip_pose_graph_analyze(_p(fx), K, _p(ea), _p(eb), len(ea), _p(order), _p(first), C.byref(n), C.byref(kind),
                                            C.byref(blocks))
    if rc not in (OK, E_CAPACITY):
        raise MslamHipError(rc, "pose_graph_analyze: K outside 0..%d, E outside 0..%d, an index out of range or an edge from a "
                                "pose to itself" % (POSE_GRAPH_MAX_KEYFRAMES_SPARSE, POSE_GRAPH_MAX_EDGES))
    return dict(order=order[:n.value].copy(), first=first[:n.value].copy(), n_free=n.value, ordering=kind.value,
                envelope_blocks=blocks.value, fits=rc == OK)


def ba_global_analyze(fixed, K, obs_kf, obs_lm, L=None):
    """The symbolic phase of Context.bundle_adjust_global's SPARSE solver (mslam_hip_bundle_adjust_global_analyze): host only,
    no context, no GPU.  fixed: [K] flags or None; observations (keyframe index below K, landmark index below L; L defaults
    to one past the largest).  Nodes are the free keyframes that have an observation, adjacent when they share a landmark; a
    node needs no neighbour.  -> dict(order = keyframe index per position [n_free], first [n_free], n_free, ordering =
    PG_ORDER_NATURAL or PG_ORDER_RCM, envelope_blocks, n_pairs = the covisible pairs k1 <= k2 with the diagonal, fits = the
    envelope is within POSE_GRAPH_MAX_ENVELOPE_BLOCKS (the library's E_CAPACITY is fits = False here: the analysis itself is
    complete)).  MslamHipError(E_INVALID): K above 16384, L or M above 2^24, an index out of range."""
    K = int(K)
    ok = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
    ol = np.ascontiguousarray(obs_lm, np.int32).reshape(-1)
    if len(ok) != len(ol):
        raise MslamHipError(E_INVALID, "ba_global_analyze: %d / %d observation ends" % (len(ok), len(ol)))
    L = (int(ol.max()) + 1 if len(ol) else 0) if L is None else int(L)
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
    if fx is not None and len(fx) != K:
        raise MslamHipError(E_INVALID, "ba_global_analyze: %d keyframes, %d fixed flags" % (K, len(fx)))
    order, first = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1), np.int32)
    n, kind, blocks, pairs = C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int(0)
    rc = lib().mslam_hip_bundle_adjust_global_analyze(_p(fx), K, _p(ok), _p(ol), len(ok), L, _p(order), _p(first), C.byref(n),
                                                      C.byref(kind), C.byref(blocks), C.byref(pairs))
    if rc not in (OK, E_CAPACITY):
        raise MslamHipError(rc, "ba_global_analyze: K outside 0..%d, L or M outside 0..2^24 or an index out of range"
                            % BA_GLOBAL_MAX_KEYFRAMES_SPARSE)
    return dict(order=order[:n.value].copy(), first=first[:n.value].copy(), n_free=n.value, ordering=kind.value,
                envelope_blocks=blocks.value, n_pairs=pairs.value, fits=rc == OK)


def default_params(**kw):
    p = Params()
    lib().mslam_hip_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


class Context:
    """Owner of one mslam_hip_ctx (one per GPU / caller thread)."""

    def __init__(self, **kw):
        self.params = default_params(**kw)
        h = C.c_void_p()
        rc = lib().mslam_hip_create(C.byref(self.params), C.byref(h))
        if rc != OK:
            raise MslamHipError(rc, (lib().mslam_hip_last_error(None) or b"").decode())
        self._h = h
        self.L = lib()
        self._lm_cull_capacity = 1024    # rows of kf_cull_landmarks[_search]'s list: grows to what a call reported

    def close(self):
        if getattr(self, "_h", None):
            self.L.mslam_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise MslamHipError(rc, (self.L.mslam_hip_last_error(self._h) or b"").decode())

    # ---- detector ------------------------------------------------------------------------------
    def detect(self, bgr, max_out=None):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        H, W = bgr.shape[:2]
        max_out = max_out or self.params.max_keypoints
        xy = np.empty((max_out, 2), np.float32)
        desc = np.empty((max_out, 32), np.uint8)
        octave = np.empty(max_out, np.int32)
        angle = np.empty(max_out, np.float32)
        resp = np.empty(max_out, np.float32)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_detect(self._h, _p(bgr), W, H, max_out, _p(xy), _p(desc), _p(octave), _p(angle),
                                          _p(resp), C.byref(n)))
        k = n.value
        return dict(xy=xy[:k].copy(), desc=desc[:k].copy(), octave=octave[:k].copy(), angle=angle[:k].copy(),
                    response=resp[:k].copy())

    def detect_batch_dev(self, d_bgr_ptr, n_frames):
        self._chk(self.L.mslam_hip_detect_batch_dev(self._h, C.c_void_p(d_bgr_ptr), int(n_frames)))

    def match_batch_dev(self, ratio=0.7, chain_previous=True):
        self._chk(self.L.mslam_hip_match_batch_dev(self._h, C.c_double(ratio), int(bool(chain_previous))))

    def sync(self):
        self._chk(self.L.mslam_hip_sync(self._h))

    def batch_view(self):
        v = BatchView()
        self._chk(self.L.mslam_hip_get_batch_view(self._h, C.byref(v)))
        return v

    # ---- matcher -------------------------------------------------------------------------------
    def match(self, from_desc, to_desc, ratio=0.7):
        f = np.ascontiguousarray(from_desc, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(to_desc, np.uint8).reshape(-1, 32)
        fi = np.empty(max(len(t), 1), np.int32)
        ti = np.empty(max(len(t), 1), np.int32)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_match(self._h, _p(f), len(f), _p(t), len(t), C.c_double(ratio), _p(fi), _p(ti),
                                         C.byref(n)))
        return fi[:n.value].copy(), ti[:n.value].copy()

    def join_matcher(self):
        self._chk(self.L.mslam_hip_join_matcher(self._h))

    def set_matcher(self, kind):
        """MATCHER_AUTO (matrix cores up to 32736 train rows) or MATCHER_POPCOUNT (xor/popcount always)."""
        self._chk(self.L.mslam_hip_set_matcher(self._h, int(kind)))

    def get_matcher(self):
        return self.L.mslam_hip_get_matcher(self._h)

    def set_cv_keypoint_order(self, order):
        """CV_ORDER_LIBSTDCXX (default: the order of a GCC build of the reference) or CV_ORDER_RASTER (FAST's order)."""
        self._chk(self.L.mslam_hip_set_cv_keypoint_order(self._h, int(order)))

    def last_match_kernel(self):
        """'matrix' / 'popcount' / 'guided': the kernel the last matcher launch took (None before the first)"""
        return {1: "matrix", 2: "popcount", 3: "guided"}.get(self.L.mslam_hip_last_match_kernel(self._h))

    def match_knn2(self, from_desc, to_desc):
        f = np.ascontiguousarray(from_desc, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(to_desc, np.uint8).reshape(-1, 32)
        n = max(len(t), 1)
        out = [np.empty(n, np.int32) for _ in range(4)]
        self._chk(self.L.mslam_hip_match_knn2(self._h, _p(f), len(f), _p(t), len(t), *[_p(o) for o in out]))
        return tuple(o[:len(t)].copy() for o in out)

    # ---- guided matching: landmarks matched in a window round their projection ---------------------
    def _guided_inputs(self, kp_desc, kp_xy, lm_desc, lm_world, R, t):
        kd = np.ascontiguousarray(kp_desc, np.uint8).reshape(-1, 32)
        kx = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        ld = np.ascontiguousarray(lm_desc, np.uint8).reshape(-1, 32)
        lw = np.ascontiguousarray(lm_world, np.float64).reshape(-1, 3)
        if len(kd) != len(kx) or len(ld) != len(lw):
            raise MslamHipError(E_INVALID, "match_guided: descriptors and points do not pair up")
        return kd, kx, ld, lw, np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)

    def match_guided_knn2(self, kp_desc, kp_xy, lm_desc, lm_world, R, t, radius, focal=(525.0, 525.0),
                          principal=(319.5, 239.5), width=640, height=480):
        """per landmark the two keypoints of least Hamming distance among those within `radius` px (square window) of its
        projection under the world -> camera pose (R, t) -> (idx0, idx1, dist0, dist1, n_cand), each [n_lm] int32"""
        kd, kx, ld, lw, R, t = self._guided_inputs(kp_desc, kp_xy, lm_desc, lm_world, R, t)
        out = [np.empty(max(len(ld), 1), np.int32) for _ in range(5)]
        self._chk(self.L.mslam_hip_match_guided_knn2(self._h, _p(kd), _p(kx), len(kd), _p(ld), _p(lw), len(ld), _p(R), _p(t),
                                                     C.c_double(focal[0]), C.c_double(focal[1]), C.c_double(principal[0]),
                                                     C.c_double(principal[1]), int(width), int(height), C.c_double(radius),
                                                     *[_p(o) for o in out]))
        return tuple(o[:len(ld)].copy() for o in out)

    def match_guided(self, kp_desc, kp_xy, lm_desc, lm_world, R, t, radius, max_distance=256, ratio=0.7, focal=(525.0, 525.0),
                     principal=(319.5, 239.5), width=640, height=480):
        """match_guided_knn2 + acceptance (d0 <= max_distance, and the ratio test where a second candidate exists)
        -> (keypoint indices, landmark indices), ordered by landmark"""
        kd, kx, ld, lw, R, t = self._guided_inputs(kp_desc, kp_xy, lm_desc, lm_world, R, t)
        fi = np.empty(max(len(ld), 1), np.int32)
        ti = np.empty(max(len(ld), 1), np.int32)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_match_guided(self._h, _p(kd), _p(kx), len(kd), _p(ld), _p(lw), len(ld), _p(R), _p(t),
                                                C.c_double(focal[0]), C.c_double(focal[1]), C.c_double(principal[0]),
                                                C.c_double(principal[1]), int(width), int(height), C.c_double(radius),
                                                int(max_distance), C.c_double(ratio), _p(fi), _p(ti), C.byref(n)))
        return fi[:n.value].copy(), ti[:n.value].copy()

    def set_guided_match(self, radius, max_distance=256, width=None, height=None):
        """radius > 0: relocalize, track, track_window and track_window_dev match each landmark among the keypoints within
        `radius` px of its projection under the call's guess (calls without a guess keep the brute-force matcher);
        radius <= 0: off (the default).  width, height: the frame extent (default: the context's)."""
        self._chk(self.L.mslam_hip_set_guided_match(self._h, C.c_double(radius), int(max_distance),
                                                    int(self.params.width if width is None else width),
                                                    int(self.params.height if height is None else height)))

    def get_guided_match(self):
        """-> (radius, max_distance, width, height); radius 0 = off"""
        r, d, w, h = C.c_double(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.mslam_hip_get_guided_match(self._h, C.byref(r), C.byref(d), C.byref(w), C.byref(h)))
        return r.value, d.value, w.value, h.value

    def set_union_descriptor(self, mode):
        """Which descriptor a row of kf_union carries.  "recent" (UNION_DESC_RECENT, the default and the reference's rule):
        the most recent observation's.  "distinctive" (UNION_DESC_DISTINCTIVE, an extension after ORB-SLAM's
        ComputeDistinctiveDescriptors): among the landmark's observations in the listed entries, one per entry, the one
        with the least median Hamming distance to all of them; ties go to the largest keyframe id.  Rows, order, world
        points, ids, counts and serials do not depend on the mode."""
        if isinstance(mode, str):
            if mode not in _UNION_DESC_NAMES:
                raise MslamHipError(E_INVALID, "set_union_descriptor: mode %r is not recent / distinctive" % mode)
            mode = _UNION_DESC_NAMES[mode]
        self._chk(self.L.mslam_hip_set_union_descriptor(self._h, int(mode)))

    def get_union_descriptor(self):
        """-> UNION_DESC_RECENT or UNION_DESC_DISTINCTIVE"""
        m = C.c_int(0)
        self._chk(self.L.mslam_hip_get_union_descriptor(self._h, C.byref(m)))
        return m.value

    # ---- RGB-D back-projection (rgbd_feature_frontend.cpp:101-138) ------------------------------
    def backproject(self, depth, xy, factor=1.0 / 5000.0, focal=(525.0, 525.0), principal=(319.5, 239.5)):
        depth = np.ascontiguousarray(depth, np.uint16)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        h, w = depth.shape
        n = len(xy)
        xyz = np.zeros((max(n, 1), 3), np.float64)
        valid = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.mslam_hip_backproject(self._h, _p(depth), w, h, C.c_float(factor), C.c_double(focal[0]),
                                               C.c_double(focal[1]), C.c_double(principal[0]), C.c_double(principal[1]),
                                               _p(xy), n, _p(xyz), _p(valid)))
        return xyz[:n].copy(), valid[:n].astype(bool)

    def backproject_batch_dev(self, d_depth_ptr, factor=1.0 / 5000.0, focal=(525.0, 525.0), principal=(319.5, 239.5)):
        self._chk(self.L.mslam_hip_backproject_batch_dev(self._h, C.c_void_p(d_depth_ptr), C.c_float(factor),
                                                         C.c_double(focal[0]), C.c_double(focal[1]),
                                                         C.c_double(principal[0]), C.c_double(principal[1])))

    def pack_batch_dev(self, out_ptr, capacity_bytes, with_points=True):
        """exactly count[t] keypoint / match_count[t] match records per frame of the last batch, back to back, into out_ptr
        (device memory or page-locked mapped host memory) on the context's stream; parse with unpack_batch()"""
        self._chk(self.L.mslam_hip_pack_batch_dev(self._h, C.c_void_p(out_ptr), C.c_size_t(capacity_bytes), 1 if with_points else 0))

    def packed_capacity(self, n_frames, with_points=True):
        return int(self.L.mslam_hip_packed_capacity(self._h, int(n_frames), 1 if with_points else 0))

    def points_view(self):
        v = PointsView()
        self._chk(self.L.mslam_hip_get_points_view(self._h, C.byref(v)))
        return v

    def pnp_batch_dev(self, focal=(525.0, 525.0), principal=(319.5, 239.5), iterations=100, reprojection_error=5.0, seed=0):
        """one RANSAC PnP per frame of the last batch from its matches + the previous frame's back-projected points
        (after detect_batch_dev, match_batch_dev, backproject_batch_dev); results: pnp_view()"""
        self._chk(self.L.mslam_hip_pnp_batch_dev(self._h, C.c_double(focal[0]), C.c_double(focal[1]), C.c_double(principal[0]),
                                                 C.c_double(principal[1]), int(iterations), C.c_double(reprojection_error),
                                                 C.c_uint64(seed)))

    def pnp_set_confidence(self, confidence):
        """RANSAC confidence of pnp_ransac / pnp_batch_dev (default 0.99, cv_ransac_pnp.cpp:57); outside (0, 1): no early exit"""
        self._chk(self.L.mslam_hip_pnp_set_confidence(self._h, C.c_double(confidence)))

    def pnp_view(self):
        v = PnpView()
        self._chk(self.L.mslam_hip_get_pnp_view(self._h, C.byref(v)))
        return v

    # ---- PnP RANSAC (cv_ransac_pnp.cpp:14-85) ---------------------------------------------------
    def pnp_ransac(self, object_points, image_points, focal=(525.0, 525.0), principal=(319.5, 239.5), rvec=None,
                   tvec=None, iterations=100, reprojection_error=5.0, seed=0):
        """-> (rvec[3], tvec[3], inlier mask[n]) of the world -> camera transform, or None when no model was found
        (cv::solvePnPRansac returning false).  rvec/tvec given = useExtrinsicGuess."""
        obj = np.ascontiguousarray(object_points, np.float32).reshape(-1, 3)
        img = np.ascontiguousarray(image_points, np.float32).reshape(-1, 2)
        guess = rvec is not None and tvec is not None
        r = np.array(rvec if guess else (0, 0, 0), np.float64)
        t = np.array(tvec if guess else (0, 0, 0), np.float64)
        mask = np.zeros(len(obj), np.uint8)
        n_in = C.c_int(0)
        rc = self.L.mslam_hip_pnp_ransac(self._h, _p(obj), _p(img), len(obj), C.c_double(focal[0]), C.c_double(focal[1]),
                                         C.c_double(principal[0]), C.c_double(principal[1]), int(guess), int(iterations),
                                         C.c_double(reprojection_error), C.c_uint64(seed), _p(r), _p(t), _p(mask),
                                         C.byref(n_in))
        if rc == E_NO_MODEL:
            return None
        self._chk(rc)
        return r, t, mask.astype(bool)

    # ---- RANSAC rigid alignment of 3-D points (k_align.hip; no reference counterpart) -------------
    def align_ransac(self, src, dst, max_distance, iterations=100, seed=0, record=False):
        """dst_i ~ R src_i + t -> (rvec[3], tvec[3], inlier mask[n]) of the world -> camera transform, or None when no
        hypothesis reached 4 inliers.  max_distance: the inlier bound on |R src + t - dst|, in the points' unit.
        record=True: a fourth item, the kernel's own record (16 doubles: R row-major, t, inliers, best hypothesis, status, 0)."""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dst, np.float32).reshape(-1, 3)
        if len(s) != len(d):
            raise MslamHipError(E_INVALID, "align_ransac: src and dst differ in length")
        r, t = np.zeros(3, np.float64), np.zeros(3, np.float64)
        mask = np.zeros(len(s), np.uint8)
        n_in = C.c_int(0)
        rc = self.L.mslam_hip_align_ransac(self._h, _p(s), _p(d), len(s), int(iterations), C.c_double(max_distance),
                                           C.c_uint64(seed), _p(r), _p(t), _p(mask), C.byref(n_in))
        if rc == E_NO_MODEL:
            return None
        self._chk(rc)
        if record:
            return r, t, mask.astype(bool), read_device(self, self.align_view().single_pose, (16,), np.float64)
        return r, t, mask.astype(bool)

    def align_batch_dev(self, max_distance, iterations=100, seed=0):
        """one alignment per frame t >= 1 of the last batch from its matches and the back-projected points of both frames
        (after detect_batch_dev, match_batch_dev, backproject_batch_dev); results: align_view()"""
        self._chk(self.L.mslam_hip_align_batch_dev(self._h, int(iterations), C.c_double(max_distance), C.c_uint64(seed)))

    def align_view(self):
        v = AlignView()
        self._chk(self.L.mslam_hip_get_align_view(self._h, C.byref(v)))
        return v

    def set_track_pose(self, kind, max_distance=0.0):
        """the estimator behind track / track_window / track_window_dev: "pnp" (default) or "align" with its inlier bound
        (TRACK_POSE_* are accepted as well); relocalize runs PnP under either"""
        k = _TRACK_POSE_NAMES.get(kind, kind)
        if k not in _TRACK_POSE_NAMES.values():
            raise MslamHipError(E_INVALID, "set_track_pose: %r is not pnp / align" % (kind,))
        self._chk(self.L.mslam_hip_set_track_pose(self._h, int(k), C.c_double(max_distance)))

    def get_track_pose(self):
        """-> (kind, max_distance)"""
        k, d = C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_get_track_pose(self._h, C.byref(k), C.byref(d)))
        return k.value, d.value

    # ---- dense TSDF map that follows the keyframe poses (k_tsdf.hip) ------------------------------
    def tsdf_create(self, dims, voxel, origin, trunc=None, max_depth=3.0, max_frames=1024, width=640, height=480,
                    factor=1.0 / 5000.0, focal=(525.0, 525.0), principal=(319.5, 239.5)):
        """A zeroed volume of dims = (nx, ny, nz) voxels whose voxel (0, 0, 0) has its corner at `origin`; replaces an existing
        volume and drops its frames.  trunc defaults to 4 voxels; max_depth may be inf."""
        p = TsdfParams()
        p.nx, p.ny, p.nz = (int(v) for v in dims)
        p.max_frames = int(max_frames)
        p.voxel = float(voxel)
        p.origin[0], p.origin[1], p.origin[2] = (float(v) for v in origin)
        p.trunc = 4.0 * float(voxel) if trunc is None else float(trunc)
        p.max_depth = float(max_depth)
        p.width, p.height, p.factor = int(width), int(height), float(factor)
        p.fx, p.fy = (float(v) for v in focal)
        p.cx, p.cy = (float(v) for v in principal)
        self._chk(self.L.mslam_hip_tsdf_create(self._h, C.byref(p)))

    def tsdf_destroy(self):
        self._chk(self.L.mslam_hip_tsdf_destroy(self._h))

    def tsdf_info(self):
        """-> (TsdfParams, number of retained frames)"""
        p, n = TsdfParams(), C.c_int(0)
        self._chk(self.L.mslam_hip_tsdf_info(self._h, C.byref(p), C.byref(n)))
        return p, n.value

    @staticmethod
    def _tsdf_pose(R, t, n=1):
        return np.ascontiguousarray(R, np.float64).reshape(n, 9), np.ascontiguousarray(t, np.float64).reshape(n, 3)

    def tsdf_add_frame(self, frame_id, depth, R, t):
        """Integrates a depth image (u16 [height][width]: a host array, or an int device address that is copied) at the world
        -> camera pose (R, t) and retains it under frame_id."""
        R, t = self._tsdf_pose(R, t)
        if isinstance(depth, (int, np.integer)):
            self._chk(self.L.mslam_hip_tsdf_add_frame_dev(self._h, int(frame_id), C.c_void_p(int(depth)), _p(R), _p(t)))
            return
        p, _ = self.tsdf_info()
        d = np.ascontiguousarray(depth, np.uint16)
        if d.shape != (p.height, p.width):
            raise MslamHipError(E_INVALID, "tsdf_add_frame: depth is %r, the volume's camera %d x %d" % (d.shape, p.width, p.height))
        self._chk(self.L.mslam_hip_tsdf_add_frame(self._h, int(frame_id), _p(d), _p(R), _p(t)))

    def tsdf_get_frame(self, frame_id):
        """-> (R[3][3], t[3]): the pose the frame is integrated at"""
        R, t = np.zeros((3, 3), np.float64), np.zeros(3, np.float64)
        self._chk(self.L.mslam_hip_tsdf_get_frame(self._h, int(frame_id), _p(R), _p(t)))
        return R, t

    def tsdf_update_poses(self, frame_ids, R, t):
        """Frames whose pose differs in any bit from the stored one are taken out at the stored pose and put back at the new
        one, all in batched sweeps -> the number of frames moved."""
        ids = np.ascontiguousarray(frame_ids, np.int32).reshape(-1)
        R, t = self._tsdf_pose(R, t, len(ids))
        moved = C.c_int(0)
        self._chk(self.L.mslam_hip_tsdf_update_poses(self._h, _p(ids), _p(R), _p(t), len(ids), C.byref(moved)))
        return moved.value

    def tsdf_remove_frame(self, frame_id):
        self._chk(self.L.mslam_hip_tsdf_remove_frame(self._h, int(frame_id)))

    def tsdf_read(self):
        """-> (S, W), int32 [nz][ny][nx] each (test / debug read-back)"""
        p, _ = self.tsdf_info()
        S, W = np.zeros((p.nz, p.ny, p.nx), np.int32), np.zeros((p.nz, p.ny, p.nx), np.int32)
        self._chk(self.L.mslam_hip_tsdf_read(self._h, _p(S), _p(W)))
        return S, W

    def tsdf_extract(self, min_weight=1, normals=True):
        """-> (xyz f32 [n][3], normal f32 [n][3] or None): the surface points in voxel order, by a count call and a fill"""
        n = C.c_int(0)
        rc = self.L.mslam_hip_tsdf_extract(self._h, int(min_weight), None, None, 0, C.byref(n))
        if rc != E_CAPACITY:
            self._chk(rc)
        xyz = np.zeros((n.value, 3), np.float32)
        nrm = np.zeros((n.value, 3), np.float32) if normals else None
        if n.value:
            self._chk(self.L.mslam_hip_tsdf_extract(self._h, int(min_weight), _p(xyz), _p(nrm), n.value, C.byref(n)))
        return xyz, nrm

    def tsdf_raycast_params(self, R, t, camera=None, z_near=0.1, z_far=None, step=None, coarse=None, min_weight=1):
        """-> TsdfRaycastParams with the defaults of tsdf_raycast filled in"""
        v, _ = self.tsdf_info()
        R, t = self._tsdf_pose(R, t)
        q = TsdfRaycastParams()
        if camera is None:
            camera = dict(width=v.width, height=v.height, focal=(v.fx, v.fy), principal=(v.cx, v.cy))
        q.width, q.height = int(camera["width"]), int(camera["height"])
        q.fx, q.fy = (float(x) for x in camera["focal"])
        q.cx, q.cy = (float(x) for x in camera["principal"])
        if z_far is None:
            z_far = v.max_depth
            if not np.isfinite(z_far):
                ext = np.array([v.nx, v.ny, v.nz], np.float64) * v.voxel
                mid = np.array(list(v.origin), np.float64) + 0.5 * ext
                z_far = float(np.linalg.norm(ext) + np.linalg.norm(-R.reshape(3, 3).T @ t.reshape(3) - mid))
        q.z_near, q.z_far = float(z_near), float(z_far)
        q.step = v.voxel / 2 if step is None else float(step)
        if coarse is None:
            k = np.floor(v.trunc / (2 * q.step)) if q.step > 0 else 1.0    # (a bad step is the library's to refuse)
            coarse = int(k) if np.isfinite(k) and k >= 1 else 1
        q.coarse = min(int(coarse), 0x7fffffff)
        q.min_weight = int(min_weight)
        return q

    def tsdf_raycast(self, R, t, camera=None, z_near=0.1, z_far=None, step=None, coarse=None, min_weight=1, normals=True,
                     out=None, with_hits=False):
        """The view of the volume from the world -> camera pose (R, t) -> (depth f32 [h][w], xyz f32 [h][w][3], normal f32
        [h][w][3] or None); zeros where the ray finds no surface.  camera = dict(width, height, focal, principal) defaults to
        the volume's; z_far to the volume's max_depth (when that is inf: the volume's diagonal plus the distance of the camera
        centre to its middle); step to voxel / 2; coarse to max(1, floor(trunc / (2 step))).  out = (depth, xyz or None,
        normal or None) as int device addresses renders into the caller's device buffers on the context's stream instead and
        returns None (with_hits: the stream is drained and the number of hits returned).  with_hits on the host form
        -> (depth, xyz, normal, n_hits)."""
        q = self.tsdf_raycast_params(R, t, camera, z_near, z_far, step, coarse, min_weight)
        R, t = self._tsdf_pose(R, t)
        n = C.c_int(0)
        hits = C.byref(n) if with_hits else None
        if out is not None:
            d_depth, d_xyz, d_normal = (None if a is None else C.c_void_p(int(a)) for a in out)
            self._chk(self.L.mslam_hip_tsdf_raycast_dev(self._h, C.byref(q), _p(R), _p(t), d_depth, d_xyz, d_normal, hits))
            return n.value if with_hits else None
        if q.width < 1 or q.height < 1 or q.width * q.height > 1 << 30:
            raise MslamHipError(E_INVALID, "tsdf_raycast: width, height must be >= 1 with at most 2^30 pixels")
        depth = np.zeros((q.height, q.width), np.float32)
        xyz = np.zeros((q.height, q.width, 3), np.float32)
        nrm = np.zeros((q.height, q.width, 3), np.float32) if normals else None
        self._chk(self.L.mslam_hip_tsdf_raycast(self._h, C.byref(q), _p(R), _p(t), _p(depth), _p(xyz), _p(nrm), hits))
        return (depth, xyz, nrm, n.value) if with_hits else (depth, xyz, nrm)

    # ---- frame-to-model alignment: point-to-plane ICP (k_icp.hip) ---------------------------------
    @staticmethod
    def icp_params(camera, model_camera=None, levels=ICP_LEVELS, dist_max=ICP_DIST_MAX, cos_min=ICP_COS_MIN,
                   min_pairs=ICP_MIN_PAIRS, rot_tol=0.0, trans_tol=0.0):
        """-> IcpParams.  camera = dict(width, height, focal, principal, factor, max_depth) is the frame's, model_camera =
        dict(width, height, focal, principal) the model's (None: left zero, for tsdf_icp)."""
        q = IcpParams()
        q.width, q.height, q.factor = int(camera["width"]), int(camera["height"]), float(camera["factor"])
        q.fx, q.fy = (float(v) for v in camera["focal"])
        q.cx, q.cy = (float(v) for v in camera["principal"])
        q.max_depth = float(camera["max_depth"])
        if model_camera is not None:
            q.model_width, q.model_height = int(model_camera["width"]), int(model_camera["height"])
            q.mfx, q.mfy = (float(v) for v in model_camera["focal"])
            q.mcx, q.mcy = (float(v) for v in model_camera["principal"])
        levels = [(int(a), int(b)) for a, b in levels]
        q.n_levels = len(levels) if len(levels) <= 4 else 5    # (more than 4 is the library's to refuse)
        for l, (stride, iterations) in enumerate(levels[:4]):
            q.stride[l], q.iterations[l] = stride, iterations
        q.dist_max, q.cos_min, q.min_pairs = float(dist_max), float(cos_min), int(min_pairs)
        q.rot_tol, q.trans_tol = float(rot_tol), float(trans_tol)
        return q

    @staticmethod
    def _icp_out(R, t, res, rec):
        return dict(R=R, t=t, status=res.status, iterations=res.iterations, count=res.count, level=res.level, cost=res.cost,
                    pivots=np.array(list(res.pivots), np.float64), record=rec[:max(res.iterations, 0)], result=res)

    def icp_point_plane(self, depth, camera, model_xyz, model_normal, model_camera, Rm, tm, R0=None, t0=None, **kw):
        """Aligns a depth frame (u16 [h][w] with its camera) to a model given as world-frame xyz and normal images (f32
        [mh][mw][3], a zero normal: no surface) seen through model_camera from the world -> camera pose (Rm, tm), from the
        world -> camera guess (R0, t0) (default: the model's pose) -> dict(R, t, status, iterations, count, level, cost,
        pivots, record, result).  The keywords are icp_params'.  The images are host arrays, or all three int device
        addresses."""
        q = self.icp_params(camera, model_camera, **kw)
        Rm, tm = self._tsdf_pose(Rm, tm)
        R0, t0 = (Rm, tm) if R0 is None else self._tsdf_pose(R0, t0)
        R, t, res = np.zeros((3, 3), np.float64), np.zeros(3, np.float64), IcpResult()
        rec = np.zeros(256, ICP_RECORD)
        if isinstance(depth, (int, np.integer)):
            self._chk(self.L.mslam_hip_icp_point_plane_dev(self._h, C.byref(q), C.c_void_p(int(depth)), C.c_void_p(int(model_xyz)),
                                                           C.c_void_p(int(model_normal)), _p(Rm), _p(tm), _p(R0), _p(t0), _p(R),
                                                           _p(t), C.byref(res), _p(rec), len(rec)))
            return self._icp_out(R, t, res, rec)
        d = np.ascontiguousarray(depth, np.uint16)
        xyz, nrm = np.ascontiguousarray(model_xyz, np.float32), np.ascontiguousarray(model_normal, np.float32)
        if d.shape != (q.height, q.width) or xyz.shape != (q.model_height, q.model_width, 3) or nrm.shape != xyz.shape:
            raise MslamHipError(E_INVALID, "icp_point_plane: depth %r, model %r / %r do not fit the cameras" % (d.shape, xyz.shape, nrm.shape))
        self._chk(self.L.mslam_hip_icp_point_plane(self._h, C.byref(q), _p(d), _p(xyz), _p(nrm), _p(Rm), _p(tm), _p(R0), _p(t0),
                                                   _p(R), _p(t), C.byref(res), _p(rec), len(rec)))
        return self._icp_out(R, t, res, rec)

    def icp_linearize(self, depth, camera, model_xyz, model_normal, model_camera, Rm, tm, R, t, stride=1, **kw):
        """One linearisation at the world -> camera pose (R, t) over the pixels of `stride` -> (A21 f64 [21], g f64 [6], count,
        cost): the upper triangle of J^T J row-major, J^T r, the pairs, sum r r."""
        q = self.icp_params(camera, model_camera, **kw)
        Rm, tm = self._tsdf_pose(Rm, tm)
        R, t = self._tsdf_pose(R, t)
        d = np.ascontiguousarray(depth, np.uint16)
        xyz, nrm = np.ascontiguousarray(model_xyz, np.float32), np.ascontiguousarray(model_normal, np.float32)
        if d.shape != (q.height, q.width) or xyz.shape != (q.model_height, q.model_width, 3) or nrm.shape != xyz.shape:
            raise MslamHipError(E_INVALID, "icp_linearize: depth %r, model %r / %r do not fit the cameras" % (d.shape, xyz.shape, nrm.shape))
        A, g, n, cost = np.zeros(21, np.float64), np.zeros(6, np.float64), C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_icp_linearize(self._h, C.byref(q), _p(d), _p(xyz), _p(nrm), _p(Rm), _p(tm), _p(R), _p(t),
                                                 int(stride), _p(A), _p(g), C.byref(n), C.byref(cost)))
        return A, g, n.value, cost.value

    def tsdf_icp(self, depth, R0, t0, raycast=None, **kw):
        """Renders the volume at the world -> camera guess (R0, t0) (raycast: keywords of tsdf_raycast_params, by default its
        defaults) and aligns the depth frame (u16 [h][w] of the volume's camera: a host array or an int device address) to the
        render -> the dict of icp_point_plane.  The keywords are icp_params'."""
        v, _ = self.tsdf_info()
        rq = self.tsdf_raycast_params(R0, t0, **(raycast or {}))
        q = self.icp_params(dict(width=v.width, height=v.height, focal=(v.fx, v.fy), principal=(v.cx, v.cy), factor=v.factor,
                                 max_depth=v.max_depth), None, **kw)
        R0, t0 = self._tsdf_pose(R0, t0)
        R, t, res = np.zeros((3, 3), np.float64), np.zeros(3, np.float64), IcpResult()
        rec = np.zeros(256, ICP_RECORD)
        if isinstance(depth, (int, np.integer)):
            self._chk(self.L.mslam_hip_tsdf_icp_dev(self._h, C.byref(q), C.byref(rq), C.c_void_p(int(depth)), _p(R0), _p(t0), _p(R),
                                                    _p(t), C.byref(res), _p(rec), len(rec)))
            return self._icp_out(R, t, res, rec)
        d = np.ascontiguousarray(depth, np.uint16)
        if d.shape != (v.height, v.width):
            raise MslamHipError(E_INVALID, "tsdf_icp: depth is %r, the volume's camera %d x %d" % (d.shape, v.width, v.height))
        self._chk(self.L.mslam_hip_tsdf_icp(self._h, C.byref(q), C.byref(rq), _p(d), _p(R0), _p(t0), _p(R), _p(t), C.byref(res),
                                            _p(rec), len(rec)))
        return self._icp_out(R, t, res, rec)

    # ---- min-MSE PnP (MinMseTracker, ceres_reprojection_error_pnp.cpp:18-110) --------------------
    def pnp_min_mse(self, object_points, image_points, focal=(525.0, 525.0), principal=(319.5, 239.5), rvec=(0, 0, 0),
                    tvec=(0, 0, 0)):
        """Levenberg-Marquardt on the reprojection error of every point, from (rvec, tvec) (angle-axis, translation)
        -> (rvec, tvec, termination, iterations, final cost); termination 0 CONVERGENCE, 1 NO_CONVERGENCE.
        Raises MslamHipError(E_NO_MODEL) when the minimiser ends in FAILURE (Summary::IsSolutionUsable() == false)."""
        obj = np.ascontiguousarray(object_points, np.float64).reshape(-1, 3)
        img = np.ascontiguousarray(image_points, np.float64).reshape(-1, 2)
        if len(obj) != len(img):
            raise MslamHipError(E_INVALID, "pnp_min_mse: %d object points, %d image points" % (len(obj), len(img)))
        r = np.array(rvec, np.float64).reshape(3)
        t = np.array(tvec, np.float64).reshape(3)
        term, iters, cost = C.c_int(-1), C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_pnp_min_mse(self._h, _p(obj), _p(img), len(obj), C.c_double(focal[0]), C.c_double(focal[1]),
                                               C.c_double(principal[0]), C.c_double(principal[1]), _p(r), _p(t),
                                               C.byref(term), C.byref(iters), C.byref(cost)))
        return r, t, term.value, iters.value, cost.value

    def set_pnp_mse_loss(self, kind, scale=0.0):
        """the loss function of pnp_min_mse and pnp_min_mse_batch_dev from now on (an extension: the reference's call has
        none, so every mismatch pulls the pose with full weight): kind "none" (the default state) / "huber" / "cauchy" or
        BA_LOSS_*; scale a in pixels, finite and > 0 for huber and cauchy, ignored for none.  s = |observed - projected|^2
        per point; the formulas are set_ba_loss's.  The costs become 1/2 sum rho.  Nothing else reads the setting."""
        self._chk(self.L.mslam_hip_set_pnp_mse_loss(self._h, _loss_kind(kind, "set_pnp_mse_loss"), C.c_double(scale)))

    def get_pnp_mse_loss(self):
        """-> (kind as BA_LOSS_*, scale); (BA_LOSS_NONE, 0.0) when no loss is set"""
        k, s = C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_get_pnp_mse_loss(self._h, C.byref(k), C.byref(s)))
        return k.value, s.value

    def pnp_min_mse_batch_dev(self, d_object, d_image, d_n, n_problems, capacity, d_pose, d_info, focal=(525.0, 525.0),
                              principal=(319.5, 239.5)):
        """one min-MSE PnP per problem on device data (raw device pointers), asynchronous on the context's stream:
        object f64[n_problems][capacity][3], image f64[n_problems][capacity][2], n i32[n_problems],
        pose f64[n_problems][6] (r, t) in / out, info f64[n_problems][4] = termination, iterations, initial cost, final cost"""
        self._chk(self.L.mslam_hip_pnp_min_mse_batch_dev(self._h, C.c_void_p(d_object), C.c_void_p(d_image), C.c_void_p(d_n),
                                                         int(n_problems), int(capacity), C.c_double(focal[0]),
                                                         C.c_double(focal[1]), C.c_double(principal[0]),
                                                         C.c_double(principal[1]), C.c_void_p(d_pose), C.c_void_p(d_info)))

    # ---- keyframe store + verified relocalisation (rgbd_feature_frontend.cpp:402-431, :495-534) ----
    def kf_add(self, id, desc, world_xyz, lids=None):
        """store keyframe `id`: n landmarks = descriptors (n x 32) + world points (n x 3 f64); an existing id is replaced.
        lids = None: the landmarks get fresh landmark ids; otherwise n caller-chosen ids in [0, 2^62) (mslam_hip_kf_add_ids)"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        w = np.ascontiguousarray(world_xyz, np.float64).reshape(-1, 3)
        if len(d) != len(w):
            raise MslamHipError(E_INVALID, "kf_add: %d descriptors, %d world points" % (len(d), len(w)))
        if lids is None:
            self._chk(self.L.mslam_hip_kf_add(self._h, int(id), _p(d), _p(w), len(d)))
            return
        l = np.ascontiguousarray(lids, np.int64).reshape(-1)
        if len(l) != len(d):
            raise MslamHipError(E_INVALID, "kf_add: %d descriptors, %d landmark ids" % (len(d), len(l)))
        self._chk(self.L.mslam_hip_kf_add_ids(self._h, int(id), _p(d), _p(w), _p(l), len(d)))

    def kf_add_from_batch_dev(self, id, frame, R=np.eye(3), t=(0, 0, 0), z_max=3.0):
        """store frame `frame` of the last detect + back-project batch as keyframe `id` (valid depth, z <= z_max,
        world = R p + t); asynchronous on the context's stream"""
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        self._chk(self.L.mslam_hip_kf_add_from_batch_dev(self._h, int(id), int(frame), _p(R), _p(t), C.c_double(z_max)))

    def kf_remove(self, id):
        self._chk(self.L.mslam_hip_kf_remove(self._h, int(id)))

    def kf_clear(self):
        self._chk(self.L.mslam_hip_kf_clear(self._h))

    def kf_reserve(self, max_entries):
        self._chk(self.L.mslam_hip_kf_reserve(self._h, int(max_entries)))

    def kf_size(self):
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_size(self._h, C.byref(n)))
        return n.value

    def kf_read(self, id):
        """-> (desc [n, 32] u8, world_xyz [n, 3] f64) of a stored keyframe (debug read-back; synchronises)"""
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_read(self._h, int(id), None, None, 0, C.byref(n)))
        d = np.empty((max(n.value, 1), 32), np.uint8)
        w = np.empty((max(n.value, 1), 3), np.float64)
        self._chk(self.L.mslam_hip_kf_read(self._h, int(id), _p(d), _p(w), n.value, C.byref(n)))
        return d[:n.value].copy(), w[:n.value].copy()

    def kf_read_ids(self, id):
        """-> landmark ids [n] i64 of a stored keyframe (debug read-back; synchronises)"""
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_read_ids(self._h, int(id), None, 0, C.byref(n)))
        l = np.empty(max(n.value, 1), np.int64)
        self._chk(self.L.mslam_hip_kf_read_ids(self._h, int(id), _p(l), n.value, C.byref(n)))
        return l[:n.value].copy()

    # ---- bundle adjustment (ceres_backend.cpp:185-240) ----------------------------------------------
    def bundle_adjust(self, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed=None, max_iterations=100, outlier_threshold=0.15):
        """CeresBackend::bundleAdjustment's solve: poses [K, 7] (qx qy qz qw px py pz, camera -> world, K <= 64), landmarks
        [L, 3], observations (keyframe index, landmark index, camera-frame point [M, 3]); fixed = [K] flags or None.
        -> dict(poses, landmarks, outlier [M] bool, termination, iterations, rejected_steps, invalid_steps, n_outliers,
        initial_cost, final_cost).  termination 2 (FAILURE) is a result here (MSLAM_HIP_E_NO_MODEL): poses and landmarks
        come back unchanged."""
        return self._bundle_adjust(self.L.mslam_hip_bundle_adjust, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed,
                                   max_iterations, outlier_threshold)

    def bundle_adjust_global(self, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed=None, max_iterations=100, outlier_threshold=0.15):
        """CeresBackend::globalBundleAdjustment's solve: bundle_adjust's arguments and result with K <= 1024, always through
        the blocked solver (covisible-pair Schur complement, blocked Cholesky over many workgroups), at any K.  After
        set_ba_global_solver("sparse"): K <= 16384, the reduced system on its block envelope (E_CAPACITY when the envelope
        is above POSE_GRAPH_MAX_ENVELOPE_BLOCKS: nothing touched).  After set_ba_global_pcg(): K <= 16384, the reduced
        system by preconditioned conjugate gradients on its non-zero blocks, whatever set_ba_global_solver says."""
        return self._bundle_adjust(self.L.mslam_hip_bundle_adjust_global, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed,
                                   max_iterations, outlier_threshold)

    def set_ba_global_solver(self, kind):
        """the linear solver of bundle_adjust_global from now on: "dense" (the default state: the blocked Cholesky of the dense
        reduced camera system, K <= 1024) / "sparse" (a Cholesky factor on the block envelope of the covisibility graph after a
        NATURAL or reverse Cuthill-McKee order, K <= 16384, an envelope of at most POSE_GRAPH_MAX_ENVELOPE_BLOCKS blocks, else
        E_CAPACITY) or BA_GLOBAL_SOLVER_*.  bundle_adjust and pose_graph do not read the setting."""
        self._chk(self.L.mslam_hip_set_ba_global_solver(self._h, _pg_solver_kind(kind, "set_ba_global_solver")))

    def get_ba_global_solver(self):
        """-> BA_GLOBAL_SOLVER_DENSE or BA_GLOBAL_SOLVER_SPARSE"""
        k = C.c_int(0)
        self._chk(self.L.mslam_hip_get_ba_global_solver(self._h, C.byref(k)))
        return k.value

    def set_ba_global_pcg(self, enable=True, max_iterations=BA_GLOBAL_PCG_MAX_ITERATIONS, tolerance=BA_GLOBAL_PCG_TOLERANCE):
        """bundle_adjust_global solves its reduced camera system by block-Jacobi preconditioned conjugate gradients from now
        on (enable = False: by set_ba_global_solver's kind again, which this setting never changes): K <= 16384 and at most
        POSE_GRAPH_MAX_ENVELOPE_BLOCKS non-zero blocks (ba_global_analyze's n_pairs), else E_CAPACITY.  CG ends at |r| <=
        tolerance |b| or after max_iterations, whose iterate is taken.  For maps that revisit their ground; thin rings stay
        "sparse"'s.  bundle_adjust and pose_graph do not read the setting."""
        self._chk(self.L.mslam_hip_set_ba_global_pcg(self._h, _pcg_flag(enable), _pcg_int(max_iterations), C.c_double(float(tolerance))))

    def get_ba_global_pcg(self):
        """-> (enabled, max_iterations, tolerance)"""
        e, m, t = C.c_int(0), C.c_int(0), C.c_double(0.0)
        self._chk(self.L.mslam_hip_get_ba_global_pcg(self._h, C.byref(e), C.byref(m), C.byref(t)))
        return bool(e.value), m.value, t.value

    def ba_global_pcg_stats(self):
        """the linear solves of the last bundle_adjust_global -> dict(solves, iterations (CG, in total), longest (CG
        iterations of one solve), at_cap (solves that ended at max_iterations), breakdowns); zeros without PCG"""
        st = PcgStats()
        self._chk(self.L.mslam_hip_get_ba_global_pcg_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in PcgStats._fields_}

    def ba_global_analyze(self, fixed, K, obs_kf, obs_lm, L=None):
        """the module's ba_global_analyze: the symbolic phase bundle_adjust_global would run with "sparse" (no GPU work)"""
        return ba_global_analyze(fixed, K, obs_kf, obs_lm, L)

    def set_ba_loss(self, kind, scale=0.0):
        """the loss function of bundle_adjust and bundle_adjust_global from now on (an extension: the reference has none):
        kind "none" (the default state) / "huber" / "cauchy" or BA_LOSS_*; scale a in metres, finite and > 0 for huber and
        cauchy, ignored for none.  s = |r_m|^2 per observation, b = a^2: huber rho = s for s <= b, else 2 a sqrt(s) - b;
        cauchy rho = b log(1 + s / b).  The costs a solve reports become 1/2 sum rho; the outlier mask is still judged on
        the plain residual.  pose_graph and pnp_min_mse do not read the setting: set_pose_graph_loss and set_pnp_mse_loss
        are theirs."""
        self._chk(self.L.mslam_hip_set_ba_loss(self._h, _loss_kind(kind, "set_ba_loss"), C.c_double(scale)))

    def get_ba_loss(self):
        """-> (kind as BA_LOSS_*, scale); (BA_LOSS_NONE, 0.0) when no loss is set"""
        k, s = C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_get_ba_loss(self._h, C.byref(k), C.byref(s)))
        return k.value, s.value

    def _bundle_adjust(self, entry, poses, landmarks, obs_kf, obs_lm, obs_cam, fixed, max_iterations, outlier_threshold):
        x = np.array(poses, np.float64, order="C").reshape(-1, 7)        # a copy in row-major order, whatever the argument's
        lm = np.array(landmarks, np.float64, order="C").reshape(-1, 3)
        ok = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
        ol = np.ascontiguousarray(obs_lm, np.int32).reshape(-1)
        oc = np.ascontiguousarray(obs_cam, np.float64).reshape(-1, 3)
        if not len(ok) == len(ol) == len(oc):
            raise MslamHipError(E_INVALID, "bundle_adjust: %d / %d / %d observations" % (len(ok), len(ol), len(oc)))
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
        if fx is not None and len(fx) != len(x):
            raise MslamHipError(E_INVALID, "bundle_adjust: %d poses, %d fixed flags" % (len(x), len(fx)))
        mask = np.zeros(max(len(ok), 1), np.uint8)
        out = BaSummary()
        rc = entry(self._h, _p(x), _p(fx), len(x), _p(lm), len(lm), _p(ok), _p(ol), _p(oc), len(ok), int(max_iterations),
                   C.c_double(outlier_threshold), _p(mask), C.byref(out))
        if rc != E_NO_MODEL:
            self._chk(rc)
        res = {k: getattr(out, k) for k, _ in BaSummary._fields_ if k != "reserved"}
        res.update(poses=x, landmarks=lm, outlier=mask[:len(ok)].astype(bool))
        return res

    def set_pose_graph_solver(self, kind):
        """the linear solver of pose_graph from now on: "dense" (the default state: the blocked Cholesky of the dense normal
        equations, K <= 1024) / "sparse" (a Cholesky factor on the block envelope after a NATURAL or reverse Cuthill-McKee
        order, K <= 16384, an envelope of at most POSE_GRAPH_MAX_ENVELOPE_BLOCKS blocks, else E_CAPACITY) or PG_SOLVER_*.
        Nothing else reads the setting."""
        self._chk(self.L.mslam_hip_set_pose_graph_solver(self._h, _pg_solver_kind(kind, "set_pose_graph_solver")))

    def get_pose_graph_solver(self):
        """-> PG_SOLVER_DENSE or PG_SOLVER_SPARSE"""
        k = C.c_int(0)
        self._chk(self.L.mslam_hip_get_pose_graph_solver(self._h, C.byref(k)))
        return k.value

    def set_pose_graph_pcg(self, enable=True, max_iterations=POSE_GRAPH_PCG_MAX_ITERATIONS, tolerance=POSE_GRAPH_PCG_TOLERANCE):
        """pose_graph solves its damped normal equations by block-Jacobi preconditioned conjugate gradients from now on
        (enable = False: by set_pose_graph_solver's kind again, which this setting never changes): K <= 16384, the non-zero
        blocks alone, no order and no envelope.  CG ends at |r| <= tolerance |b| or after max_iterations, whose iterate is
        taken.  For graphs that revisit their ground; CG needs about nine iterations per pose of a thin chain, so thin chains
        stay "sparse"'s.  A setting of its own: pose_graph_covariance, pose_graph_edge_weights and the bundle adjustments do
        not read it, and set_ba_global_pcg does not touch it."""
        self._chk(self.L.mslam_hip_set_pose_graph_pcg(self._h, _pcg_flag(enable), _pcg_int(max_iterations), C.c_double(float(tolerance))))

    def get_pose_graph_pcg(self):
        """-> (enabled, max_iterations, tolerance)"""
        e, m, t = C.c_int(0), C.c_int(0), C.c_double(0.0)
        self._chk(self.L.mslam_hip_get_pose_graph_pcg(self._h, C.byref(e), C.byref(m), C.byref(t)))
        return bool(e.value), m.value, t.value

    def pose_graph_pcg_stats(self):
        """the linear solves of the last pose_graph -> dict(solves, iterations (CG, in total), longest (CG iterations of one
        solve), at_cap (solves that ended at max_iterations), breakdowns); zeros without PCG or without a system"""
        st = PcgStats()
        self._chk(self.L.mslam_hip_get_pose_graph_pcg_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in PcgStats._fields_}

    def set_pose_graph_loss(self, kind, scale=0.0):
        """the loss function of pose_graph from now on, with either linear solver (an extension): kind "none" (the default
        state) / "huber" / "cauchy" or BA_LOSS_*; scale a in the unit of the weighted residual, finite and > 0 for huber and
        cauchy, ignored for none.  s = |r_e|^2 per edge over all six components after sqrt_info; the formulas are
        set_ba_loss's.  The costs a solve reports become 1/2 sum rho.  pose_graph_edge_weights reads it too; the bundle
        adjustments and pnp_min_mse do not."""
        self._chk(self.L.mslam_hip_set_pose_graph_loss(self._h, _loss_kind(kind, "set_pose_graph_loss"), C.c_double(scale)))

    def get_pose_graph_loss(self):
        """-> (kind as BA_LOSS_*, scale); (BA_LOSS_NONE, 0.0) when no loss is set"""
        k, s = C.c_int(0), C.c_double(0)
        self._chk(self.L.mslam_hip_get_pose_graph_loss(self._h, C.byref(k), C.byref(s)))
        return k.value, s.value

    def _pose_graph_edges(self, who, edge_a, edge_b, edge_meas, sqrt_info):
        ea = np.ascontiguousarray(edge_a, np.int32).reshape(-1)
        eb = np.ascontiguousarray(edge_b, np.int32).reshape(-1)
        z = np.ascontiguousarray(edge_meas, np.float64).reshape(-1, 7)
        w = None if sqrt_info is None else np.ascontiguousarray(sqrt_info, np.float64).reshape(-1, 36)
        if not len(ea) == len(eb) == len(z) or (w is not None and len(w) != len(ea)):
            raise MslamHipError(E_INVALID, "%s: %d / %d edge ends, %d measurements, %s sqrt_info" % (
                who, len(ea), len(eb), len(z), "no" if w is None else len(w)))
        return ea, eb, z, w

    def pose_graph_edge_weights(self, poses, edge_a, edge_b, edge_meas, sqrt_info=None):
        """what the pose-graph loss makes of every edge at the given poses (pose_graph's arguments; K <= 16384 whichever
        solver is set) -> (chi2 [E], weight [E]): chi2 = |r_e|^2 and weight = rho'(chi2) under set_pose_graph_loss, 1.0
        without a loss.  At a solve's result it shows which edges the solve down-weighted."""
        x = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        ea, eb, z, w = self._pose_graph_edges("pose_graph_edge_weights", edge_a, edge_b, edge_meas, sqrt_info)
        chi2, weight = np.zeros(max(len(ea), 1)), np.zeros(max(len(ea), 1))
        self._chk(self.L.mslam_hip_pose_graph_edge_weights(self._h, _p(x), len(x), _p(ea), _p(eb), _p(z), _p(w), len(ea),
                                                           _p(chi2), _p(weight)))
        return chi2[:len(ea)], weight[:len(ea)]

    def pose_graph(self, poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, max_iterations=100):
        """The pose-graph solve behind closeLoop: poses [K, 7] (qx qy qz qw px py pz, camera -> world, K <= 1024, or 16384
        after set_pose_graph_solver("sparse") or set_pose_graph_pcg()), E edges
        (a, b) with edge_meas [E, 7] = q then p of pose b in a's frame, sqrt_info [E, 6, 6] or None for identity, fixed = [K]
        flags or None.  -> dict(poses, termination, iterations, rejected_steps, invalid_steps, n_outliers = 0, initial_cost,
        final_cost).  termination 2 (FAILURE) is a result here (MSLAM_HIP_E_NO_MODEL): the poses come back unchanged.
        After set_pose_graph_loss the cost is 1/2 sum rho(|r_e|^2) and both costs report that."""
        x = np.array(poses, np.float64, order="C").reshape(-1, 7)        # a copy in row-major order, whatever the argument's
        ea, eb, z, w = self._pose_graph_edges("pose_graph", edge_a, edge_b, edge_meas, sqrt_info)
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
        if fx is not None and len(fx) != len(x):
            raise MslamHipError(E_INVALID, "pose_graph: %d poses, %d fixed flags" % (len(x), len(fx)))
        out = BaSummary()
        rc = self.L.mslam_hip_pose_graph(self._h, _p(x), _p(fx), len(x), _p(ea), _p(eb), _p(z), _p(w), len(ea),
                                         int(max_iterations), C.byref(out))
        if rc != E_NO_MODEL:
            self._chk(rc)
        res = {k: getattr(out, k) for k, _ in BaSummary._fields_ if k != "reserved"}
        res.update(poses=x)
        return res

    def pose_graph_covariance(self, poses, edge_a, edge_b, edge_meas, sqrt_info=None, fixed=None, poses_of=(), pairs=()):
        """Marginal covariances of pose_graph's problem at `poses` (mslam_hip_pose_graph_covariance; pose_graph's arguments,
        K <= 16384 whichever solver is set): blocks of (J^T J)^-1 over the free poses that have an edge, on the solver's
        tangent (delta, dp) per pose (delta is half a rotation vector in the world frame), under set_pose_graph_loss.
        poses_of: pose indices; pairs: (a, b) index pairs, each joined by an edge unless one of the two is constant.
        -> dict(cov [P, 6, 6], cross [Q, 6, 6]): cov[p] the block of poses_of[p], cross[q] = E[d_a d_b^T] with rows from a.  A
        constant pose gives zeros.  MslamHipError: E_INVALID for a free pose without an edge, a pair a == b or a pair no
        edge joins; E_NO_MODEL for a rank-deficient problem (a component without an edge to a constant pose, a pivot that
        is not > 0); E_CAPACITY for an envelope above POSE_GRAPH_MAX_ENVELOPE_BLOCKS.  Nothing is returned then."""
        x = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        ea, eb, z, w = self._pose_graph_edges("pose_graph_covariance", edge_a, edge_b, edge_meas, sqrt_info)
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
        if fx is not None and len(fx) != len(x):
            raise MslamHipError(E_INVALID, "pose_graph_covariance: %d poses, %d fixed flags" % (len(x), len(fx)))
        idx = np.ascontiguousarray(poses_of, np.int32).reshape(-1)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        cov, cross = np.zeros((max(len(idx), 1), 6, 6)), np.zeros((max(len(pr), 1), 6, 6))
        self._chk(self.L.mslam_hip_pose_graph_covariance(self._h, _p(x), _p(fx), len(x), _p(ea), _p(eb), _p(z), _p(w), len(ea),
                                                         _p(idx), len(idx), _p(cov), _p(pa), _p(pb), len(pr), _p(cross)))
        return dict(cov=cov[:len(idx)], cross=cross[:len(pr)])

    def kf_update_world(self, landmark_ids, world_xyz):
        """every landmark of every stored keyframe whose landmark id is listed takes the listed world point -> the number
        of store landmarks written"""
        l = np.ascontiguousarray(landmark_ids, np.int64).reshape(-1)
        w = np.ascontiguousarray(world_xyz, np.float64).reshape(-1, 3)
        if len(l) != len(w):
            raise MslamHipError(E_INVALID, "kf_update_world: %d ids, %d points" % (len(l), len(w)))
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_update_world(self._h, _p(l), _p(w), len(l), C.byref(n)))
        return n.value

    # ---- landmark fusion (an extension: the reference's closeLoop is empty) ------------------------
    def _fuse_pairs(self, entry, head, names, R, t, radius, max_distance, ratio, max_world_distance, focal, principal, width, height,
                    capacity, tail):
        """a fusion call: `head` = the C arguments that name the entries, `names` = its pair arrays in the C argument order
        (the *_lid are i64, the others i32), each of `capacity` rows (default: max_keypoints, which holds every result: a
        call has at most one pair per keep landmark) -> dict of the arrays cut to the count; E_CAPACITY raises carrying
        `needed`, the count"""
        cap = int(self.params.max_keypoints if capacity is None else capacity)
        cols = {k: np.zeros(max(cap, 1), np.int64 if k.endswith("_lid") else np.int32) for k in names}
        n = C.c_int(0)
        rc = entry(self._h, *head, _p(R), _p(t), C.c_double(focal[0]), C.c_double(focal[1]), C.c_double(principal[0]),
                   C.c_double(principal[1]), int(self.params.width if width is None else width),
                   int(self.params.height if height is None else height), C.c_double(radius), int(max_distance), C.c_double(ratio),
                   C.c_double(max_world_distance), *(_p(v) for v in cols.values()), cap, C.byref(n), *tail)
        if rc == E_CAPACITY:
            e = MslamHipError(rc, (self.L.mslam_hip_last_error(self._h) or b"").decode())
            e.needed = n.value
            raise e
        self._chk(rc)
        return {k: v[:n.value].copy() for k, v in cols.items()}

    def _fuse_call(self, entry, keep_id, drop_id, R, t, *rest):
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        return self._fuse_pairs(entry, (int(keep_id), int(drop_id)), ("keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist"), R, t, *rest)

    def kf_fuse_search(self, keep_id, drop_id, R, t, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf,
                       focal=(525.0, 525.0), principal=(319.5, 239.5), width=None, height=None, capacity=None):
        """the landmarks of entry drop_id that duplicate landmarks of entry keep_id: both projected under the world -> camera
        pose (R, t), each keep landmark matched among the drop landmarks within `radius` px and max_world_distance metres,
        one to one -> dict(keep_pos, drop_pos, keep_lid, drop_lid, dist), ordered by keep position.  Changes nothing.
        More pairs than `capacity` (default: max_keypoints): MslamHipError E_CAPACITY carrying `needed`."""
        return self._fuse_call(self.L.mslam_hip_kf_fuse_search, keep_id, drop_id, R, t, radius, max_distance, ratio,
                               max_world_distance, focal, principal, width, height, capacity, ())

    def kf_replace_ids(self, from_ids, to_ids, world_xyz=None):
        """every landmark of every stored keyframe whose id is from_ids[p] takes the id to_ids[p] and, when given, the world
        point world_xyz[p]; simultaneous, the later of a repeated `from` wins -> the number of store landmarks that matched"""
        f = np.ascontiguousarray(from_ids, np.int64).reshape(-1)
        t = np.ascontiguousarray(to_ids, np.int64).reshape(-1)
        w = None if world_xyz is None else np.ascontiguousarray(world_xyz, np.float64).reshape(-1, 3)
        if len(f) != len(t) or (w is not None and len(w) != len(f)):
            raise MslamHipError(E_INVALID, "kf_replace_ids: %d from ids, %d to ids, %s points" % (len(f), len(t), "no" if w is None else len(w)))
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_replace_ids(self._h, _p(f), _p(t), _p(w), len(f), C.byref(n)))
        return n.value

    def kf_fuse(self, keep_id, drop_id, R, t, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf, focal=(525.0, 525.0),
                principal=(319.5, 239.5), width=None, height=None, capacity=None):
        """kf_fuse_search, then every store landmark with a pair's drop id takes the keep id and the keep landmark's world
        point, in one call with one synchronisation -> kf_fuse_search's dict plus n_rewritten"""
        nr = C.c_int(0)
        out = self._fuse_call(self.L.mslam_hip_kf_fuse, keep_id, drop_id, R, t, radius, max_distance, ratio,
                              max_world_distance, focal, principal, width, height, capacity, (C.byref(nr),))
        out["n_rewritten"] = nr.value
        return out

    # ---- landmark fusion into many target entries (SearchAndFuse's loop over the connected keyframes, one call) ----
    def _fuse_multi_call(self, entry, keep_id, drop_ids, R, t, *rest):
        ids = np.ascontiguousarray(drop_ids, np.int32).reshape(-1)
        R = np.ascontiguousarray(R, np.float64).reshape(-1)
        t = np.ascontiguousarray(t, np.float64).reshape(-1)
        if len(R) != 9 * len(ids) or len(t) != 3 * len(ids):
            raise MslamHipError(E_INVALID, "kf_fuse_multi: %d drop ids, %d R values, %d t values" % (len(ids), len(R), len(t)))
        return self._fuse_pairs(entry, (int(keep_id), _p(ids), len(ids)), ("target", "keep_pos", "drop_pos", "keep_lid", "drop_lid", "dist"),
                                R, t, *rest)

    def kf_fuse_search_multi(self, keep_id, drop_ids, R, t, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf,
                             focal=(525.0, 525.0), principal=(319.5, 239.5), width=None, height=None, capacity=None):
        """the landmarks of the entries drop_ids (1..64, distinct) that duplicate landmarks of entry keep_id: kf_fuse_search
        per target m under its own world -> camera pose (R[m], t[m]), with eligibility taken over all listed entries, then
        one row per drop id (the least (dist, target, keep_pos)) and one per keep id (the least (dist, target, drop_pos))
        -> dict(target, keep_pos, drop_pos, keep_lid, drop_lid, dist), ordered by (target, keep_pos).  Changes nothing.
        More pairs than a given `capacity`: MslamHipError E_CAPACITY carrying `needed`."""
        return self._fuse_multi_call(self.L.mslam_hip_kf_fuse_search_multi, keep_id, drop_ids, R, t, radius, max_distance, ratio,
                                     max_world_distance, focal, principal, width, height, capacity, ())

    def kf_fuse_multi(self, keep_id, drop_ids, R, t, radius, max_distance=50, ratio=0.7, max_world_distance=np.inf,
                      focal=(525.0, 525.0), principal=(319.5, 239.5), width=None, height=None, capacity=None):
        """kf_fuse_search_multi, then every store landmark with a pair's drop id takes the keep id and the keep landmark's
        world point, in one call with one synchronisation -> kf_fuse_search_multi's dict plus n_rewritten"""
        nr = C.c_int(0)
        out = self._fuse_multi_call(self.L.mslam_hip_kf_fuse_multi, keep_id, drop_ids, R, t, radius, max_distance, ratio,
                                    max_world_distance, focal, principal, width, height, capacity, (C.byref(nr),))
        out["n_rewritten"] = nr.value
        return out

    # ---- removeObservation (rgbd_feature_frontend.cpp:469-487, commented out in the reference) ----
    def kf_remove_observations(self, kf_ids, landmark_ids):
        """row p removes landmark landmark_ids[p] from store entry kf_ids[p], every position that holds it; the survivors
        keep their order and the entry's count drops -> dict(removed = [n] i32: the positions row p's landmark held before
        the call, n_removed = the store positions removed, each counted once)"""
        k = np.ascontiguousarray(kf_ids, np.int32).reshape(-1)
        l = np.ascontiguousarray(landmark_ids, np.int64).reshape(-1)
        if len(k) != len(l):
            raise MslamHipError(E_INVALID, "kf_remove_observations: %d keyframe ids, %d landmark ids" % (len(k), len(l)))
        removed = np.zeros(max(len(k), 1), np.int32)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_kf_remove_observations(self._h, _p(k), _p(l), len(k), _p(removed), C.byref(n)))
        return dict(removed=removed[:len(k)].copy(), n_removed=n.value)

    # ---- keyframe culling (an extension: the reference has removeKeyframe and no policy that calls it) ----
    def kf_observers(self, ids, landmark_ids):
        """-> counts [n] i32: how many of the listed store entries `ids` (1..4096, distinct) hold each landmark id at one
        position at least; 0 for an id none of them holds"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        l = np.ascontiguousarray(landmark_ids, np.int64).reshape(-1)
        counts = np.zeros(max(len(l), 1), np.int32)
        self._chk(self.L.mslam_hip_kf_observers(self._h, _p(ids), len(ids), _p(l), len(l), _p(counts)))
        return counts[:len(l)].copy()

    def _cull_call(self, entry, ids, cand, min_observers, ratio, min_landmarks):
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        cand = np.ascontiguousarray(cand, np.int32).reshape(-1)
        m = max(len(cand), 1)
        culled, nl, nr, n = np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros(m, np.int32), C.c_int(0)
        self._chk(entry(self._h, _p(ids), len(ids), _p(cand), len(cand), int(min_observers), C.c_double(ratio), int(min_landmarks),
                        _p(culled), _p(nl), _p(nr), C.byref(n)))
        k = len(cand)
        return dict(culled=culled[:k].astype(bool), n_landmarks=nl[:k].copy(), n_redundant=nr[:k].copy(), n_culled=n.value)

    def kf_cull_search(self, ids, cand, min_observers=3, ratio=0.9, min_landmarks=1):
        """the greedy culling pass over the candidates `cand` (distinct, each one of the listed entries `ids`), in the order
        given: a candidate goes when it has at least min_landmarks distinct landmark ids and more than `ratio` of them are
        held by at least min_observers other listed entries, counted without the candidates culled before it
        -> dict(culled [n_cand] bool, n_landmarks, n_redundant [n_cand] i32, n_culled).  Changes nothing."""
        return self._cull_call(self.L.mslam_hip_kf_cull_search, ids, cand, min_observers, ratio, min_landmarks)

    def kf_cull(self, ids, cand, min_observers=3, ratio=0.9, min_landmarks=1):
        """kf_cull_search, then the culled entries leave the store as kf_remove would remove them -> the same dict"""
        return self._cull_call(self.L.mslam_hip_kf_cull, ids, cand, min_observers, ratio, min_landmarks)

    # ---- landmark culling (an extension: the reference has no such step; the model is ORB-SLAM's MapPointCulling) ----
    def kf_remove_landmarks(self, ids, landmark_ids):
        """every position of every listed store entry `ids` (1..4096, distinct) whose landmark id is listed is removed;
        the survivors keep their order and the entries' counts drop; entries that are not listed are untouched
        -> dict(removed = [n] i32: the store positions that held landmark_ids[p], entry_removed = [n_ids] i32: the
        positions entry ids[k] lost, n_removed = their sum)"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        l = np.ascontiguousarray(landmark_ids, np.int64).reshape(-1)
        removed, lost, n = np.zeros(max(len(l), 1), np.int32), np.zeros(max(len(ids), 1), np.int32), C.c_int(0)
        self._chk(self.L.mslam_hip_kf_remove_landmarks(self._h, _p(ids), len(ids), _p(l), len(l), _p(removed), _p(lost), C.byref(n)))
        return dict(removed=removed[:len(l)].copy(), entry_removed=lost[:len(ids)].copy(), n_removed=n.value)

    def _lm_cull_call(self, entry, ids, cand, min_observers, tail):
        """the search or the fused call with the wrapper's growing list capacity: on E_CAPACITY nothing has changed, so the
        call is repeated once with the count it reported"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        cand = np.ascontiguousarray(cand, np.int32).reshape(-1)
        for attempt in range(2):
            cap = self._lm_cull_capacity
            l, o, n = np.zeros(cap, np.int64), np.zeros(cap, np.int32), C.c_int(0)
            rc = entry(self._h, _p(ids), len(ids), _p(cand), len(cand), int(min_observers), _p(l), _p(o), cap, C.byref(n), *tail)
            if rc != E_CAPACITY or attempt or n.value <= cap:
                break
            self._lm_cull_capacity = n.value
        self._chk(rc)
        return dict(landmark_ids=l[:n.value].copy(), observers=o[:n.value].copy())

    def kf_cull_landmarks_search(self, ids, cand, min_observers=2):
        """the landmark ids that at least one candidate entry `cand` (distinct, each one of the listed entries `ids`) holds
        and that fewer than min_observers listed entries hold -> dict(landmark_ids [n] i64, ascending, observers [n] i32).
        Changes nothing."""
        return self._lm_cull_call(self.L.mslam_hip_kf_cull_landmarks_search, ids, cand, min_observers, ())

    def kf_cull_landmarks(self, ids, cand, min_observers=2):
        """kf_cull_landmarks_search, then the found landmarks leave every listed entry as kf_remove_landmarks removes them,
        in one call with one synchronisation -> the search's dict plus entry_removed [n_ids] i32 and n_removed"""
        lost, nr = np.zeros(max(np.size(ids), 1), np.int32), C.c_int(0)
        out = self._lm_cull_call(self.L.mslam_hip_kf_cull_landmarks, ids, cand, min_observers, (_p(lost), C.byref(nr)))
        out.update(entry_removed=lost[:np.size(ids)].copy(), n_removed=nr.value)
        return out

    # ---- the local map (basic_map.cpp:141-237, rgbd_feature_frontend.cpp:57-80, :256-277) ---------
    def kf_covisible(self, id, ids):
        """-> counts [len(ids)]: how many distinct landmark ids of entry `id` each entry of ids (<= 64) holds as well"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        counts = np.zeros(max(len(ids), 1), np.int32)
        self._chk(self.L.mslam_hip_kf_covisible(self._h, int(id), _p(ids), len(ids), _p(counts)))
        return counts[:len(ids)].copy()

    def kf_union(self, dst_id, ids, sync=True):
        """entry dst_id = one landmark per distinct landmark id of the listed entries (1..64), each the observation of the
        listed entry with the largest id, ordered by list position, then landmark position.
        sync=True -> the number of landmarks (MslamHipError E_CAPACITY carries `needed` when they exceed max_keypoints);
        sync=False enqueues only -> None, and an overflow surfaces at the next sync()"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if not sync:
            self._chk(self.L.mslam_hip_kf_union_dev(self._h, int(dst_id), _p(ids), len(ids)))
            return None
        n = C.c_int(0)
        rc = self.L.mslam_hip_kf_union(self._h, int(dst_id), _p(ids), len(ids), C.byref(n))
        if rc == E_CAPACITY:
            e = MslamHipError(rc, (self.L.mslam_hip_last_error(self._h) or b"").decode())
            e.needed = n.value
            raise e
        self._chk(rc)
        return n.value

    def relocalize(self, desc, xy, cand_ids, focal=(525.0, 525.0), principal=(319.5, 239.5), valid=None, ratio=0.7,
                   iterations=100, reprojection_error=5.0, seed=0, rvec=None, tvec=None, min_inliers=60, with_pairs=False):
        """one query frame (desc [n, 32], xy [n, 2], optional valid [n]) against the stored keyframes cand_ids (<= 64):
        per candidate match -> correspondences -> RANSAC PnP (seed + position), then the ranking.
        -> dict(best = position in cand_ids or -1, candidates = [dict(n_matches, n_correspondences, n_inliers, status,
        rvec, tvec)], and with with_pairs also pairs = [(from, to)] and inliers = [mask over the correspondences]).
        best = -1 is a result here (MSLAM_HIP_E_NO_MODEL), not an exception."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        p2 = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        if len(d) != len(p2):
            raise MslamHipError(E_INVALID, "relocalize: %d descriptors, %d points" % (len(d), len(p2)))
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(-1)
        if v is not None and len(v) != len(d):
            raise MslamHipError(E_INVALID, "relocalize: valid mask of the wrong length")
        ids = np.ascontiguousarray(cand_ids, np.int32).reshape(-1)
        P = len(ids)
        guess = rvec is not None and tvec is not None
        r = np.array(rvec if guess else (0, 0, 0), np.float64)
        t = np.array(tvec if guess else (0, 0, 0), np.float64)
        out = (RelocCandidate * max(P, 1))()
        best = C.c_int(-1)
        stride = self.params.max_keypoints if with_pairs else 0
        pf = np.zeros((max(P, 1), stride), np.int32) if with_pairs else None
        pt = np.zeros((max(P, 1), stride), np.int32) if with_pairs else None
        inl = np.zeros((max(P, 1), stride), np.uint8) if with_pairs else None
        rc = self.L.mslam_hip_relocalize(self._h, _p(d), _p(p2), _p(v), len(d), _p(ids), P, C.c_double(focal[0]),
                                         C.c_double(focal[1]), C.c_double(principal[0]), C.c_double(principal[1]),
                                         C.c_double(ratio), int(iterations), C.c_double(reprojection_error), C.c_uint64(seed),
                                         int(guess), _p(r), _p(t), int(min_inliers), out, C.byref(best), _p(pf), _p(pt),
                                         _p(inl), int(stride))
        if rc != E_NO_MODEL:
            self._chk(rc)
        cands = [dict(n_matches=o.n_matches, n_correspondences=o.n_correspondences, n_inliers=o.n_inliers, status=o.status,
                      rvec=np.array(o.rvec[:]), tvec=np.array(o.tvec[:])) for o in out[:P]]
        res = dict(best=best.value, candidates=cands)
        if with_pairs:
            res["pairs"] = [(pf[k, :c["n_matches"]].copy(), pt[k, :c["n_matches"]].copy()) for k, c in enumerate(cands)]
            res["inliers"] = [inl[k, :c["n_correspondences"]].astype(bool) for k, c in enumerate(cands)]
        return res

    # ---- the keyframe tracking step (rgbd_feature_frontend.cpp:279-400, :544-575) -----------------
    def kf_visible(self, ids, R, t, focal=(525.0, 525.0), principal=(319.5, 239.5), width=640, height=480):
        """findBetterReferenceKeyframe's count: per stored keyframe of ids (<= 64) the landmarks that project into a
        width x height frame seen from the world -> camera pose (R, t) -> (counts [len(ids)], best = position of the first
        maximum, -1 for an empty list)"""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        counts = np.zeros(max(len(ids), 1), np.int32)
        best = C.c_int(-1)
        self._chk(self.L.mslam_hip_kf_visible(self._h, _p(ids), len(ids), _p(R), _p(t), C.c_double(focal[0]), C.c_double(focal[1]),
                                              C.c_double(principal[0]), C.c_double(principal[1]), int(width), int(height),
                                              _p(counts), C.byref(best)))
        return counts[:len(ids)].copy(), best.value

    def track(self, desc, xy, depth, ref_id, vote_ids=(), new_id=-1, factor=1.0 / 5000.0, focal=(525.0, 525.0),
              principal=(319.5, 239.5), ratio=0.7, iterations=100, reprojection_error=5.0, seed=0, rvec=None, tvec=None,
              min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, with_pairs=False, with_entry=False,
              pair_stride=None, entry_capacity=None):
        """RgbdFeatureFrontend::track against the stored keyframe ref_id in one call: depth filter, match, PnP (guess =
        rvec, tvec), the reference vote over vote_ids, and — when a keyframe is required and new_id >= 0 — the new entry.
        -> dict of mslam_hip_track_result's fields (R as [3, 3]) plus vote_counts, and with with_pairs pairs = (from, to)
        and inliers, with with_entry entry_src / entry_kp.  tracked = 0 is a result here (MSLAM_HIP_E_NO_MODEL)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        p2 = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        if len(d) != len(p2):
            raise MslamHipError(E_INVALID, "track: %d descriptors, %d points" % (len(d), len(p2)))
        depth = np.ascontiguousarray(depth, np.uint16)
        h, w = depth.shape
        ids = np.ascontiguousarray(vote_ids, np.int32).reshape(-1)
        guess = rvec is not None and tvec is not None
        r = np.array(rvec if guess else (0, 0, 0), np.float64)
        t = np.array(tvec if guess else (0, 0, 0), np.float64)
        K = self.params.max_keypoints
        stride = (K if pair_stride is None else int(pair_stride)) if with_pairs else 0
        cap = (K if entry_capacity is None else int(entry_capacity)) if with_entry else 0
        pf = np.zeros(max(stride, 1), np.int32) if with_pairs else None
        pt = np.zeros(max(stride, 1), np.int32) if with_pairs else None
        inl = np.zeros(max(stride, 1), np.uint8) if with_pairs else None
        es = np.zeros(max(cap, 1), np.int32) if with_entry else None
        ek = np.zeros(max(cap, 1), np.int32) if with_entry else None
        counts = np.zeros(max(len(ids), 1), np.int32)
        out = TrackResult()
        rc = self.L.mslam_hip_track(self._h, _p(d), _p(p2), len(d), _p(depth), w, h, C.c_float(factor), C.c_double(focal[0]),
                                    C.c_double(focal[1]), C.c_double(principal[0]), C.c_double(principal[1]), int(ref_id),
                                    _p(ids), len(ids), C.c_double(ratio), int(iterations), C.c_double(reprojection_error),
                                    C.c_uint64(seed), int(guess), _p(r), _p(t), int(min_matched_points),
                                    int(new_keyframe_min_landmarks), int(new_id), C.c_double(z_max), C.byref(out), _p(counts),
                                    _p(pf), _p(pt), _p(inl), int(stride), _p(es), _p(ek), int(cap))
        if rc != E_NO_MODEL:
            self._chk(rc)
        res = {k: getattr(out, k) for k, _ in TrackResult._fields_ if k not in ("rvec", "tvec", "R")}
        res.update(rvec=np.array(out.rvec[:]), tvec=np.array(out.tvec[:]), R=np.array(out.R[:]).reshape(3, 3),
                   vote_counts=counts[:len(ids)].copy())
        if with_pairs:
            res["pairs"] = (pf[:out.n_matches].copy(), pt[:out.n_matches].copy())
            res["inliers"] = inl[:out.n_correspondences].astype(bool)
        if with_entry:
            res["entry_src"], res["entry_kp"] = es[:out.n_entry].copy(), ek[:out.n_entry].copy()
        return res

    # ---- the tracking step on a window of frames (between two events of the loop the frames are independent) ----
    def _window_records(self, out, counts, S, n_vote, first, es, ek):
        recs = []
        for s in range(S):
            o = out[s]
            r = {k: getattr(o, k) for k, _ in TrackResult._fields_ if k not in ("rvec", "tvec", "R")}
            r.update(rvec=np.array(o.rvec[:]), tvec=np.array(o.tvec[:]), R=np.array(o.R[:]).reshape(3, 3),
                     vote_counts=counts[s, :n_vote].copy())
            if es is not None:
                k = o.n_entry if s == first else 0
                r["entry_src"], r["entry_kp"] = es[:k].copy(), ek[:k].copy()
            recs.append(r)
        return recs

    def track_window(self, descs, xys, depths, ref_id, vote_ids=(), new_id=-1, ref_vote_pos=-1, factor=1.0 / 5000.0,
                     focal=(525.0, 525.0), principal=(319.5, 239.5), ratio=0.7, iterations=100, reprojection_error=5.0, seed=0,
                     rvec=None, tvec=None, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, with_entry=False,
                     entry_capacity=None, stride=None, pad_value=0):
        """Context.track for S = len(descs) frames (1..256) against the one stored keyframe ref_id in one call: descs[s]
        [n_s, 32], xys[s] [n_s, 2], depths[s] [h, w] u16 (one size).  Frame s gets the seed `seed + s`; all frames share the
        guess (rvec, tvec).  ref_vote_pos = the position of the current reference keyframe in vote_ids (-1: a vote never is
        an event).  stride (default: the largest n_s) and pad_value shape the padded arrays the C call takes.
        -> (records, first_event): per frame the dict Context.track returns (without pairs), as computed against ref_id;
        first_event = the first frame that is not tracked, requires a keyframe or votes for another keyframe, or S.  With
        new_id >= 0 a keyframe the frame first_event requires is built in the store (keyframe_added, n_entry, n_inherited
        and, with with_entry, entry_src / entry_kp on that record).  Frame 0 not tracked is a result here, not an exception."""
        S = len(descs)
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descs]
        ps = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in xys]
        if len(ps) != S or len(depths) != S or any(len(d) != len(p) for d, p in zip(ds, ps)):
            raise MslamHipError(E_INVALID, "track_window: descriptors, points and depth frames do not pair up")
        n = np.array([len(d) for d in ds], np.int32)
        st = int(n.max() if S else 0) if stride is None else int(stride)
        if S and st < n.max():
            raise MslamHipError(E_INVALID, "track_window: stride is smaller than a frame's keypoint count")
        d = np.full((max(S, 1), max(st, 1), 32), pad_value, np.uint8)
        p2 = np.full((max(S, 1), max(st, 1), 2), pad_value, np.float32)
        for s in range(S):
            d[s, :n[s]], p2[s, :n[s]] = ds[s], ps[s]
        depth = np.ascontiguousarray(np.stack([np.asarray(x, np.uint16) for x in depths]) if S else np.zeros((1, 1, 1)), np.uint16)
        h, w = depth.shape[1:]
        ids = np.ascontiguousarray(vote_ids, np.int32).reshape(-1)
        guess = rvec is not None and tvec is not None
        r = np.array(rvec if guess else (0, 0, 0), np.float64)
        t = np.array(tvec if guess else (0, 0, 0), np.float64)
        K = self.params.max_keypoints
        cap = (K if entry_capacity is None else int(entry_capacity)) if with_entry else 0
        es = np.zeros(max(cap, 1), np.int32) if with_entry else None
        ek = np.zeros(max(cap, 1), np.int32) if with_entry else None
        counts = np.zeros((max(S, 1), max(len(ids), 1)), np.int32)
        out = (TrackResult * max(S, 1))()
        first = C.c_int(0)
        rc = self.L.mslam_hip_track_window(self._h, _p(d), _p(p2), _p(n), st, _p(depth), S, w, h, C.c_float(factor),
                                           C.c_double(focal[0]), C.c_double(focal[1]), C.c_double(principal[0]),
                                           C.c_double(principal[1]), int(ref_id), _p(ids), len(ids), int(ref_vote_pos),
                                           C.c_double(ratio), int(iterations), C.c_double(reprojection_error), C.c_uint64(seed),
                                           int(guess), _p(r), _p(t), int(min_matched_points), int(new_keyframe_min_landmarks),
                                           int(new_id), C.c_double(z_max), out, C.byref(first), _p(counts), _p(es), _p(ek),
                                           int(cap))
        if rc != E_NO_MODEL:
            self._chk(rc)
        return self._window_records(out, counts, S, len(ids), first.value, es, ek), first.value

    def track_window_dev(self, first_frame, n_frames, ref_id, vote_ids=(), new_id=-1, ref_vote_pos=-1, focal=(525.0, 525.0),
                         principal=(319.5, 239.5), ratio=0.7, iterations=100, reprojection_error=5.0, seed=0, rvec=None,
                         tvec=None, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0, with_entry=False,
                         entry_capacity=None):
        """track_window on frames first_frame .. first_frame + n_frames - 1 of the last detect_batch_dev +
        backproject_batch_dev batch: nothing is uploaded but the vote list -> (records, first_event)"""
        S = int(n_frames)
        ids = np.ascontiguousarray(vote_ids, np.int32).reshape(-1)
        guess = rvec is not None and tvec is not None
        r = np.array(rvec if guess else (0, 0, 0), np.float64)
        t = np.array(tvec if guess else (0, 0, 0), np.float64)
        K = self.params.max_keypoints
        cap = (K if entry_capacity is None else int(entry_capacity)) if with_entry else 0
        es = np.zeros(max(cap, 1), np.int32) if with_entry else None
        ek = np.zeros(max(cap, 1), np.int32) if with_entry else None
        counts = np.zeros((max(S, 1), max(len(ids), 1)), np.int32)
        out = (TrackResult * max(S, 1))()
        first = C.c_int(0)
        rc = self.L.mslam_hip_track_window_dev(self._h, int(first_frame), S, C.c_double(focal[0]), C.c_double(focal[1]),
                                               C.c_double(principal[0]), C.c_double(principal[1]), int(ref_id), _p(ids),
                                               len(ids), int(ref_vote_pos), C.c_double(ratio), int(iterations),
                                               C.c_double(reprojection_error), C.c_uint64(seed), int(guess), _p(r), _p(t),
                                               int(min_matched_points), int(new_keyframe_min_landmarks), int(new_id),
                                               C.c_double(z_max), out, C.byref(first), _p(counts), _p(es), _p(ek), int(cap))
        if rc != E_NO_MODEL:
            self._chk(rc)
        S = S if 1 <= S <= 256 else 0
        return self._window_records(out, counts, S, len(ids), first.value, es, ek), first.value

    # ---- bag of words --------------------------------------------------------------------------
    def bow_load(self, blob):
        b = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob)
        self._chk(self.L.mslam_hip_bow_load(self._h, _p(b), C.c_size_t(b.size)))

    def bow_info(self):
        v = [C.c_int() for _ in range(6)]
        self._chk(self.L.mslam_hip_bow_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("k", "L", "n_nodes", "n_words", "scoring", "weighting"), [x.value for x in v]))

    def bow_set_assignment(self, mode):
        """BOW_ASSIGN_TREE (DBoW3's descent) or BOW_ASSIGN_FLAT (exhaustive search over all words)"""
        self._chk(self.L.mslam_hip_bow_set_assignment(self._h, int(mode)))

    def bow_words(self, desc):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        w = np.empty(max(len(d), 1), np.uint32)
        wt = np.empty(max(len(d), 1), np.float64)
        self._chk(self.L.mslam_hip_bow_words(self._h, _p(d), len(d), _p(w), _p(wt)))
        return w[:len(d)].copy(), wt[:len(d)].copy()

    def bow_transform(self, desc):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        w = np.empty(max(len(d), 1), np.uint32)
        v = np.empty(max(len(d), 1), np.float64)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_bow_transform(self._h, _p(d), len(d), _p(w), _p(v), C.byref(n)))
        return w[:n.value].copy(), v[:n.value].copy()

    def bow_score(self, w1, v1, w2, v2):
        w1 = np.ascontiguousarray(w1, np.uint32)
        w2 = np.ascontiguousarray(w2, np.uint32)
        v1 = np.ascontiguousarray(v1, np.float64)
        v2 = np.ascontiguousarray(v2, np.float64)
        s = C.c_double(0)
        self._chk(self.L.mslam_hip_bow_score(self._h, _p(w1), _p(v1), len(w1), _p(w2), _p(v2), len(w2), C.byref(s)))
        return s.value

    def bow_db_add(self, desc):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        e = C.c_int(-1)
        self._chk(self.L.mslam_hip_bow_db_add(self._h, _p(d), len(d), C.byref(e)))
        return e.value

    def bow_db_query(self, desc, max_results=4):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        ids = np.empty(max(max_results, 1), np.int32)
        sc = np.empty(max(max_results, 1), np.float64)
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_bow_db_query(self._h, _p(d), len(d), max_results, _p(ids), _p(sc), C.byref(n)))
        return ids[:n.value].copy(), sc[:n.value].copy()

    def bow_db_remove(self, entry_id):
        self._chk(self.L.mslam_hip_bow_db_remove(self._h, int(entry_id)))

    def bow_db_reserve(self, max_entries):
        self._chk(self.L.mslam_hip_bow_db_reserve(self._h, int(max_entries)))

    def bow_db_size(self):
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_bow_db_size(self._h, C.byref(n)))
        return n.value

    def bow_db_clear(self):
        self._chk(self.L.mslam_hip_bow_db_clear(self._h))

    def bow_batch_dev(self, add_to_db=True):
        self._chk(self.L.mslam_hip_bow_batch_dev(self._h, int(bool(add_to_db))))

    def bow_cross_score_dev(self, d_words, d_values, d_n, n_sets, capacity, d_scores):
        self._chk(self.L.mslam_hip_bow_cross_score_dev(self._h, C.c_void_p(d_words), C.c_void_p(d_values),
                                                       C.c_void_p(d_n), int(n_sets), int(capacity),
                                                       C.c_void_p(d_scores)))

    def bow_pack_dev(self, k_max, d_out):
        self._chk(self.L.mslam_hip_bow_pack_dev(self._h, int(k_max), C.c_void_p(d_out)))

    def bow_cross_score_packed_dev(self, d_sets, n_sets, self_set, n_frames, k_max, d_scores, stream=None):
        self._chk(self.L.mslam_hip_bow_cross_score_packed_dev(self._h, C.c_void_p(d_sets), int(n_sets), int(self_set),
                                                              int(n_frames), int(k_max), C.c_void_p(d_scores),
                                                              C.c_void_p(stream)))

    def bow_view(self):
        v = BowView()
        self._chk(self.L.mslam_hip_get_bow_view(self._h, C.byref(v)))
        return v

    # ---- debug ---------------------------------------------------------------------------------
    def level_geometry(self):
        n = self.params.n_levels
        w = (C.c_int * 16)()
        h = (C.c_int * 16)()
        s = (C.c_float * 16)()
        self._chk(self.L.mslam_hip_level_geometry(self._h, w, h, s))
        return list(w[:n]), list(h[:n]), np.array(s[:n], np.float32)

    def debug_image(self, what, frame, level):
        w, h, _ = self.level_geometry()
        out = np.empty((h[level], w[level]), np.uint8)
        n = C.c_size_t(0)
        self._chk(self.L.mslam_hip_debug_read(self._h, what, frame, level, _p(out), C.c_size_t(out.size), C.byref(n)))
        return out

    def debug_keypoints(self, what, frame, level):
        out = np.empty((self.params.max_candidates, 3), np.float32)
        n = C.c_size_t(0)
        self._chk(self.L.mslam_hip_debug_read(self._h, what, frame, level, _p(out), C.c_size_t(out.nbytes),
                                              C.byref(n)))
        return out[:n.value].copy()

    def debug_cells(self, level):
        """[n_cells, 6] the level's FAST cells (x0, y0, cw, ch, ox, oy) in launch order (in-tree detector)"""
        out = np.empty((2048, 6), np.int32)
        n = C.c_size_t(0)
        self._chk(self.L.mslam_hip_debug_read(self._h, DBG_CELLS, 0, level, _p(out), C.c_size_t(out.nbytes),
                                              C.byref(n)))
        return out[:n.value].copy()

    def debug_forms(self):
        """(levels produced by the fused level kernels, 1 when the blurred slab is kept in tiles) of this context"""
        out = np.zeros(2, np.int32)
        n = C.c_size_t(0)
        self._chk(self.L.mslam_hip_debug_read(self._h, DBG_FORMS, 0, 0, _p(out), C.c_size_t(out.nbytes), C.byref(n)))
        return int(out[0]), int(out[1])

    def debug_quad_direct_levels(self):
        """per level: True when its quadtree selection runs in the direct form (pairs of at most QUAD_DIRECT_MAX_CANDIDATES)"""
        out = np.zeros(1, np.uint32)
        n = C.c_size_t(0)
        self._chk(self.L.mslam_hip_debug_read(self._h, DBG_QUAD_DIRECT, 0, 0, _p(out), C.c_size_t(out.nbytes), C.byref(n)))
        return [bool((int(out[0]) >> l) & 1) for l in range(self.params.n_levels)]

    def debug_counts(self, what, n_frames):
        """[n_frames, n_levels] FAST candidates (DBG_CANDIDATES) or selected keypoints (DBG_SELECTED) of the last batch"""
        out = np.zeros((max(n_frames, 1), self.params.n_levels), np.int32)
        self._chk(self.L.mslam_hip_debug_counts(self._h, int(what), _p(out), int(out.shape[0])))
        return out[:n_frames]

    def set_profiling(self, enable):
        """0 = off, 1/True = every stage, serialised on one stream, 2 = every stage launch, in place."""
        self._chk(self.L.mslam_hip_set_profiling(self._h, int(enable)))

    def stage_times(self, cap=256):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = C.c_int(0)
        self._chk(self.L.mslam_hip_get_stage_times(self._h, names, ms, cap, C.byref(n)))
        return [(names[i].decode(), ms[i]) for i in range(n.value)]


def qlz_decompress(data, n_packets, capacity=None):
    """host-only: decode consecutive QuickLZ packets (what follows nChunks in a compressed DBoW3 vocabulary)"""
    src = np.frombuffer(bytes(data), np.uint8)
    cap = capacity if capacity is not None else 10000 * n_packets + 16
    dst = np.empty(max(cap, 1), np.uint8)
    n = C.c_size_t(0)
    L = lib()
    L.mslam_hip_qlz_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    rc = L.mslam_hip_qlz_decompress(_p(src), src.size, int(n_packets), _p(dst), dst.size, C.byref(n))
    if rc != OK:
        raise MslamHipError(rc, "qlz_decompress failed")
    return dst[:n.value].tobytes()


# ---- mirrors of the reference plugin interfaces ---------------------------------------------------
class RgbFrame:
    """types/rgb_frame.hpp:12-16 — interleaved 3-channel bytes (B,G,R as the providers deliver them)."""

    def __init__(self, data, width, height):
        self.data = np.ascontiguousarray(data, np.uint8).reshape(height, width, 3)
        self.size = (width, height)


class OrbKeypoint:
    """KeypointDescriptor<uint8_t,32> (feature_interface.hpp:18-30): keypoint {id, coordinates} + descriptor."""
    __slots__ = ("id", "coordinates", "descriptor")

    def __init__(self, id, coordinates, descriptor):
        self.id, self.coordinates, self.descriptor = id, coordinates, descriptor


class HipOrbDetector:
    """IFeatureDetector<RgbFrame, uint8_t, 32> backed by the HIP extractor
    (drop-in for DistributedOrbOpenCvDetector, distributed_cv_feature.cpp:1181-1222)."""

    def __init__(self, width=640, height=480, **kw):
        self.ctx = Context(width=width, height=height, **kw)

    def detect(self, sensorData):
        r = self.ctx.detect(sensorData.data)
        # id = running index, coordinates widened to double (distributed_cv_feature.cpp:1203-1208)
        return [OrbKeypoint(i, (float(x), float(y)), d) for i, ((x, y), d) in enumerate(zip(r["xy"].astype(np.float64),
                                                                                          r["desc"]))]


class HipOrbMatcher:
    """IFeatureMatcher<uint8_t, 32> (drop-in for OrbOpenCvMatcher, orb_feature.cpp:84-130)."""

    def __init__(self, ctx=None, ratio=0.7):
        self.ctx = ctx or Context()
        self.ratio = ratio

    def match(self, firstDescriptors, secondDescriptors):
        f = np.array([k.descriptor for k in firstDescriptors], np.uint8).reshape(-1, 32)
        t = np.array([k.descriptor for k in secondDescriptors], np.uint8).reshape(-1, 32)
        fi, ti = self.ctx.match(f, t, self.ratio)
        return [(int(a), int(b)) for a, b in zip(fi, ti)]  # DescriptorMatch{fromIndex, toIndex}


class HipOrbRelocalizer:
    """IRelocalizer<SensorState, uint8_t, 32> over the DBoW3 database kernels
    (what OrbRelocalizer is wired for, orb_relocalizer.cpp:26-50)."""

    def __init__(self, vocabulary_blob, ctx=None, max_results=4):
        self.ctx = ctx or Context()
        self.ctx.bow_load(vocabulary_blob)
        self.max_results = max_results
        self._entry_to_keyframe = {}
        self._with_landmarks = set()   # entries addKeyframeLandmarks has stored landmarks for

    def addKeyframe(self, keyframe, keypoints):
        assert len(keypoints) > 0  # orb_relocalizer.cpp:42
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        self._entry_to_keyframe[self.ctx.bow_db_add(d)] = keyframe

    def removeKeyframe(self, keyframe):
        for e, k in list(self._entry_to_keyframe.items()):
            if k is keyframe:
                del self._entry_to_keyframe[e]
                self.ctx.bow_db_remove(e)
                if e in self._with_landmarks:
                    self._with_landmarks.discard(e)
                    self.ctx.kf_remove(e)

    def addKeyframeLandmarks(self, keyframe, keypoints, worldPoints):
        """extension: the landmarks of a keyframe addKeyframe has fed (descriptors of `keypoints` + their world points),
        stored on the device under the keyframe's BoW entry id — what relocalizePose verifies candidates against"""
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        for e, k in self._entry_to_keyframe.items():
            if k is keyframe:
                self.ctx.kf_add(e, d, np.asarray(worldPoints, np.float64).reshape(-1, 3))
                self._with_landmarks.add(e)
                return
        raise KeyError("addKeyframeLandmarks: the keyframe has not been added")

    def _verify(self, keypoints, entries, camera, valid, rvec, tvec, min_inliers, seed):
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        xy = np.array([k.coordinates for k in keypoints], np.float32).reshape(-1, 2)
        focal, principal = camera
        r = self.ctx.relocalize(d, xy, entries, focal, principal, valid=valid, rvec=rvec, tvec=tvec, min_inliers=min_inliers,
                                seed=seed)
        table = [dict(c, keyframe=self._entry_to_keyframe[e]) for e, c in zip(entries, r["candidates"])]
        if r["best"] < 0:
            return None, None, 0, table
        b = table[r["best"]]
        return b["keyframe"], (b["rvec"], b["tvec"]), b["n_inliers"], table

    def relocalizePose(self, keypoints, camera=((525.0, 525.0), (319.5, 239.5)), valid=None, rvec=None, tvec=None,
                       min_inliers=60, seed=0):
        """extension (what RgbdFeatureFrontend::relocalize's commented body does, rgbd_feature_frontend.cpp:495-534): the BoW
        candidates of relocalize(), each verified by match + RANSAC PnP against its stored landmarks
        -> (keyframe, (rvec, tvec), inliers, per-candidate table), keyframe None when no candidate reaches min_inliers"""
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        ids, _ = self.ctx.bow_db_query(d, self.max_results + len(self._entry_to_keyframe))
        entries = [int(i) for i in ids if i in self._entry_to_keyframe][:self.max_results]   # relocalize()'s candidates
        entries = [e for e in entries if e in self._with_landmarks]                           # (only stored ones can be verified)
        return self._verify(keypoints, entries, camera, valid, rvec, tvec, min_inliers, seed)

    def relocalize(self, keypoints):
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        ids, _ = self.ctx.bow_db_query(d, self.max_results + len(self._entry_to_keyframe))
        out = [self._entry_to_keyframe[i] for i in ids if i in self._entry_to_keyframe]
        return out[:self.max_results]


class HipLoopDetector:
    """ILoopDetector<State>: detectLoop() takes no arguments (loop_detection.hpp:10-15), so it is fed
    through the relocalizer's addKeyframe; it reports the best-scoring earlier keyframe of the most
    recently added one, or None."""

    def __init__(self, relocalizer, min_score=0.05, exclude_recent=1):
        self.reloc = relocalizer
        self.min_score = min_score
        self.exclude_recent = exclude_recent
        self._last = None
        self._last_entry, self._last_keypoints = None, None

    def feed(self, keyframe, keypoints):
        d = np.array([k.descriptor for k in keypoints], np.uint8).reshape(-1, 32)
        n_db = len(self.reloc._entry_to_keyframe)
        ids, sc = self.reloc.ctx.bow_db_query(d, n_db) if n_db else (np.empty(0, np.int32), np.empty(0))
        self._last = None
        self._last_entry, self._last_keypoints = None, keypoints
        for i, s in zip(ids, sc):
            if s >= self.min_score and i < n_db - self.exclude_recent and i in self.reloc._entry_to_keyframe:
                self._last = self.reloc._entry_to_keyframe[i]
                self._last_entry = int(i)
                break
        self.reloc.addKeyframe(keyframe, keypoints)

    def detectLoop(self):
        return self._last

    def detectLoopVerified(self, camera=((525.0, 525.0), (319.5, 239.5)), valid=None, rvec=None, tvec=None, min_inliers=60,
                           seed=0):
        """extension: detectLoop()'s candidate for the last fed keyframe, verified by match + RANSAC PnP against its stored
        landmarks -> (keyframe, (rvec, tvec), inliers, per-candidate table); keyframe None when there is no candidate, it has
        no stored landmarks, or it has fewer than min_inliers inliers"""
        if self._last_entry is None or self._last_entry not in self.reloc._with_landmarks:
            return None, None, 0, []
        return self.reloc._verify(self._last_keypoints, [self._last_entry], camera, valid, rvec, tvec, min_inliers, seed)


def rotation_to_quaternion(R):
    """unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (the branch with the largest divisor)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = [R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1], R[0, 0] + R[1, 1] + R[2, 2]]
    i = int(np.argmax(t))
    r = np.sqrt(1.0 + t[i])
    if i == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], r * r]) / (2.0 * r)
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = r * r, R[j, i] + R[i, j], R[k, i] + R[i, k], R[k, j] - R[j, k]
        q /= 2.0 * r
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def quaternion_to_rotation(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rvec_to_rotation(rvec):
    """Rodrigues' formula: the rotation matrix of an axis-angle vector"""
    w = np.asarray(rvec, np.float64).reshape(3)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def rotation_to_rvec(R):
    """the axis-angle vector of a rotation matrix, through the unit quaternion with w >= 0 (an angle in [0, pi])"""
    q = rotation_to_quaternion(R)
    n = np.linalg.norm(q[:3])
    return np.zeros(3) if n < 1e-300 else 2.0 * np.arctan2(n, q[3]) * q[:3] / n


def quaternion_product(a, b):
    """a (x) b, x y z w"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def relative_pose(Ta, Tb):
    """T_a^-1 o T_b for two states (qx qy qz qw px py pz): pose b in a's frame, the measurement of a pose-graph edge (a, b)"""
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    qi = np.array([-Ta[0], -Ta[1], -Ta[2], Ta[3]]) / np.dot(Ta[:4], Ta[:4])
    q = quaternion_product(qi, Tb[:4])
    return np.concatenate([q / np.linalg.norm(q), quaternion_to_rotation(Ta[:4]).T @ (Tb[4:] - Ta[4:])])


class HipBackend:
    """CeresBackend (ceres_backend.cpp) on Context.bundle_adjust: the keyframes' states (camera -> world: qx qy qz qw px py
    pz), their observations (landmark id, camera-frame point: what ReprojectionError's constructor forms, :24-28) and the
    landmarks' world points, kept on the host; the solve runs on the device.  The first keyframe added is constant, as the
    reference's keyframe 1 is (:155-159).  By default nothing is removed: the outlier observations are returned.
    remove_observations() is the backend's side of removeObservation (rgbd_feature_frontend.cpp:469-487, a body the
    reference leaves commented out), and local_ba / global_ba with prune = True use it: solve, remove the result's
    outlier_observations, and when any were removed solve once more from the refined state (one extra round, not a loop).
    The returned dict is the last solve's and gains pruned = dict(pairs = [(keyframe id, landmark id), ...], first = the
    first solve's dict); a FAILURE of the first solve prunes nothing.  By default the cost has no loss function, so one gross outlier
    can drag its landmark until the landmark's good observations are flagged too, and the landmark then goes with them.
    loss = ("huber", a) or ("cauchy", a) (a in metres; an extension, the reference has no loss): every solve of this backend
    runs with Context.set_ba_loss(kind, a) and puts the context's previous setting back afterwards, also when the solve
    raises; the costs in the result are then 1/2 sum rho.  loss = None (the default) never touches the setting.
    The backend never touches the keyframe store: its caller does (Context.kf_remove_observations with pruned["pairs"]).
    remove_keyframe() is the backend's side of keyframe culling (Context.kf_cull): every keyframe but the first can leave.
    remove_landmarks() is the backend's side of landmark culling (Context.kf_cull_landmarks): the ids leave every keyframe.
    global_solver = True: global_ba() goes through
    Context.bundle_adjust_global and takes up to 1024 keyframes; local_ba and neighbours are the same in both modes.
    close_loop() is the body of the reference's empty closeLoop (rgbd_feature_frontend.cpp:577-580): a pose graph over every
    keyframe on Context.pose_graph; self.anchor names, per landmark, the keyframe that created it.
    pose_graph_solver = "sparse": close_loop runs with Context.set_pose_graph_solver("sparse") and puts the context's previous
    setting back afterwards, also when the solve raises, and takes up to 16384 keyframes.  "dense" (the default) never touches
    the setting, as loss = None does not (a context is DENSE unless its owner said otherwise), and takes up to 1024.
    global_ba() has its own setting: global_linear_solver = "sparse" (with global_solver = True) runs it with
    Context.set_ba_global_solver("sparse"), puts the context's previous setting back afterwards, also when the solve raises,
    and takes up to 16384 keyframes; "dense" (the default) never touches the setting and takes up to 1024.
    global_pcg = (max_iterations, tolerance) or True for the defaults (needs global_solver = True, else
    MslamHipError(E_INVALID), as bad values are, before a context is touched; an extension): global_ba() runs with
    Context.set_ba_global_pcg and puts the context's previous setting back afterwards, also when the solve raises, takes up to
    16384 keyframes whatever global_linear_solver is, and its result gains pcg = Context.ba_global_pcg_stats().  None (the
    default) never touches the setting.
    pose_graph_pcg = (max_iterations, tolerance) or True for the defaults (bad values are MslamHipError(E_INVALID) before a
    context is touched; an extension): close_loop runs with Context.set_pose_graph_pcg and puts the context's previous setting
    back afterwards, also when the solve raises, takes up to 16384 keyframes whatever pose_graph_solver is, and its result
    gains pcg = Context.pose_graph_pcg_stats().  None (the default) never touches the setting.
    pose_graph_loss = ("huber", a) or ("cauchy", a) (a in the unit of the weighted residual; an extension): close_loop runs
    with Context.set_pose_graph_loss(kind, a) and puts the context's previous setting back afterwards, also when the solve
    raises; its result gains edge_chi2 and edge_weight (Context.pose_graph_edge_weights at the returned poses; the loop edge
    is the last).  None (the default) never touches the setting.  No rejection policy follows from the weights here:
    loop_problem() has one loop edge on odometry edges measured at the current poses, a chain always bends to such an
    edge, and the weight at the solution says nothing about whether the loop was right."""

    MAX_KEYFRAMES = 64
    MAX_GLOBAL_KEYFRAMES = 1024
    MAX_GLOBAL_KEYFRAMES_SPARSE = BA_GLOBAL_MAX_KEYFRAMES_SPARSE

    def __init__(self, ctx, max_iterations=100, outlier_threshold=0.15, global_solver=False, loss=None, pose_graph_solver="dense",
                 global_linear_solver="dense", pose_graph_loss=None, global_pcg=None, pose_graph_pcg=None):
        self.global_pcg = _pcg_setting(global_pcg, "HipBackend")    # of Context.set_ba_global_pcg
        self.pose_graph_pcg = _pcg_setting(pose_graph_pcg, "HipBackend", "pose_graph_pcg")    # of Context.set_pose_graph_pcg
        if self.global_pcg is not None and not global_solver:
            raise MslamHipError(E_INVALID, "HipBackend: global_pcg needs global_solver = True")
        self.ctx, self.max_iterations, self.outlier_threshold = ctx, int(max_iterations), float(outlier_threshold)
        self.pose_graph_solver = _pg_solver_kind(pose_graph_solver, "HipBackend")    # of Context.set_pose_graph_solver
        if self.pose_graph_solver not in (PG_SOLVER_DENSE, PG_SOLVER_SPARSE):
            raise MslamHipError(E_INVALID, "HipBackend: pose_graph_solver %r is not dense / sparse" % (pose_graph_solver,))
        self.global_solver = bool(global_solver)
        self.global_linear_solver = _pg_solver_kind(global_linear_solver, "HipBackend")    # of Context.set_ba_global_solver
        if self.global_linear_solver not in (BA_GLOBAL_SOLVER_DENSE, BA_GLOBAL_SOLVER_SPARSE):
            raise MslamHipError(E_INVALID, "HipBackend: global_linear_solver %r is not dense / sparse" % (global_linear_solver,))
        self.loss = None if loss is None else (loss[0], float(loss[1]))    # (kind, scale) of Context.set_ba_loss
        # (kind, scale) of Context.set_pose_graph_loss
        self.pose_graph_loss = None if pose_graph_loss is None else (pose_graph_loss[0], float(pose_graph_loss[1]))
        self.poses = {}       # id -> [7]
        self.obs = {}         # id -> (landmark ids [n] i64, camera points [n, 3])
        self.landmarks = {}   # landmark id -> [3]
        self.anchor = {}      # landmark id -> the keyframe that created it (close_loop moves the landmark with that keyframe)
        self.first = None

    def add_keyframe(self, id, pose, landmark_ids, cam_points):
        """a keyframe with its observations; a landmark id the backend has not seen starts at the world point the
        observation gives under this pose (addNewLandmarks' toGlobalCoordinates)"""
        pose = np.array(pose, np.float64).reshape(7)
        lids = np.array(landmark_ids, np.int64).reshape(-1)
        cam = np.array(cam_points, np.float64).reshape(-1, 3)
        if len(lids) != len(cam):
            raise MslamHipError(E_INVALID, "add_keyframe: %d landmark ids, %d camera points" % (len(lids), len(cam)))
        if self.first is None:
            self.first = int(id)
        self.poses[int(id)] = pose
        self.obs[int(id)] = (lids, cam)
        world = cam @ quaternion_to_rotation(pose[:4]).T + pose[4:]
        for l, w in zip(lids.tolist(), world):
            self.landmarks.setdefault(l, w.copy())
            self.anchor.setdefault(l, int(id))

    def neighbours(self, ref, graph, deep_level=1):
        """getNeighbourKeyframes (basic_map.cpp:209-237) with its `level <= deepLevel` test, as HipKeyframeTracker.neighbours
        restates it; more than 64: the 64 largest ids"""
        result, queue = set(), [(ref, 0)]
        while queue:
            cur, level = queue.pop(0)
            result.add(cur)
            if level <= deep_level:
                queue.extend((nb, level + 1) for nb in sorted(graph.get(cur, ())) if nb not in result)
        return sorted(k for k in result if k in self.poses)[-self.MAX_KEYFRAMES:]

    def problem(self, kf_ids):
        """the arrays Context.bundle_adjust takes for the listed keyframes -> (poses, fixed, landmark id list, landmarks,
        obs_kf, obs_lm, obs_cam)"""
        index, lids, okf, olm, ocam = {}, [], [], [], []
        for k, id in enumerate(kf_ids):
            ids, cam = self.obs[id]
            for l in ids.tolist():
                if l not in index:
                    index[l] = len(lids)
                    lids.append(l)
            okf.append(np.full(len(ids), k, np.int32))
            olm.append(np.array([index[l] for l in ids.tolist()], np.int32))
            ocam.append(cam)
        poses = np.array([self.poses[id] for id in kf_ids], np.float64).reshape(-1, 7)
        fixed = np.array([id == self.first for id in kf_ids], np.uint8)
        lm = np.array([self.landmarks[l] for l in lids], np.float64).reshape(-1, 3)
        cat = lambda a, dt, w: np.concatenate(a) if a else np.zeros((0,) + w, dt)
        return poses, fixed, lids, lm, cat(okf, np.int32, ()), cat(olm, np.int32, ()), cat(ocam, np.float64, (3,))

    def _solve(self, kf_ids, blocked=False):
        poses, fixed, lids, lm, okf, olm, ocam = self.problem(kf_ids)
        solve = self.ctx.bundle_adjust_global if blocked else self.ctx.bundle_adjust
        if self.loss is None:
            res = solve(poses, lm, okf, olm, ocam, fixed, self.max_iterations, self.outlier_threshold)
        else:
            # the setting belongs to the context: this backend's loss holds for this solve only, also when it raises
            before = self.ctx.get_ba_loss()
            self.ctx.set_ba_loss(*self.loss)
            try:
                res = solve(poses, lm, okf, olm, ocam, fixed, self.max_iterations, self.outlier_threshold)
            finally:
                self.ctx.set_ba_loss(*before)
        if res["termination"] != 2:
            for k, id in enumerate(kf_ids):
                self.poses[id] = res["poses"][k].copy()
            for i, l in enumerate(lids):
                self.landmarks[l] = res["landmarks"][i].copy()
        res.update(keyframes=list(kf_ids), landmark_ids=np.array(lids, np.int64),
                   outlier_observations=[(kf_ids[k], lids[l]) for k, l in zip(okf[res["outlier"]], olm[res["outlier"]])])
        return res

    def remove_observations(self, pairs):
        """removeObservation's bookkeeping (rgbd_feature_frontend.cpp:469-487) for (keyframe id, landmark id) pairs: the
        named observations leave self.obs, every position that holds the id; a landmark whose anchor keyframe no longer
        observes it is re-anchored to the smallest keyframe id that still does; a landmark with no observation left leaves
        `landmarks` and `anchor`.  A pair the backend does not hold is ignored.  -> the number of observations dropped"""
        gone = {}
        for kf, lid in pairs:
            gone.setdefault(int(kf), set()).add(int(lid))
        n, touched = 0, set()
        for kf, drop in gone.items():
            if kf not in self.obs:
                continue
            lids, cam = self.obs[kf]
            hit = np.array([l in drop for l in lids.tolist()], bool).reshape(-1)
            if hit.any():
                n += int(np.count_nonzero(hit))
                touched.update(lids[hit].tolist())
                self.obs[kf] = (lids[~hit].copy(), cam[~hit].copy())
        observers = {}
        if touched:
            for kf in sorted(self.obs):
                for l in touched.intersection(self.obs[kf][0].tolist()):
                    observers.setdefault(l, []).append(kf)
        for l in touched:
            who = observers.get(l)
            if not who:
                self.landmarks.pop(l, None)
                self.anchor.pop(l, None)
            elif self.anchor.get(l) not in who:
                self.anchor[l] = who[0]
        return n

    def remove_keyframe(self, id):
        """keyframe culling's bookkeeping (BasicMap::removeKeyframe, basic_map.cpp:110-115, with what the landmarks need):
        the keyframe leaves `poses` and `obs`; a landmark anchored at it is re-anchored to the smallest remaining keyframe id
        that observes it; a landmark nobody observes any more leaves `landmarks` and `anchor`.  The first keyframe (the
        gauge: it alone is constant) and an id the backend does not hold are MslamHipError(E_INVALID)
        -> dict(n_observations = the observations dropped, orphans = the landmark ids that left, ascending)"""
        id = int(id)
        if id not in self.poses or id == self.first:
            raise MslamHipError(E_INVALID, "remove_keyframe: %r is the first keyframe or not a keyframe of the backend" % id)
        lids, _ = self.obs.pop(id)
        del self.poses[id]
        touched, observers = set(lids.tolist()), {}
        for kf in sorted(self.obs):
            for l in touched.intersection(self.obs[kf][0].tolist()):
                observers.setdefault(l, []).append(kf)
        orphans = []
        for l in sorted(touched):
            who = observers.get(l)
            if not who:
                self.landmarks.pop(l, None)
                self.anchor.pop(l, None)
                orphans.append(l)
            elif self.anchor.get(l) == id:
                self.anchor[l] = who[0]
        return dict(n_observations=len(lids), orphans=orphans)

    def remove_landmarks(self, lids):
        """landmark culling's bookkeeping (Context.kf_cull_landmarks): the listed landmark ids leave every keyframe's
        observations, at every position, and leave `landmarks` and `anchor`; an id the backend does not hold is ignored
        -> dict(n_observations = the observations dropped, n_landmarks = the landmarks that left)"""
        gone = set(int(l) for l in np.asarray(lids, np.int64).reshape(-1).tolist())
        n_obs = 0
        if gone:
            for kf in sorted(self.obs):
                ids, cam = self.obs[kf]
                hit = np.array([l in gone for l in ids.tolist()], bool).reshape(-1)
                if hit.any():
                    n_obs += int(np.count_nonzero(hit))
                    self.obs[kf] = (ids[~hit].copy(), cam[~hit].copy())
        n_lm = 0
        for l in gone:
            n_lm += self.landmarks.pop(l, None) is not None
            self.anchor.pop(l, None)
        return dict(n_observations=n_obs, n_landmarks=n_lm)

    def _solve_pruned(self, kf_ids, blocked, prune):
        """_solve; with prune, the result's outlier observations are removed and, when any were, one more solve from the
        refined state follows (one extra round, not a loop): the last solve's dict plus pruned = dict(pairs, first)"""
        res = self._solve(kf_ids, blocked)
        if not prune:
            return res
        first, pairs = dict(res), []
        if res["termination"] != 2:
            pairs = sorted(set(res["outlier_observations"]))
            if self.remove_observations(pairs) > 0:
                res = self._solve(kf_ids, blocked)
        res["pruned"] = dict(pairs=pairs, first=first)
        return res

    def local_ba(self, ref_id, graph, prune=False):
        """localBundleAdjustment (:162-171): the observations of getNeighbourKeyframes(ref, deepLevel = 1).  prune: see
        the class docstring"""
        return self._solve_pruned(self.neighbours(ref_id, graph, 1), False, prune)

    def global_ba(self, prune=False):
        """globalBundleAdjustment (:173-183) over every keyframe; more than 64 (with global_solver 1024: the reduced system is
        dense; 16384 with global_linear_solver = "sparse" too) is MslamHipError(E_CAPACITY), raised before the context is
        touched.  prune: see the class docstring"""
        sparse = self.global_solver and self.global_linear_solver == BA_GLOBAL_SOLVER_SPARSE
        pcg = self.global_pcg if self.global_solver else None
        cap = self.MAX_GLOBAL_KEYFRAMES_SPARSE if sparse or pcg else self.MAX_GLOBAL_KEYFRAMES if self.global_solver else self.MAX_KEYFRAMES
        if len(self.poses) > cap:
            raise MslamHipError(E_CAPACITY, "global_ba: %d keyframes, at most %d per solve" % (len(self.poses), cap))
        if pcg:
            before = self.ctx.get_ba_global_pcg()
            self.ctx.set_ba_global_pcg(True, *pcg)
            try:
                res = self._solve_pruned(sorted(self.poses), True, prune)
                res["pcg"] = self.ctx.ba_global_pcg_stats()
                return res
            finally:
                self.ctx.set_ba_global_pcg(*before)
        if not sparse:
            return self._solve_pruned(sorted(self.poses), self.global_solver, prune)
        before = self.ctx.get_ba_global_solver()
        self.ctx.set_ba_global_solver(BA_GLOBAL_SOLVER_SPARSE)
        try:
            return self._solve_pruned(sorted(self.poses), True, prune)
        finally:
            self.ctx.set_ba_global_solver(before)

    def fuse(self, keep_lids, drop_lids):
        """landmark fusion's bookkeeping: every observation of drop_lids[p] becomes one of keep_lids[p] (simultaneously, the
        later of a repeated drop id wins, as Context.kf_replace_ids), `landmarks` and `anchor` lose the dropped ids, the kept
        landmark keeps its point and its anchor -> the number of observations rewritten"""
        keep = np.asarray(keep_lids, np.int64).reshape(-1).tolist()
        drop = np.asarray(drop_lids, np.int64).reshape(-1).tolist()
        if len(keep) != len(drop):
            raise MslamHipError(E_INVALID, "fuse: %d keep ids, %d drop ids" % (len(keep), len(drop)))
        to = dict(zip(drop, keep))
        n = 0
        for id, (lids, cam) in self.obs.items():
            new = np.array([to.get(l, l) for l in lids.tolist()], np.int64).reshape(-1)
            n += int(np.count_nonzero([l in to for l in lids.tolist()]))
            self.obs[id] = (new, cam)
        for d, k in to.items():
            if d != k:
                self.landmarks.pop(d, None)
                self.anchor.pop(d, None)
        return n

    def loop_problem(self, cur_id, loop_id, rvec, tvec, graph, sqrt_info=None):
        """the arrays Context.pose_graph takes for a loop between keyframes loop_id and cur_id -> (keyframe ids, poses,
        fixed, edge_a, edge_b, edge_meas, sqrt_info): every graph edge i < j with both ends in self.poses, in sorted order,
        measured on the current poses (T_i^-1 T_j: an odometry edge holds what is believed now); the loop edge
        (loop_id, cur_id, Z) last, Z = T_loop^-1 o T_cur* with T_cur* = (R^T, -R^T t) the pose (rvec, tvec) names.
        sqrt_info (6 x 6, or None) weighs the loop edge; the others are identity."""
        ids = sorted(self.poses)
        index = {id: k for k, id in enumerate(ids)}
        poses = np.array([self.poses[id] for id in ids], np.float64).reshape(-1, 7)
        ea, eb, meas = [], [], []
        for i in ids:
            for j in sorted(graph.get(i, ())):
                if i < j and j in index:
                    ea.append(index[i]), eb.append(index[j]), meas.append(relative_pose(self.poses[i], self.poses[j]))
        R = rvec_to_rotation(rvec)
        T_cur = np.concatenate([rotation_to_quaternion(R.T), -R.T @ np.asarray(tvec, np.float64).reshape(3)])
        ea.append(index[int(loop_id)]), eb.append(index[int(cur_id)]), meas.append(relative_pose(self.poses[int(loop_id)], T_cur))
        info = None
        if sqrt_info is not None:
            info = np.tile(np.eye(6), (len(ea), 1, 1))
            info[-1] = np.asarray(sqrt_info, np.float64).reshape(6, 6)
        fixed = np.array([id == self.first for id in ids], np.uint8)
        return ids, poses, fixed, np.array(ea, np.int32), np.array(eb, np.int32), np.array(meas, np.float64).reshape(-1, 7), info

    def close_loop(self, cur_id, loop_id, rvec, tvec, graph, sqrt_info=None, covariance=False):
        """closeLoop: (rvec, tvec) is the world -> camera pose of keyframe cur_id found by PnP against loop_id's stored
        landmarks.  Solves loop_problem() on the device; on a usable termination the poses are replaced and every landmark
        moves rigidly with its anchor keyframe, X' = T_a' T_a^-1 X.  -> the summary and keyframes, poses_before, poses,
        landmark_ids, landmarks (FAILURE: everything as it was).  More than 1024 keyframes (16384 with
        pose_graph_solver = "sparse" or with pose_graph_pcg) is MslamHipError(E_CAPACITY), a keyframe the backend does not
        hold MslamHipError(E_INVALID), both raised before the context is touched.  With pose_graph_pcg the result gains pcg.
        covariance = True (an extension): after a usable termination one Context.pose_graph_covariance call on the same
        problem at the solved poses, under the same loss; the result gains covariance = dict(cur, loop, cross): the 6 x 6
        marginals of cur_id and loop_id on the tangent (delta, dp) and cross = E[d_cur d_loop^T] (the loop edge joins the
        two, so the block is inside the envelope; a constant keyframe gives zeros).  None when the problem is rank
        deficient (E_NO_MODEL: no constant keyframe in the graph's component).  With False nothing new runs.  The
        covariance keeps the envelope factor and its bound under pose_graph_pcg too: on a graph whose envelope is above
        POSE_GRAPH_MAX_ENVELOPE_BLOCKS the solve succeeds with PCG and the covariance call's MslamHipError(E_CAPACITY)
        propagates, as it does with the other solvers."""
        sparse_cap = self.pose_graph_solver == PG_SOLVER_SPARSE or self.pose_graph_pcg is not None
        cap = POSE_GRAPH_MAX_KEYFRAMES_SPARSE if sparse_cap else POSE_GRAPH_MAX_KEYFRAMES
        if len(self.poses) > cap:
            raise MslamHipError(E_CAPACITY, "close_loop: %d keyframes, at most %d per solve" % (len(self.poses), cap))
        if int(cur_id) not in self.poses or int(loop_id) not in self.poses or int(cur_id) == int(loop_id):
            raise MslamHipError(E_INVALID, "close_loop: keyframes %r and %r must be two keyframes of the backend" % (cur_id, loop_id))
        ids, poses, fixed, ea, eb, meas, info = self.loop_problem(cur_id, loop_id, rvec, tvec, graph, sqrt_info)
        if self.pose_graph_loss is not None:
            loss_before = self.ctx.get_pose_graph_loss()
            self.ctx.set_pose_graph_loss(*self.pose_graph_loss)
        try:
            if self.pose_graph_pcg is not None:
                before = self.ctx.get_pose_graph_pcg()
                self.ctx.set_pose_graph_pcg(True, *self.pose_graph_pcg)
                try:
                    res = self.ctx.pose_graph(poses, ea, eb, meas, info, fixed, self.max_iterations)
                    res["pcg"] = self.ctx.pose_graph_pcg_stats()
                finally:
                    self.ctx.set_pose_graph_pcg(*before)
            elif self.pose_graph_solver == PG_SOLVER_SPARSE:
                before = self.ctx.get_pose_graph_solver()
                self.ctx.set_pose_graph_solver(PG_SOLVER_SPARSE)
                try:
                    res = self.ctx.pose_graph(poses, ea, eb, meas, info, fixed, self.max_iterations)
                finally:
                    self.ctx.set_pose_graph_solver(before)
            else:
                res = self.ctx.pose_graph(poses, ea, eb, meas, info, fixed, self.max_iterations)
            if self.pose_graph_loss is not None:
                chi2, weight = self.ctx.pose_graph_edge_weights(res["poses"], ea, eb, meas, info)
                res.update(edge_chi2=chi2, edge_weight=weight)
            if covariance and res["termination"] != 2:
                kc, kl = ids.index(int(cur_id)), ids.index(int(loop_id))
                try:
                    cv = self.ctx.pose_graph_covariance(res["poses"], ea, eb, meas, info, fixed, poses_of=[kc, kl], pairs=[(kc, kl)])
                    res.update(covariance=dict(cur=cv["cov"][0], loop=cv["cov"][1], cross=cv["cross"][0]))
                except MslamHipError as e:
                    if e.code != E_NO_MODEL:
                        raise
                    res.update(covariance=None)
        finally:
            if self.pose_graph_loss is not None:
                self.ctx.set_pose_graph_loss(*loss_before)
        lids = sorted(l for l in self.landmarks if self.anchor.get(l) in self.poses)
        lm = np.array([self.landmarks[l] for l in lids], np.float64).reshape(-1, 3)
        if res["termination"] != 2:
            index = {id: k for k, id in enumerate(ids)}
            for i, l in enumerate(lids):
                k = index[self.anchor[l]]
                local = quaternion_to_rotation(poses[k, :4]).T @ (lm[i] - poses[k, 4:])
                lm[i] = quaternion_to_rotation(res["poses"][k, :4]) @ local + res["poses"][k, 4:]
                self.landmarks[l] = lm[i].copy()
            for k, id in enumerate(ids):
                self.poses[id] = res["poses"][k].copy()
        res.update(keyframes=ids, poses_before=poses, landmark_ids=np.array(lids, np.int64), landmarks=lm)
        return res


def remove_graph_node(graph, k):
    """node k and its edges leave the covisibility graph (id -> set of ids), and the graph stays as connected as it was:
    every former neighbour of k, in ascending order, that has no path left to the smallest former neighbour gets an edge to
    it (the part ORB-SLAM's spanning-tree re-parenting plays) -> the bridges added, [(neighbour, smallest neighbour), ...]"""
    nbrs = sorted(graph.pop(k, ()))
    for n in nbrs:
        graph[n].discard(k)
    bridges = []
    for n in nbrs[1:]:
        seen, stack = {n}, [n]
        while stack and nbrs[0] not in seen:
            for m in graph[stack.pop()]:
                if m not in seen:
                    seen.add(m)
                    stack.append(m)
        if nbrs[0] not in seen:
            graph[n].add(nbrs[0])
            graph[nbrs[0]].add(n)
            bridges.append((n, nbrs[0]))
    return bridges


class HipKeyframeTracker:
    """The reference front end's loop over frames (RgbdFeatureFrontend::processSensorData, rgbd_feature_frontend.cpp:185-222)
    on the device-resident keyframe store: initFirstKeyframe on the first frame (:433-470: every keypoint with a valid
    depth and z <= z_max, at the identity pose), then per frame one Context.track call against the reference keyframe with
    the previous pose as the guess; the vote's winner becomes the reference (:366-371), a required keyframe is inserted
    and becomes the reference (:373-397); when tracking fails, Context.relocalize over the stored keyframes names the new
    reference (:210-217).  Keyframe ids are 0, 1, ...; the vote list and the relocalisation candidates are the most recent
    64 of them.  Poses are world -> camera (rvec, tvec / R, t).

    local_map_depth = None: track against the reference keyframe's own entry.  local_map_depth = d (the reference: 2): track
    against the local map, as the reference does (getLandmarksWithKeypoints, :256-277).  The tracker keeps the covisibility
    graph on the host (id -> set of ids); after a keyframe is added, Context.kf_covisible of the new entry against the
    members of the local map it was tracked on (part A inherits from their union, so only they can share landmarks with it)
    adds a symmetric edge wherever the count is positive (updateCovisibility, basic_map.cpp:141-164).  The local map is the
    Context.kf_union, under the reserved id LOCAL_MAP_ID, of the reference keyframe's neighbourhood: getNeighbourKeyframes
    (basic_map.cpp:209-237) restated with its `level <= deepLevel` test, which still expands the nodes at level d and so
    reaches d + 1 hops — the reference's behaviour, kept.  A neighbourhood of more than 64 keyframes keeps its 64 largest
    ids (DEVIATES: a union lists at most 64 entries).  The union is enqueued without a synchronisation, only when the
    reference keyframe changed or a keyframe was added, and track runs with ref_id = LOCAL_MAP_ID; the reserved id is never
    in self.ids, the vote list or the relocalisation candidates.  The context's max_keypoints must hold the union; one that
    does not fit raises MslamHipError(E_CAPACITY).

    local_ba = True (needs local_map_depth, for the graph): a HipBackend is fed at every keyframe — the pose from the tracked
    pose, the landmark ids from Context.kf_read_ids, the camera points from entry_kp and Context.backproject — and runs
    local_ba on the new keyframe's neighbourhood (CeresBackend::process, ceres_backend.cpp:92-106); Context.kf_update_world
    then writes the refined points into the store and the refined keyframe poses are kept in self.backend.poses;
    self.ba_results holds every solve's summary.  Off by default: every call computes what it computed before.

    guided_radius = r (> 0): Context.set_guided_match(r, guided_max_distance) with the context's frame size — every track
    call here has a guess, so every one of them matches each landmark within r px of its projection under the previous
    pose (DEVIATES: the reference matches brute force); the relocalisation after a failure has no guess and matches brute
    force.  With process_window the radius has to cover the motion across a window.  None leaves the context's mode alone.

    track_pose = ("align", max_distance): every track / track_window call made here estimates its poses by RANSAC rigid
    alignment of (world point, camera-frame point) with that inlier bound in metres (Context.set_track_pose; DEVIATES: the
    reference estimates by PnP); the setting is applied around each call and the context's own comes back afterwards.  The
    relocalisation after a failure has no depth and runs PnP.  None (the default) leaves the context's setting alone.

    loop_closure = True (needs local_ba and a vocabulary loaded into the context, else MslamHipError(E_INVALID)): the call
    site rgbd_feature_frontend.cpp:198-205, `loopDetector->detectLoop(); closeLoop(candidate)`, with the body the reference
    leaves empty.  At every keyframe, after the covisibility edges and local BA: Context.bow_db_query of the frame's
    descriptors, then bow_db_add (self._bow_entry maps the database's entries to keyframes).  Candidates are the hits with a
    score >= loop_min_score whose keyframe is at least loop_min_gap keyframes older than the new one and not in
    self.neighbours(new_id), and only when the last closure is at least loop_min_gap keyframes back.  Context.relocalize,
    without a guess and with min_inliers = loop_min_inliers, verifies at most loop_max_candidates of them (best score
    first).  On a winner: HipBackend.close_loop, Context.kf_update_world with the moved landmarks, the tracker's pose becomes
    the corrected pose of the new keyframe, the local map is rebuilt, and with loop_global_ba HipBackend.global_ba and
    kf_update_world follow.  self.loop_results holds every attempt; the frame's dict gains loop = (cur, loop) or None.
    pose_graph_solver = "dense" (the default) or "sparse" goes to the backend: close_loop then takes up to 1024 or up to
    16384 keyframes (HipBackend; Context.set_pose_graph_solver).  The optional global solve behind a closure
    (loop_global_ba) has its own setting, whatever pose_graph_solver is: ba_global_solver = "dense" (the default: a cap of
    1024 keyframes, the behaviour it had) or "sparse" (HipBackend(global_linear_solver="sparse"); Context.set_ba_global_solver:
    up to 16384 keyframes, the reduced camera system on its block envelope).  ba_global_pcg = (max_iterations, tolerance) or
    True (needs loop_global_ba, else MslamHipError(E_INVALID)) goes to HipBackend(global_pcg=...): that solve then runs by
    preconditioned conjugate gradients (Context.set_ba_global_pcg), whatever ba_global_solver is.
    pose_graph_pcg = (max_iterations, tolerance) or True (needs loop_closure, else MslamHipError(E_INVALID)) goes to
    HipBackend(pose_graph_pcg=...): close_loop then solves by preconditioned conjugate gradients (Context.set_pose_graph_pcg)
    and takes up to 16384 keyframes, whatever pose_graph_solver is.  On a map that revisits its ground the pose graph has
    the covisibility graph's sparsity, so the pair pose_graph_pcg and ba_global_pcg takes such a map through both solves.
    loop_covariance = True (needs loop_closure, else MslamHipError(E_INVALID); an extension): close_loop runs with
    covariance = True and the attempt's dict in self.loop_results gains covariance = dict(cur, loop, cross), the marginal
    covariances of the two ends of the loop edge at the solved poses (HipBackend.close_loop; Context.pose_graph_covariance).
    With False (the default) nothing new runs and the records are what they were.
    pose_graph_loss = ("huber", a) or ("cauchy", a) (needs loop_closure, else MslamHipError(E_INVALID); an extension) goes to
    the backend too: close_loop solves with that loss on every edge and its dict in self.loop_results gains edge_chi2 and
    edge_weight (HipBackend; Context.set_pose_graph_loss; the context is left with the setting it had).  None (the default)
    is the tracker without the option, bit for bit.  NO REJECTION POLICY is built on the weights: the problem has one loop
    edge on odometry edges measured at the current poses, a chain always bends to such an edge, and so the loop edge's
    weight at the solution does not tell a wrong loop from a right one.  The loss matters to callers of Context.pose_graph
    whose graphs carry several loop edges.
    Without loop_fusion the new keyframe's landmarks keep their own ids, so no covisibility edge joins the two keyframes and
    the loop is known to the pose graph of that one call only.

    loop_fusion = True (needs loop_closure, else MslamHipError(E_INVALID); an extension, the reference has no such step):
    after close_loop and kf_update_world and before the optional global BA, the duplicates across the loop get one
    identity.  Two unions under the reserved ids FUSE_KEEP_ID and FUSE_DROP_ID hold self.neighbours(loop keyframe) (keep)
    and self.neighbours(new keyframe) (drop); Context.kf_fuse with the corrected pose of the new keyframe, the frame's
    extent, loop_fuse_radius, loop_fuse_max_distance, the tracker's ratio and loop_fuse_world_distance rewrites the store;
    the unions are removed; HipBackend.fuse renames the observations; Context.kf_covisible of every member of the new side
    against the old side adds a graph edge wherever the count is positive; the local map is rebuilt.  The attempt's dict
    gains fusion = dict(n_pairs, n_rewritten, edges).  The reserved ids are never in self.ids, the vote list or the
    candidates.  Off (the default): none of this runs and no union is built, so serials and fresh ids are unchanged.

    loop_fusion_keyframes = True (needs loop_fusion, else MslamHipError(E_INVALID); SearchAndFuse's loop over the connected
    keyframes): the fusion step builds the keep union alone and calls Context.kf_fuse_multi with every keyframe of
    self.neighbours(new keyframe) as a target of its own, each under the inverse of its corrected pose
    self.backend.poses[k].  Keyframes that are on the old side as well stay in the list: eligibility is taken over all
    listed entries, which makes them harmless.  One union is built instead of two, so later serials differ from a run
    without the option.  The attempt's fusion dict gains targets.  Off (the default): the fusion step makes exactly the
    calls described above.
    The keep and drop unions are Context.kf_union calls, so they follow the context's union descriptor mode (below).
    STILL OUT: old-side landmarks that no new-side keyframe sees stay unfused.  The descriptors of a fused pair are not
    merged in the store: every keyframe's entry keeps the observation it made.  With union_descriptor = "distinctive" the
    unions built afterwards choose among the observations of both sides, which now share one id; nothing is written back.

    ba_prune = True (needs local_ba, else MslamHipError(E_INVALID)): the consumer of the backend's outlier mask,
    RgbdFeatureFrontend::update(const BackendOutputType&) (rgbd_feature_frontend.cpp:224-230) with the removeObservation
    body the reference leaves commented out (:469-487).  The keyframe's solve is HipBackend.local_ba(prune = True);
    Context.kf_remove_observations then removes pruned["pairs"] from the store (pruned["n_removed"] = the store positions
    removed), kf_update_world writes the final landmarks and the local map is rebuilt, because the entries changed.  With
    loop_global_ba the global solve after a loop is pruned the same way.  ba_results still gets one dict per keyframe, and
    the covisibility graph keeps its edges (the reference's neighbour sets never shrink either).  CAVEAT: without ba_loss
    there is no loss function, so a gross outlier can drag its landmark until the landmark's good observations are flagged
    as well; removal then deletes that landmark everywhere, as the reference's pipeline would.  With ba_loss the outlier's
    weight falls with its residual, the landmark stays with its good observations, and the mask (still judged on the plain
    residual) flags the outlier alone: tests/test_ba_loss.py shows 11 to 26 good observations flagged without a loss and
    none with one on three scenes.  Off by default: nothing is removed.

    ba_loss = ("huber", a) or ("cauchy", a), a in metres (needs local_ba, else MslamHipError(E_INVALID); an extension, the
    reference passes no loss function to Ceres): handed to the backend as HipBackend(loss = ...), so the local solve at
    every keyframe, the pruned second solve of ba_prune and the global solve of loop_global_ba minimise 1/2 sum rho(|r|^2)
    with Ceres's HuberLoss or CauchyLoss (Context.set_ba_loss).  The backend sets the loss for its solve and restores the
    context's setting afterwards.  There is no default scale.  None (the default): no setting is touched and every result
    keeps its bits.  NOT MEASURED: whether the trajectory improves on any sequence.

    kf_cull = True (needs local_ba, else MslamHipError(E_INVALID): the backend holds the observations, the graph the
    neighbours; an extension, the reference has removeKeyframe — basic_map.cpp:110-115, relocalizer.hpp:19 — and no policy
    that calls it; the model is ORB-SLAM's KeyFrameCulling): at every keyframe insertion, last, after the covisibility
    edges, local BA, pruning and the loop closure, Context.kf_cull judges cull_candidates(new_id) — HipBackend.neighbours
    of the new keyframe at depth 1, ascending, never the new keyframe, the reference keyframe, the backend's first keyframe,
    a keyframe the backend does not hold or a reserved id — with self.ids as the map (more than 4096 keyframes:
    MslamHipError(E_CAPACITY) before the context is touched): a candidate goes when more than cull_ratio of its landmarks
    are held by at least cull_min_observers other keyframes, counted without the candidates that went before it.  A culled
    keyframe leaves the store, self.ids, the backend (HipBackend.remove_keyframe), the BoW database (bow_db_remove, and
    self._bow_entry) and the graph; remove_graph_node keeps the graph connected, which the pose graph needs: every former
    neighbour with no path left to the smallest former neighbour gets an edge to it.  The local map is rebuilt.
    self.cull_results gains one dict per call that had candidates: keyframe, listed, candidates, culled, n_landmarks,
    n_redundant, bridges.  Off by default: nothing is removed.  STILL OUT: ORB-SLAM's scale condition (the store keeps no
    octave).

    union_descriptor = "distinctive" (needs local_map_depth, else MslamHipError(E_INVALID); an extension, the reference
    matches against the most recent observation; the model is ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors):
    Context.set_union_descriptor at construction, so every union built on the context from then on — the local map, and
    the keep and drop unions of loop_fusion — carries, for a landmark observed in three or more of the listed keyframes,
    the descriptor with the least median Hamming distance to the landmark's other observations (one per listed keyframe;
    ties: the largest keyframe id) instead of the most recent one.  Rows, order, points, ids and serials are unchanged.
    "recent" sets the reference's rule; None (the default) leaves the context's mode alone.  DEVIATES from ORB-SLAM: one
    observation per listed keyframe, the tie rule, no UpdateNormalAndDepth, no write-back into the keyframes.  NOT
    MEASURED: whether the trajectory improves on any sequence.

    lm_cull = True (needs no other option; an extension, the reference has no such step; the model is ORB-SLAM's
    MapPointCulling, run before KeyFrameCulling as there): at every keyframe insertion, on both paths, after the covisibility
    edges, local BA, pruning and the loop closure and before kf_cull's step.  Part B of every new keyframe gives a fresh id
    to each keypoint it did not match, and most of those are never matched again; nothing else removes them.  The new id
    joins a pending list; the keyframes inserted at least lm_cull_age insertions ago leave it, and those of them still in
    self.ids are the candidates of one Context.kf_cull_landmarks with self.ids as the map (more than 4096 keyframes:
    MslamHipError(E_CAPACITY) before the context is touched; the reserved ids are never listed, so a union neither counts
    as an observer nor changes): a landmark that a candidate holds (fresh or inherited) and that fewer than
    lm_cull_min_observers keyframes hold leaves every keyframe's entry.  With a backend, HipBackend.remove_landmarks
    follows.  The local map is rebuilt when anything was removed.  self.lm_cull_results gains one dict per call made:
    keyframe, listed, candidates, landmark_ids, n_removed, n_backend.  Off by default: nothing is removed.  STILL OUT:
    MapPointCulling's found / visible ratio (the store keeps no such counters).

    dense_map = dict(dims=(nx, ny, nz), voxel=, origin=(x, y, z), trunc=4 voxel, max_depth=3.0, max_frames=1024) (needs no
    other option; an extension, the reference's only dense output is the viewer's per-frame cloud): a TSDF volume on the
    context (Context.tsdf_create, at the first keyframe, with the frame's size and the tracker's intrinsics and depth factor;
    max_depth's default is the reference's zThreshold) that holds exactly the retained keyframes at their current poses.  At
    every keyframe insertion, on both paths, right after the keyframe has its id and before local BA, the keyframe's depth
    image is added under the keyframe id at the tracked pose (keyframe 0: the identity).  After every step that changes
    self.backend.poses — local BA, close_loop, global BA — one Context.tsdf_update_poses lists the keyframes whose back-end
    pose (camera -> world, inverted to the library's world -> camera) differs from the pose they are integrated at by more
    than dense_update = (translation in metres, between the two camera centres; angle in radians, of the relative rotation):
    each is taken out at the old pose and put back at the new one.  The defaults are voxel / 2 and voxel / (2 max_depth),
    half a voxel at the far end of the range (an infinite max_depth: 0).  NOT MEASURED: whether these defaults are good on any
    sequence.  A keyframe kf_cull removes leaves the volume too.  self.dense_poses maps keyframe id -> (R, t) it is
    integrated at; self.dense_results gains one dict per update call: listed, moved.  Without local_ba the poses never move
    and nothing is re-integrated.  None (the default): nothing new runs.

    dense_icp = dict(levels, dist_max, cos_min, min_pairs, max_rms) (every key optional; needs dense_map; an extension):
    frame-to-model alignment where features fail.  When a frame is not tracked and the volume exists, Context.tsdf_icp aligns
    the frame's depth image to the volume's render at the current pose, from the current pose.  The result is accepted when
    its status is not DEGENERATE and sqrt(cost / count), the RMS point-to-plane residual in metres, is <= max_rms (default:
    one voxel edge; NOT MEASURED on any real sequence): self.R, self.tvec and self.rvec become that pose and the frame's dict
    gains dense_tracked=True; either way the result is reported under `dense` and relocalisation runs as before.  `tracked`
    stays False: the keyframe policy, the store and the back end never see an ICP pose.  A frame that tracks is untouched, so
    a run in which every frame tracks is the same with and without the option.  None (the default): nothing new runs."""

    LOCAL_MAP_ID = 0x7fffffff
    FUSE_KEEP_ID, FUSE_DROP_ID = 0x7ffffffe, 0x7ffffffd
    LOOP_QUERY_RESULTS = 64    # hits asked of the database before the filters: the newest keyframes fill the top of the list

    def __init__(self, ctx, focal=(525.0, 525.0), principal=(319.5, 239.5), factor=1.0 / 5000.0, ratio=0.7, iterations=100,
                 reprojection_error=5.0, seed=0, min_matched_points=10, new_keyframe_min_landmarks=30, z_max=3.0,
                 reloc_min_inliers=60, local_map_depth=None, guided_radius=None, guided_max_distance=256, local_ba=False,
                 loop_closure=False, loop_min_score=0.05, loop_min_gap=10, loop_min_inliers=60, loop_max_candidates=4,
                 loop_global_ba=False, loop_fusion=False, loop_fuse_radius=8.0, loop_fuse_max_distance=50,
                 loop_fuse_world_distance=0.1, ba_prune=False, kf_cull=False, cull_min_observers=3, cull_ratio=0.9, lm_cull=False,
                 lm_cull_min_observers=2, lm_cull_age=2, ba_loss=None, loop_fusion_keyframes=False, union_descriptor=None,
                 pose_graph_solver="dense", ba_global_solver="dense", pose_graph_loss=None, loop_covariance=False,
                 ba_global_pcg=None, pose_graph_pcg=None, track_pose=None, dense_map=None, dense_update=None, dense_icp=None):
        self.ctx = ctx
        self.dense_map, self.dense_update, self.dense_poses, self.dense_results = None, None, {}, []
        if dense_map is not None:
            unknown = set(dense_map) - {"dims", "voxel", "origin", "trunc", "max_depth", "max_frames"}
            if unknown or not {"dims", "voxel", "origin"} <= set(dense_map):
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: dense_map is dict(dims, voxel, origin[, trunc, max_depth, "
                                               "max_frames])")
            self.dense_map = dict(dense_map)
            self.dense_map.setdefault("max_depth", 3.0)
            voxel, far = float(self.dense_map["voxel"]), float(self.dense_map["max_depth"])
            self.dense_update = (voxel / 2, voxel / (2 * far)) if dense_update is None else (float(dense_update[0]), float(dense_update[1]))
        elif dense_update is not None:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: dense_update needs dense_map")
        self._dense_created = False
        self.dense_icp = None
        if dense_icp is not None:
            if self.dense_map is None:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: dense_icp needs dense_map")
            if set(dense_icp) - {"levels", "dist_max", "cos_min", "min_pairs", "max_rms"}:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: dense_icp is dict([levels, dist_max, cos_min, min_pairs, max_rms])")
            self.dense_icp = dict(dense_icp)
            self.dense_icp.setdefault("max_rms", float(self.dense_map["voxel"]))
        if track_pose is not None:
            if len(track_pose) != 2 or track_pose[0] not in _TRACK_POSE_NAMES:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: track_pose is None or (\"pnp\" / \"align\", max_distance)")
            if track_pose[0] == "align" and not float(track_pose[1]) > 0:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: track_pose align needs max_distance > 0")
        self.track_pose = None if track_pose is None else (track_pose[0], float(track_pose[1]))
        if _pcg_setting(pose_graph_pcg, "HipKeyframeTracker", "pose_graph_pcg") is not None and not loop_closure:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: pose_graph_pcg needs loop_closure (close_loop takes the setting)")
        if _pcg_setting(ba_global_pcg, "HipKeyframeTracker") is not None and not (loop_closure and loop_global_ba):
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: ba_global_pcg needs loop_closure and loop_global_ba")
        if loop_covariance and not loop_closure:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: loop_covariance needs loop_closure (close_loop computes it)")
        self.loop_covariance = bool(loop_covariance)
        if union_descriptor is not None:
            if local_map_depth is None:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: union_descriptor needs local_map_depth (the union it applies to)")
            if union_descriptor not in _UNION_DESC_NAMES and union_descriptor not in _UNION_DESC_NAMES.values():
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: union_descriptor %r is not recent / distinctive" % (union_descriptor,))
        if ba_loss is not None and not local_ba:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: ba_loss needs local_ba (the backend's solves take the loss)")
        self.ba_loss = None if ba_loss is None else (ba_loss[0], float(ba_loss[1]))
        if pose_graph_loss is not None and not loop_closure:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: pose_graph_loss needs loop_closure (close_loop takes the loss)")
        self.pose_graph_loss = None if pose_graph_loss is None else (pose_graph_loss[0], float(pose_graph_loss[1]))
        self.lm_cull, self.lm_cull_min_observers, self.lm_cull_age = bool(lm_cull), int(lm_cull_min_observers), int(lm_cull_age)
        self.lm_cull_results = []
        self._lm_pending = []        # (keyframe id, the insertion count at which it was inserted): not judged yet
        self._lm_inserted = 0        # keyframe insertions seen by _lm_cull
        if kf_cull and not local_ba:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: kf_cull needs local_ba (the backend holds the observations, "
                                           "the graph the neighbours)")
        self.kf_cull, self.cull_min_observers, self.cull_ratio = bool(kf_cull), int(cull_min_observers), float(cull_ratio)
        self.cull_results = []
        if ba_prune and not local_ba:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: ba_prune needs local_ba (the backend finds the outliers)")
        self.ba_prune = bool(ba_prune)
        if loop_fusion and not loop_closure:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: loop_fusion needs loop_closure")
        if loop_fusion_keyframes and not loop_fusion:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: loop_fusion_keyframes needs loop_fusion")
        self.loop_fusion_keyframes = bool(loop_fusion_keyframes)
        self.loop_fusion, self.loop_fuse_radius = bool(loop_fusion), float(loop_fuse_radius)
        self.loop_fuse_max_distance, self.loop_fuse_world_distance = int(loop_fuse_max_distance), float(loop_fuse_world_distance)
        self._extent = None          # (width, height) of the last frame's depth image: the frame loop_fusion projects into
        if local_ba and local_map_depth is None:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker: local_ba needs local_map_depth (the covisibility graph)")
        if loop_closure:
            if not local_ba:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: loop_closure needs local_ba (the backend holds the poses)")
            try:
                ctx.bow_info()
            except MslamHipError:
                raise MslamHipError(E_INVALID, "HipKeyframeTracker: loop_closure needs a vocabulary (Context.bow_load)")
        self.loop_closure, self.loop_min_score, self.loop_min_gap = bool(loop_closure), float(loop_min_score), int(loop_min_gap)
        self.loop_min_inliers, self.loop_max_candidates = int(loop_min_inliers), int(loop_max_candidates)
        self.loop_global_ba = bool(loop_global_ba)
        self.loop_results = []
        self._bow_entry = {}         # BoW database entry -> keyframe id
        self._last_closure = None    # the keyframe at which the last loop was closed
        # with loop_global_ba the backend's global solve is the one without the 64-keyframe cap
        self.backend = HipBackend(ctx, global_solver=bool(loop_closure and loop_global_ba), loss=self.ba_loss,
                                  pose_graph_solver=pose_graph_solver, global_linear_solver=ba_global_solver,
                                  pose_graph_loss=self.pose_graph_loss, global_pcg=ba_global_pcg,
                                  pose_graph_pcg=pose_graph_pcg) if local_ba else None
        self.ba_results = []
        if guided_radius is not None:
            ctx.set_guided_match(guided_radius, guided_max_distance)
        if union_descriptor is not None:
            ctx.set_union_descriptor(union_descriptor)
        self.local_map_depth = local_map_depth
        self.graph = {}            # covisibility: id -> set of ids
        self.local_map = []        # the entries the current union lists
        self._local_map_of = None  # the reference keyframe the current union was built for (None: rebuild)
        self.focal, self.principal, self.factor = tuple(focal), tuple(principal), factor
        self.ratio, self.iterations, self.reprojection_error, self.seed = ratio, iterations, reprojection_error, seed
        self.min_matched_points, self.new_keyframe_min_landmarks = min_matched_points, new_keyframe_min_landmarks
        self.z_max, self.reloc_min_inliers = z_max, reloc_min_inliers
        self.ids = []
        self.reference = None
        self.rvec, self.tvec, self.R = np.zeros(3), np.zeros(3), np.eye(3)
        self.frame = 0
        self.window_calls = self.window_computed = self.window_discarded = 0   # process_window's counters

    @contextlib.contextmanager
    def _track_pose_scope(self):
        """the tracker's track_pose around one of its own tracking calls; the context's setting comes back afterwards, as
        close_loop does with the solver settings.  None: the context's setting is left alone."""
        if self.track_pose is None:
            yield
            return
        before = self.ctx.get_track_pose()
        self.ctx.set_track_pose(*self.track_pose)
        try:
            yield
        finally:
            self.ctx.set_track_pose(*before)

    def processSensorData(self, desc, xy, depth):
        """one frame: descriptors [n, 32], keypoint coordinates [n, 2], depth image [h, w] u16
        -> dict(tracked, n_inliers, rvec, tvec, R, reference, keyframe = the id added or -1, relocalized, step)"""
        seed = self.seed + self.frame
        self.frame += 1
        self._extent = np.asarray(depth).shape[1::-1]
        if self.reference is None:
            xyz, valid = self.ctx.backproject(depth, xy, self.factor, self.focal, self.principal)
            keep = valid & (xyz[:, 2] <= self.z_max)
            self.ctx.kf_add(0, np.asarray(desc, np.uint8).reshape(-1, 32)[keep], xyz[keep])   # identity pose: world = camera point
            if self.backend is not None:
                self.backend.add_keyframe(0, (0, 0, 0, 1, 0, 0, 0), self.ctx.kf_read_ids(0), xyz[keep])
            self.ids, self.reference = [0], 0
            self.graph = {0: set()}
            if self.dense_map is not None:
                self._dense_add(0, depth, np.eye(3), np.zeros(3))
            first = dict(tracked=True, n_inliers=0, rvec=self.rvec.copy(), tvec=self.tvec.copy(), R=self.R.copy(), reference=0,
                         keyframe=0, relocalized=False, step=None)
            if self.loop_closure:
                first["loop"] = self._close_loops(0, desc, xy, seed)
            if self.lm_cull:
                self._lm_cull(0)   # (the first insertion: keyframe 0 joins the pending list, nothing is due yet)
            return first
        vote = self.ids[-64:]
        new_id = self.ids[-1] + 1
        ref_id, rebuilt = self.reference, False
        if self.local_map_depth is not None:
            if self._local_map_of != self.reference:
                self.local_map = self.neighbours(self.reference)
                self.ctx.kf_union(self.LOCAL_MAP_ID, self.local_map, sync=False)   # track's own synchronisation covers it
                self._local_map_of, rebuilt = self.reference, True
            ref_id = self.LOCAL_MAP_ID
        with self._track_pose_scope():
            res = self.ctx.track(desc, xy, depth, ref_id, vote, new_id, self.factor, self.focal, self.principal, self.ratio,
                                 self.iterations, self.reprojection_error, seed, self.rvec, self.tvec, self.min_matched_points,
                                 self.new_keyframe_min_landmarks, self.z_max, with_entry=True)
        if rebuilt:
            self.ctx.sync()   # a union that did not fit max_keypoints left an empty entry: it surfaces here as E_CAPACITY
        out = dict(tracked=bool(res["tracked"]), n_inliers=res["n_inliers"], keyframe=-1, relocalized=False, step=res)
        if res["tracked"]:
            self.rvec, self.tvec, self.R = res["rvec"], res["tvec"], res["R"]
            if res["vote_best"] >= 0:
                self.reference = vote[res["vote_best"]]
            if res["keyframe_added"]:
                self.ids.append(new_id)
                self.reference = out["keyframe"] = new_id
                if self.dense_map is not None:
                    self._dense_add(new_id, depth, res["R"], res["tvec"])
                if self.local_map_depth is not None:
                    self.graph[new_id] = set()
                    for other, n in zip(self.local_map, self.ctx.kf_covisible(new_id, self.local_map)):
                        if n > 0 and other != new_id:
                            self.graph[new_id].add(other)
                            self.graph[other].add(new_id)
                    self._local_map_of = None   # a keyframe was added: the local map is rebuilt
                    if self.backend is not None:
                        self._local_ba(new_id, res, xy, depth)
                    if self.loop_closure:
                        out["loop"] = self._close_loops(new_id, desc, xy, seed)
                if self.lm_cull:
                    self._lm_cull(new_id)
                if self.kf_cull:
                    self._cull(new_id)
        else:
            self._dense_track(depth, out)
            reloc = self.ctx.relocalize(desc, xy, vote, self.focal, self.principal, None, self.ratio, self.iterations,
                                        self.reprojection_error, seed, min_inliers=self.reloc_min_inliers)
            if reloc["best"] >= 0:
                self.reference, out["relocalized"] = vote[reloc["best"]], True
        if self.loop_closure:
            out.setdefault("loop", None)
        out.update(rvec=self.rvec.copy(), tvec=self.tvec.copy(), R=self.R.copy(), reference=self.reference)
        return out

    def process_window(self, descs, xys, depths, window=16):
        """processSensorData over a list of frames, `window` frames per Context.track_window call: the guess is the current
        pose and the seed self.seed + the absolute frame index; the frames up to and including the call's first event are
        accepted, the event is handled exactly as processSensorData handles it (a keyframe: the id is appended and, in
        local-map mode, the covisibility edges are added and the union is rebuilt; a vote: the reference switches; a
        failure: relocalize), and the loop continues behind the event frame.  -> the per-frame dicts of processSensorData.
        DEVIATES from the frame-by-frame loop: the frames of one window share the guess of the window's start (the guess
        only starts PnP's final refit: the consensus sets are the same).  window = 1 is processSensorData.
        self.window_calls / window_computed / window_discarded count the calls, the frames they computed and the frames
        computed behind an event and thrown away."""
        out, i, N = [], 0, len(descs)
        while i < N:
            if self.reference is None:
                out.append(self.processSensorData(descs[i], xys[i], depths[i]))
                i += 1
                continue
            vote = self.ids[-64:]
            new_id = self.ids[-1] + 1
            pos = vote.index(self.reference) if self.reference in vote else -1
            S = min(int(window), N - i, 256) if pos >= 0 else 1   # a reference outside the vote list: frame by frame
            seed = self.seed + self.frame
            ref_id, rebuilt = self.reference, False
            if self.local_map_depth is not None:
                if self._local_map_of != self.reference:
                    self.local_map = self.neighbours(self.reference)
                    self.ctx.kf_union(self.LOCAL_MAP_ID, self.local_map, sync=False)   # the call's own synchronisation covers it
                    self._local_map_of, rebuilt = self.reference, True
                ref_id = self.LOCAL_MAP_ID
            with self._track_pose_scope():
                recs, first = self.ctx.track_window(descs[i:i + S], xys[i:i + S], depths[i:i + S], ref_id, vote, new_id, pos,
                                                    self.factor, self.focal, self.principal, self.ratio, self.iterations,
                                                    self.reprojection_error, seed, self.rvec, self.tvec, self.min_matched_points,
                                                    self.new_keyframe_min_landmarks, self.z_max, with_entry=True)
            if rebuilt:
                self.ctx.sync()   # a union that did not fit max_keypoints left an empty entry: it surfaces here as E_CAPACITY
            n_acc = min(first + 1, S)
            self.window_calls += 1
            self.window_computed += S
            self.window_discarded += S - n_acc
            for s in range(n_acc):
                res = recs[s]
                o = dict(tracked=bool(res["tracked"]), n_inliers=res["n_inliers"], keyframe=-1, relocalized=False, step=res)
                if res["tracked"]:
                    self.rvec, self.tvec, self.R = res["rvec"], res["tvec"], res["R"]
                    if res["vote_best"] >= 0:
                        self.reference = vote[res["vote_best"]]
                    if res["keyframe_added"]:
                        self._keyframe_added(new_id)
                        o["keyframe"] = new_id
                        if self.dense_map is not None:
                            self._dense_add(new_id, depths[i + s], res["R"], res["tvec"])
                        if self.backend is not None:
                            self._local_ba(new_id, res, xys[i + s], depths[i + s])
                        if self.loop_closure:
                            self._extent = np.asarray(depths[i + s]).shape[1::-1]
                            o["loop"] = self._close_loops(new_id, descs[i + s], xys[i + s], seed + s)
                        if self.lm_cull:
                            self._lm_cull(new_id)
                        if self.kf_cull:
                            self._cull(new_id)
                else:
                    self._dense_track(depths[i + s], o)
                    reloc = self.ctx.relocalize(descs[i + s], xys[i + s], vote, self.focal, self.principal, None, self.ratio,
                                                self.iterations, self.reprojection_error, seed + s,
                                                min_inliers=self.reloc_min_inliers)
                    if reloc["best"] >= 0:
                        self.reference, o["relocalized"] = vote[reloc["best"]], True
                if self.loop_closure:
                    o.setdefault("loop", None)
                o.update(rvec=self.rvec.copy(), tvec=self.tvec.copy(), R=self.R.copy(), reference=self.reference)
                out.append(o)
            self.frame += n_acc
            i += n_acc
        return out

    def _keyframe_added(self, new_id):
        """the bookkeeping behind a keyframe track_window built (processSensorData's, restated): the id, the reference, and
        in local-map mode the covisibility edges and the rebuild of the union"""
        self.ids.append(new_id)
        self.reference = new_id
        if self.local_map_depth is not None:
            self.graph[new_id] = set()
            for other, n in zip(self.local_map, self.ctx.kf_covisible(new_id, self.local_map)):
                if n > 0 and other != new_id:
                    self.graph[new_id].add(other)
                    self.graph[other].add(new_id)
            self._local_map_of = None

    def _dense_add(self, kf_id, depth, R, t):
        """dense_map: the keyframe's depth image joins the volume under the keyframe id at its world -> camera pose; the
        volume is created at the first keyframe, with that frame's size"""
        depth = np.ascontiguousarray(depth, np.uint16)
        if not self._dense_created:
            m = self.dense_map
            self.ctx.tsdf_create(m["dims"], m["voxel"], m["origin"], m.get("trunc"), m["max_depth"], m.get("max_frames", 1024),
                                 depth.shape[1], depth.shape[0], self.factor, self.focal, self.principal)
            self._dense_created = True
        R, t = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
        self.ctx.tsdf_add_frame(kf_id, depth, R, t)
        self.dense_poses[kf_id] = (R, t)

    def dense_render(self, R=None, t=None, **kw):
        """dense_map: Context.tsdf_raycast of the volume at the world -> camera pose (R, t), by default the pose of the latest
        tracked frame; the keywords are tsdf_raycast's.  Reads the volume only: tracking is not affected."""
        if self.dense_map is None or not self._dense_created:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker.dense_render needs dense_map and a first keyframe")
        if (R is None) != (t is None):
            raise MslamHipError(E_INVALID, "HipKeyframeTracker.dense_render: R and t go together")
        if R is None:
            R, t = self.R, self.tvec
        return self.ctx.tsdf_raycast(R, t, **kw)

    def dense_align(self, depth, R=None, t=None, **kw):
        """dense_map: Context.tsdf_icp of a depth image (u16 [h][w] of the volume's camera) against the volume's render at the
        world -> camera guess (R, t), by default the pose of the latest tracked frame; the keywords are tsdf_icp's.  Reads
        the volume only and changes no state of the tracker."""
        if self.dense_map is None or not self._dense_created:
            raise MslamHipError(E_INVALID, "HipKeyframeTracker.dense_align needs dense_map and a first keyframe")
        if (R is None) != (t is None):
            raise MslamHipError(E_INVALID, "HipKeyframeTracker.dense_align: R and t go together")
        if R is None:
            R, t = self.R, self.tvec
        return self.ctx.tsdf_icp(depth, R, t, **kw)

    def _dense_track(self, depth, out):
        """dense_icp, for a frame that was not tracked: the frame-to-model pose takes the place of the kept one when it is
        accepted; `out` gains dense and dense_tracked"""
        if self.dense_icp is None or not self._dense_created:
            return
        kw = {k: v for k, v in self.dense_icp.items() if k != "max_rms"}
        res = self.ctx.tsdf_icp(depth, self.R, self.tvec, **kw)
        ok = res["status"] != ICP_DEGENERATE and res["count"] > 0 and math.sqrt(res["cost"] / res["count"]) <= self.dense_icp["max_rms"]
        if ok:
            self.R, self.tvec = res["R"], res["t"]
            self.rvec = rotation_to_rvec(self.R)
        out["dense"], out["dense_tracked"] = res, bool(ok)

    @staticmethod
    def dense_pose_change(R0, t0, R1, t1):
        """-> (metres between the camera centres, radians of the relative rotation) of two world -> camera poses"""
        dc = R1.T @ t1 - R0.T @ t0
        cos = (np.trace(R1 @ R0.T) - 1.0) / 2.0
        return float(np.sqrt(dc @ dc)), float(np.arccos(min(1.0, max(-1.0, cos))))

    def _dense_follow(self):
        """dense_map, after a step that changed self.backend.poses: one Context.tsdf_update_poses with the keyframes whose
        back-end pose left the pose they are integrated at by more than self.dense_update"""
        ids, Rs, ts = [], [], []
        for k in sorted(self.dense_poses):
            pose = self.backend.poses.get(k)
            if pose is None:
                continue
            R = quaternion_to_rotation(pose[:4]).T              # camera -> world in the backend; the volume takes world -> camera
            t = -R @ np.asarray(pose[4:], np.float64)
            d, a = self.dense_pose_change(*self.dense_poses[k], R, t)
            if d > self.dense_update[0] or a > self.dense_update[1]:
                ids.append(k)
                Rs.append(R)
                ts.append(t)
        moved = self.ctx.tsdf_update_poses(ids, np.stack(Rs), np.stack(ts)) if ids else 0
        for k, R, t in zip(ids, Rs, ts):
            self.dense_poses[k] = (np.ascontiguousarray(R, np.float64), np.ascontiguousarray(t, np.float64))
        self.dense_results.append(dict(listed=ids, moved=moved))

    def _local_ba(self, new_id, res, xy, depth):
        """CeresBackend::process for the keyframe just added: feed the backend, solve, write the refined points back"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        cam, ok = self.ctx.backproject(depth, xy[res["entry_kp"]], self.factor, self.focal, self.principal)
        R = np.asarray(res["R"], np.float64).reshape(3, 3)      # world -> camera; the keyframe's state is camera -> world
        pose = np.concatenate([rotation_to_quaternion(R.T), -R.T @ np.asarray(res["tvec"], np.float64)])
        self.backend.add_keyframe(new_id, pose, self.ctx.kf_read_ids(new_id)[ok], cam[ok])   # (an entry's keypoints have a depth)
        ba = self.backend.local_ba(new_id, self.graph, prune=True) if self.ba_prune else self.backend.local_ba(new_id, self.graph)
        self._prune_store(ba)
        if ba["termination"] != 2:
            ba["n_written"] = self.ctx.kf_update_world(ba["landmark_ids"], ba["landmarks"])
        self.ba_results.append(ba)
        if self.dense_map is not None:
            self._dense_follow()

    def _prune_store(self, ba):
        """ba_prune: the observations a pruned solve removed from the backend leave the store too, and the union is rebuilt"""
        pruned = ba.get("pruned")
        if pruned is None:
            return
        pairs = pruned["pairs"]
        pruned["n_removed"] = self.ctx.kf_remove_observations([k for k, _ in pairs], [l for _, l in pairs])["n_removed"] if pairs else 0
        if pairs:
            self._local_map_of = None

    def _lm_cull(self, new_id):
        """lm_cull: the new keyframe joins the pending list; the keyframes inserted at least lm_cull_age insertions ago
        leave it, and those of them still in self.ids are the candidates of one Context.kf_cull_landmarks with self.ids
        as the map; the backend forgets the culled landmarks.  A call made is recorded in self.lm_cull_results"""
        self._lm_inserted += 1
        self._lm_pending.append((new_id, self._lm_inserted))
        due = [k for k, at in self._lm_pending if self._lm_inserted - at >= self.lm_cull_age]
        self._lm_pending = [(k, at) for k, at in self._lm_pending if self._lm_inserted - at < self.lm_cull_age]
        held = set(self.ids)
        cands = [k for k in due if k in held]
        if not cands:
            return
        if len(self.ids) > CULL_MAX_ENTRIES:
            raise MslamHipError(E_CAPACITY, "lm_cull: %d keyframes, at most %d per call" % (len(self.ids), CULL_MAX_ENTRIES))
        listed = list(self.ids)
        res = self.ctx.kf_cull_landmarks(listed, cands, self.lm_cull_min_observers)
        n_backend = self.backend.remove_landmarks(res["landmark_ids"])["n_observations"] if self.backend is not None else 0
        if res["n_removed"] > 0:
            self._local_map_of = None
        self.lm_cull_results.append(dict(keyframe=new_id, listed=listed, candidates=cands, landmark_ids=res["landmark_ids"],
                                         n_removed=res["n_removed"], n_backend=n_backend))

    def cull_candidates(self, new_id):
        """the keyframes _cull may remove when new_id was inserted: HipBackend.neighbours(new_id, graph, 1), ascending,
        without new_id, the reference keyframe and the backend's first keyframe (the gauge); a keyframe the backend or
        self.ids does not hold (the reserved ids among them) is never one"""
        keep, listed = {new_id, self.reference, self.backend.first}, set(self.ids)
        return [k for k in self.backend.neighbours(new_id, self.graph, 1) if k not in keep and k in listed]

    def _cull(self, new_id):
        """kf_cull: Context.kf_cull over cull_candidates(new_id) with self.ids as the map, then the bookkeeping behind
        every culled keyframe (ids, backend, BoW database, graph with its bridges); a call that had candidates is recorded
        in self.cull_results"""
        if len(self.ids) > CULL_MAX_ENTRIES:
            raise MslamHipError(E_CAPACITY, "kf_cull: %d keyframes, at most %d per call" % (len(self.ids), CULL_MAX_ENTRIES))
        cands = self.cull_candidates(new_id)
        if not cands:
            return
        listed = list(self.ids)
        res = self.ctx.kf_cull(listed, cands, self.cull_min_observers, self.cull_ratio)
        gone = [k for k, c in zip(cands, res["culled"]) if c]
        bridges = []
        for k in gone:
            self.ids.remove(k)
            self.backend.remove_keyframe(k)
            if k in self.dense_poses:
                self.ctx.tsdf_remove_frame(k)
                del self.dense_poses[k]
            for entry in [e for e, kf in self._bow_entry.items() if kf == k]:
                self.ctx.bow_db_remove(entry)
                del self._bow_entry[entry]
            bridges += remove_graph_node(self.graph, k)
        if gone:
            self._local_map_of = None
        self.cull_results.append(dict(keyframe=new_id, listed=listed, candidates=cands, culled=gone,
                                      n_landmarks=res["n_landmarks"].tolist(), n_redundant=res["n_redundant"].tolist(),
                                      bridges=bridges))

    def loop_candidates(self, new_id, entries, scores):
        """the filters between the database's hits and the verification -> keyframe ids, best score first, at most
        loop_max_candidates: score >= loop_min_score; at least loop_min_gap keyframes older than new_id; not in
        self.neighbours(new_id); none at all while the last closure is fewer than loop_min_gap keyframes back"""
        if self._last_closure is not None and new_id - self._last_closure < self.loop_min_gap:
            return []
        near = set(self.neighbours(new_id))
        hits = sorted(((float(s), self._bow_entry[int(e)]) for e, s in zip(entries, scores) if int(e) in self._bow_entry),
                      key=lambda h: (-h[0], h[1]))
        return [k for s, k in hits if s >= self.loop_min_score and new_id - k >= self.loop_min_gap and k not in near][:self.loop_max_candidates]

    def _close_loops(self, new_id, desc, xy, seed):
        """detectLoop and closeLoop for the keyframe just added -> (new_id, loop keyframe) or None.  An attempt (a verification
        that ran) is appended to self.loop_results: keyframe, candidates, inliers, loop = the verified keyframe or None, and
        for a verified one the PnP pose, close_loop's result (termination 2: nothing was corrected) and global_ba's"""
        entries, scores = self.ctx.bow_db_query(desc, max_results=self.LOOP_QUERY_RESULTS)
        self._bow_entry[self.ctx.bow_db_add(desc)] = new_id
        cands = self.loop_candidates(new_id, entries, scores)
        if not cands:
            return None
        reloc = self.ctx.relocalize(desc, xy, cands, self.focal, self.principal, None, self.ratio, self.iterations,
                                    self.reprojection_error, seed, min_inliers=self.loop_min_inliers)
        attempt = dict(keyframe=new_id, candidates=list(cands), inliers=[c["n_inliers"] for c in reloc["candidates"]], loop=None)
        self.loop_results.append(attempt)
        if reloc["best"] < 0:
            return None
        loop_id, win = cands[reloc["best"]], reloc["candidates"][reloc["best"]]
        if self.loop_covariance:
            res = self.backend.close_loop(new_id, loop_id, win["rvec"], win["tvec"], self.graph, covariance=True)
            attempt.update(covariance=res.get("covariance"))
        else:
            res = self.backend.close_loop(new_id, loop_id, win["rvec"], win["tvec"], self.graph)
        attempt.update(loop=loop_id, rvec=win["rvec"], tvec=win["tvec"], result=res)
        if res["termination"] == 2:
            return None
        res["n_written"] = self.ctx.kf_update_world(res["landmark_ids"], res["landmarks"])
        pose = self.backend.poses[new_id]                   # camera -> world; the tracker's pose is world -> camera
        self.R = quaternion_to_rotation(pose[:4]).T
        self.tvec = -self.R @ pose[4:]
        self.rvec = rotation_to_rvec(self.R)
        self._local_map_of = None
        self._last_closure = new_id
        if self.dense_map is not None:
            self._dense_follow()
        if self.loop_fusion:
            attempt["fusion"] = self._fuse_loop(new_id, loop_id)
        if self.loop_global_ba:
            ba = self.backend.global_ba(prune=True) if self.ba_prune else self.backend.global_ba()
            self._prune_store(ba)
            if ba["termination"] != 2:
                ba["n_written"] = self.ctx.kf_update_world(ba["landmark_ids"], ba["landmarks"])
            attempt["global_ba"] = ba
            if self.dense_map is not None:
                self._dense_follow()
        return (new_id, loop_id)

    def _fuse_loop(self, new_id, loop_id):
        """landmark fusion across the loop just closed: the new side's duplicates take the old side's ids and points
        -> dict(n_pairs, n_rewritten, edges = the (new side, old side) graph edges the shared landmarks add)"""
        old, new = self.neighbours(loop_id), self.neighbours(new_id)
        self.ctx.kf_union(self.FUSE_KEEP_ID, old)
        try:
            if self.loop_fusion_keyframes:
                # every keyframe of the new side is a target under its own corrected pose (camera -> world in the backend)
                Rs = [quaternion_to_rotation(self.backend.poses[k][:4]).T for k in new]
                ts = [-R @ self.backend.poses[k][4:] for R, k in zip(Rs, new)]
                got = self.ctx.kf_fuse_multi(self.FUSE_KEEP_ID, new, np.stack(Rs), np.stack(ts), self.loop_fuse_radius,
                                             self.loop_fuse_max_distance, self.ratio, self.loop_fuse_world_distance, self.focal,
                                             self.principal, self._extent[0], self._extent[1])
            else:
                self.ctx.kf_union(self.FUSE_DROP_ID, new)
                try:
                    got = self.ctx.kf_fuse(self.FUSE_KEEP_ID, self.FUSE_DROP_ID, self.R, self.tvec, self.loop_fuse_radius,
                                           self.loop_fuse_max_distance, self.ratio, self.loop_fuse_world_distance, self.focal,
                                           self.principal, self._extent[0], self._extent[1])
                finally:
                    self.ctx.kf_remove(self.FUSE_DROP_ID)
        finally:
            self.ctx.kf_remove(self.FUSE_KEEP_ID)
        self.backend.fuse(got["keep_lid"], got["drop_lid"])
        edges = []
        for k in new:
            for other, n in zip(old, self.ctx.kf_covisible(k, old)):
                if n > 0 and other != k and other not in self.graph[k]:
                    self.graph[k].add(other)
                    self.graph[other].add(k)
                    edges.append((k, other))
        self._local_map_of = None
        out = dict(n_pairs=len(got["keep_lid"]), n_rewritten=got["n_rewritten"], edges=edges)
        if self.loop_fusion_keyframes:
            out["targets"] = list(new)
        return out

    def neighbours(self, ref):
        """getNeighbourKeyframes (basic_map.cpp:209-237) on self.graph with deepLevel = local_map_depth, ascending; more than
        64: the 64 largest ids"""
        result, queue = set(), [(ref, 0)]
        while queue:
            cur, level = queue.pop(0)
            result.add(cur)
            if level <= self.local_map_depth:
                queue.extend((nb, level + 1) for nb in sorted(self.graph.get(cur, ())) if nb not in result)
        return sorted(result)[-64:]


# ---- harness helper (bench / tests): copy a context-owned device array to the host ------------------
def read_device(ctx, ptr, shape, dtype):
    """Copy a device array (raw pointer from a *_view struct) into a new numpy array."""
    out = np.empty(shape, dtype)
    if out.nbytes:
        ctx._chk(ctx.L.mslam_hip_copy_to_host(ctx._h, _p(out), C.c_void_p(ptr), C.c_size_t(out.nbytes)))
    return out
