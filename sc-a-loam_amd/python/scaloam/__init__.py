"""ctypes binding of libscaloam_hip.so (include/scaloam_hip.h) for tests, bench.py and Python callers.

This is plumbing only: every function forwards to the C-ABI; there is no Python or CPU implementation
behind it, and loading fails loudly when the HIP library has not been built.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCALOAM_LIB: another build of the same library (A/B measurements of two builds on one GPU box); never a different implementation
LIB_PATH = os.environ.get("SCALOAM_LIB") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libscaloam_hip.so"))

VLP16, HDL32, HDL64, OS1_64 = 0, 1, 2, 3
SCAN_LINES = {VLP16: 16, HDL32: 32, HDL64: 64, OS1_64: 64}

OK, E_ARG, E_LIDAR_TYPE, E_SCAN_LINE, E_TOO_MANY, E_EMPTY, E_HIP, E_NO_DEVICE, E_CAPACITY, E_STATE = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9

_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int)


class ScalError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"scaloam_hip error {code}: {msg}")
        self.code = code


class FeaturesConfig(C.Structure):
    _fields_ = [("lidar_type", C.c_int), ("n_scans", C.c_int), ("minimum_range", C.c_double), ("max_points", C.c_int),
                ("float_math", C.c_int), ("check_finite", C.c_int), ("device", C.c_int)]


class FeaturesOut(C.Structure):
    _fields_ = [("cloud", _f32p), ("src_index", _i32p), ("curvature", _f32p), ("label", _i32p), ("ring_start", _i32p),
                ("ring_end", _i32p), ("sharp", _i32p), ("less_sharp", _i32p), ("flat", _i32p), ("less_flat", _f32p),
                ("n_kept", C.c_int), ("n_sharp", C.c_int), ("n_less_sharp", C.c_int), ("n_flat", C.c_int),
                ("n_less_flat", C.c_int), ("n_tied_segments", C.c_int)]


class SCConfig(C.Structure):
    _fields_ = [("max_radius", C.c_double), ("dist_thres", C.c_double), ("max_keyframes", C.c_int), ("float_math", C.c_int),
                ("device", C.c_int), ("n_shards", C.c_int), ("shard", C.c_int), ("side_stream", C.c_int)]


class SCResult(C.Structure):
    _fields_ = [("loop_id", C.c_int), ("yaw_rad", C.c_float), ("min_dist", C.c_double), ("nn_idx", C.c_int), ("nn_shift", C.c_int),
                ("cand_idx", C.c_int * 3), ("cand_keydist", C.c_float * 3), ("cand_scdist", C.c_double * 3), ("cand_shift", C.c_int * 3)]


class SCCand(C.Structure):
    _fields_ = [("key_dist", C.c_float), ("idx", C.c_int), ("sc_dist", C.c_double), ("shift", C.c_int), ("pad", C.c_int)]


class MapConfig(C.Structure):
    _fields_ = [("line_res", C.c_float), ("plane_res", C.c_float), ("max_scan_points", C.c_int), ("max_map_points", C.c_int),
                ("device", C.c_int)]


class MapStats(C.Structure):
    _fields_ = [("n_corner_stack", C.c_int), ("n_surf_stack", C.c_int), ("n_corner_map", C.c_int), ("n_surf_map", C.c_int),
                ("n_edge", C.c_int * 2), ("n_plane", C.c_int * 2), ("lm_iters", C.c_int * 2), ("lm_success", C.c_int * 2),
                ("cost_init", C.c_double * 2), ("cost_final", C.c_double * 2), ("solved", C.c_int),
                ("n_map_corner_total", C.c_int), ("n_map_surf_total", C.c_int), ("insert_path", C.c_int)]


class ICPConfig(C.Structure):
    _fields_ = [("max_corr_dist", C.c_double), ("transformation_epsilon", C.c_double), ("fitness_epsilon", C.c_double),
                ("max_iterations", C.c_int), ("max_source", C.c_int), ("max_target", C.c_int), ("device", C.c_int)]


class ICPResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("n_correspondences", C.c_int),
                ("fitness", C.c_double), ("T", C.c_double * 16)]


class ICPPlaneResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("n_correspondences", C.c_int),
                ("fitness", C.c_double), ("plane_fitness", C.c_double), ("T", C.c_double * 16), ("normal_eq", C.c_double * 27),
                ("first_eq", C.c_double * 27)]


class RefineConfig(C.Structure):
    _fields_ = [("max_corr_dist", C.c_double), ("transformation_epsilon", C.c_double), ("fitness_epsilon", C.c_double),
                ("fitness_gate", C.c_double), ("max_iterations", C.c_int), ("max_frames", C.c_int), ("max_points", C.c_int),
                ("device", C.c_int)]


class RefineFrameResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("n_correspondences", C.c_int),
                ("accepted", C.c_int), ("fitness", C.c_double), ("T", C.c_double * 16)]


class RefinePlaneFrameResult(C.Structure):
    _fields_ = [("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("n_correspondences", C.c_int),
                ("accepted", C.c_int), ("fitness", C.c_double), ("T", C.c_double * 16), ("plane_fitness", C.c_double),
                ("normal_eq", C.c_double * 27), ("first_eq", C.c_double * 27)]


class RelocConfig(C.Structure):
    _fields_ = [("max_keyframes", C.c_int), ("max_points", C.c_int), ("max_query_points", C.c_int), ("sc_max_radius", C.c_double),
                ("sc_dist_thres", C.c_double), ("float_math", C.c_int), ("leaf", C.c_float), ("submap_half", C.c_int),
                ("fitness_thres", C.c_double), ("max_corr_dist", C.c_double), ("transformation_epsilon", C.c_double),
                ("fitness_epsilon", C.c_double), ("max_iterations", C.c_int), ("no_yaw_guess", C.c_int), ("device", C.c_int)]


class RelocResult(C.Structure):
    _fields_ = [("sc", SCResult), ("status", C.c_int), ("n_src", C.c_int), ("n_tgt", C.c_int), ("icp", ICPResult), ("pose12", C.c_double * 12)]


class RemovertConfig(C.Structure):
    _fields_ = [("max_points", C.c_int), ("max_keyframes", C.c_int), ("max_scan_points", C.c_int), ("max_resolutions", C.c_int),
                ("min_hits", C.c_int), ("device", C.c_int), ("fov_up_deg", C.c_double), ("fov_down_deg", C.c_double),
                ("min_range", C.c_double), ("max_range", C.c_double), ("diff_thres", C.c_double), ("min_res_deg", C.c_double),
                ("cell_size", C.c_double)]


class RemovertStats(C.Structure):
    _fields_ = [("points", C.c_longlong), ("keyframes", C.c_longlong), ("dynamic", C.c_longlong), ("pairs_tested", C.c_longlong),
                ("pairs_bruteforce", C.c_longlong)]


class NbrConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("max_index_points", C.c_int), ("max_query_points", C.c_int)]


NBR_MAX_K = 64   # SCAL_NBR_MAX_K


class MapMergeConfig(C.Structure):
    _fields_ = [("max_points", C.c_longlong), ("max_frame_points", C.c_int), ("device", C.c_int)]


class OdomConfig(C.Structure):
    _fields_ = [("max_points", C.c_int), ("device", C.c_int)]


class OdomStats(C.Structure):
    _fields_ = [("n_edge", C.c_int * 2), ("n_plane", C.c_int * 2), ("lm_iters", C.c_int * 2), ("lm_success", C.c_int * 2),
                ("cost_init", C.c_double * 2), ("cost_final", C.c_double * 2)]


class PipelineConfig(C.Structure):
    _fields_ = [("lidar_type", C.c_int), ("n_scans", C.c_int), ("minimum_range", C.c_double), ("max_points", C.c_int),
                ("float_math", C.c_int), ("check_finite", C.c_int), ("line_res", C.c_float), ("plane_res", C.c_float),
                ("max_map_points", C.c_int), ("sc_max_radius", C.c_double), ("sc_dist_thres", C.c_double), ("sc_max_keyframes", C.c_int),
                ("sc_mode", C.c_int), ("device", C.c_int), ("ring", C.c_int), ("depth", C.c_int), ("d_desc_ring", C.c_void_p),
                ("keyframe_meter_gap", C.c_double), ("keyframe_deg_gap", C.c_double), ("kf_max_points", C.c_int), ("loop_fitness_thres", C.c_double),
                ("pgo_map_max_points", C.c_int)]


class PipelineResult(C.Structure):
    _fields_ = [("seq", C.c_longlong), ("q_w_curr", C.c_double * 4), ("t_w_curr", C.c_double * 3), ("q_odom", C.c_double * 4),
                ("t_odom", C.c_double * 3), ("odom", OdomStats), ("map", MapStats), ("have_loop", C.c_int), ("loop", SCResult),
                ("d_descriptor", C.c_void_p), ("is_keyframe", C.c_int), ("keyframe_id", C.c_int)]


class PipelineLoop(C.Structure):
    _fields_ = [("seq", C.c_longlong), ("curr_kf", C.c_int), ("loop_kf", C.c_int), ("yaw_rad", C.c_float), ("min_dist", C.c_double),
                ("verified", C.c_int), ("converged", C.c_int), ("iterations", C.c_int), ("state", C.c_int), ("fitness", C.c_double),
                ("T", C.c_double * 16), ("n_src", C.c_int), ("n_tgt", C.c_int), ("q_rel", C.c_double * 4), ("t_rel", C.c_double * 3)]


class PoseGraphConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("max_nodes", C.c_int), ("max_edges", C.c_int)]


class PoseGraphParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("step_tol", C.c_double), ("max_linear_iterations", C.c_int), ("linear_rtol", C.c_double)]


class PoseGraphStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("linear_iterations", C.c_int), ("linear_status", C.c_int), ("last_step_max", C.c_double)]


class PipelinePgoResult(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("n_odom_edges", C.c_int), ("n_loop_edges", C.c_int), ("applied", C.c_int), ("solver", PoseGraphStats)]


class KeyframeGateState(C.Structure):
    _fields_ = [("meter_gap", C.c_double), ("rad_gap", C.c_double), ("translation_accumulated", C.c_double),
                ("rotation_accumulated", C.c_double), ("curr", C.c_double * 6)]


# every symbol include/scaloam_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "scal_last_error", "scal_device_count", "scal_version", "scal_prof_enable", "scal_prof_filter", "scal_prof_reset", "scal_prof_read", "scal_prof_names", "scal_prof_timeline", "scal_prof_timeline_dump",
    "scal_features_create", "scal_features_destroy", "scal_features_run", "scal_features_run_device", "scal_features_enqueue_host", "scal_features_stream", "scal_voxel_stream", "scal_sc_stream", "scal_map_stream", "scal_odom_stream", "scal_features_fetch",
    "scal_features_sync",
    "scal_voxel_create", "scal_voxel_destroy", "scal_voxel_downsample", "scal_voxel_downsample_device",
    "scal_sc_create", "scal_sc_destroy", "scal_sc_size", "scal_sc_insert_cloud", "scal_sc_insert_cloud_device",
    "scal_sc_insert_descriptor", "scal_sc_get_descriptor", "scal_sc_make_descriptor", "scal_sc_detect", "scal_sc_detect_enqueue", "scal_sc_batch_loop_search", "scal_sc_detect_collect", "scal_sc_distance_pairs",
    "scal_sc_distance_matrix", "scal_sc_distance_matrix_device", "scal_sc_shard_query", "scal_sc_merge_candidates", "scal_sc_insert_features", "scal_sc_make_features",
    "scal_sc_insert_descriptor_device", "scal_sc_shard_query_device", "scal_sc_shard_query_batch_device", "scal_sc_insert_descriptors_device", "scal_sc_sync", "scal_sc_make_features_enqueue", "scal_sc_wait_descriptor",
    "scal_map_create", "scal_map_destroy", "scal_map_step", "scal_map_step_features", "scal_map_export", "scal_map_export_all", "scal_map_get_wmap_wodom", "scal_map_set_merge_insert", "scal_map_get_path_counters", "scal_map_set_poll", "scal_map_debug_set_lm_polls", "scal_map_debug_set_grid_cap", "scal_map_adapter_begin", "scal_map_associate", "scal_map_get_blocks", "scal_map_eval_blocks", "scal_map_adapter_finish", "scal_odom_adapter_begin", "scal_odom_associate", "scal_odom_get_blocks", "scal_odom_eval_blocks", "scal_odom_adapter_finish", "scal_map_prefetch_features", "scal_map_prefetch_begin", "scal_map_prefetch_finish", "scal_map_enqueue_features", "scal_map_collect", "scal_map_finish",
    "scal_set_stream_mode", "scal_mapmerge_create", "scal_mapmerge_destroy", "scal_mapmerge_reset", "scal_mapmerge_add",
    "scal_mapmerge_add_batch_device", "scal_mapmerge_size", "scal_mapmerge_download", "scal_mapmerge_device_points", "scal_mapmerge_downsample", "scal_icp_create", "scal_icp_destroy", "scal_icp_align", "scal_icp_align_device", "scal_icp_set_search",
    "scal_refine_create", "scal_refine_destroy", "scal_refine_run_device", "scal_refine_run",
    "scal_odom_create", "scal_odom_destroy", "scal_odom_step", "scal_odom_step_features", "scal_odom_enqueue_features", "scal_odom_collect",
    "scal_factors_eval",
    "scal_pipeline_create", "scal_pipeline_destroy", "scal_pipeline_push_device", "scal_pipeline_push_host", "scal_pipeline_pop", "scal_pipeline_drain",
    "scal_pipeline_in_flight", "scal_pipeline_sc", "scal_pipeline_map", "scal_pipeline_odom", "scal_pipeline_features",
    "scal_pipeline_create_multi", "scal_pipeline_seqs", "scal_pipeline_push_device_multi", "scal_pipeline_pop_multi", "scal_pipeline_sc_of", "scal_pipeline_map_of",
    "scal_pipeline_pop_loop", "scal_pipeline_keyframe", "scal_keyframe_gate_init", "scal_keyframe_gate",
    "scal_pipeline_update_keyframe_poses", "scal_pipeline_pgo_map", "scal_pipeline_pgo_map_device",
    "scal_pipeline_optimize_keyframes", "scal_posegraph_create", "scal_posegraph_destroy", "scal_posegraph_set_nodes", "scal_posegraph_set_prior",
    "scal_posegraph_add_between", "scal_posegraph_clear_edges", "scal_posegraph_optimize", "scal_posegraph_get_nodes", "scal_posegraph_get_edge_weights",
    "scal_sc_detect_between", "scal_sc_detect_between_device", "scal_sc_cross_matrix", "scal_sc_cross_search", "scal_icp_align_guess", "scal_icp_align_guess_device",
    "scal_reloc_create", "scal_reloc_destroy", "scal_reloc_size", "scal_reloc_add_keyframe", "scal_reloc_query", "scal_reloc_query_batch", "scal_reloc_sc",
    "scal_removert_create", "scal_removert_destroy", "scal_removert_set_map", "scal_removert_set_map_device", "scal_removert_run", "scal_removert_compact", "scal_removert_scan_image",
    "scal_nbr_create", "scal_nbr_destroy", "scal_nbr_set_index", "scal_nbr_set_index_device", "scal_nbr_query", "scal_nbr_query_device", "scal_nbr_query_self", "scal_nbr_stats",
    "scal_nbr_knn", "scal_nbr_knn_device", "scal_nbr_knn_self",
    "scal_nbr_normals", "scal_nbr_normals_device", "scal_nbr_normals_self",
    "scal_icp_align_plane", "scal_icp_align_plane_device",
    "scal_refine_run_plane", "scal_refine_run_plane_device",
]

_lib = None


def lib():
    """Load libscaloam_hip.so.  Raises if it is missing: there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C sc-a-loam_amd` or __graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    L.scal_last_error.restype = C.c_char_p
    L.scal_version.restype = C.c_char_p
    vp = C.c_void_p
    L.scal_features_create.argtypes = [C.POINTER(FeaturesConfig), C.POINTER(vp)]
    L.scal_features_destroy.argtypes = [vp]
    L.scal_features_destroy.restype = None
    L.scal_features_run.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(FeaturesOut)]
    L.scal_features_run_device.argtypes = [vp, vp, C.c_int, C.c_int]
    L.scal_features_enqueue_host.argtypes = [vp, vp, C.c_int, C.c_int]
    for fn in ("scal_features_stream", "scal_voxel_stream", "scal_sc_stream", "scal_map_stream", "scal_odom_stream"):
        getattr(L, fn).restype = C.c_void_p
        getattr(L, fn).argtypes = [vp]
    L.scal_features_fetch.argtypes = [vp, C.POINTER(FeaturesOut)]
    L.scal_features_sync.argtypes = [vp]
    L.scal_voxel_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.scal_voxel_destroy.argtypes = [vp]
    L.scal_voxel_destroy.restype = None
    L.scal_voxel_downsample.argtypes = [vp, _f32p, C.c_int, C.c_float, _f32p, _i32p]
    L.scal_voxel_downsample_device.argtypes = [vp, vp, C.c_int, C.c_float, vp, _i32p]
    L.scal_sc_create.argtypes = [C.POINTER(SCConfig), C.POINTER(vp)]
    L.scal_sc_destroy.argtypes = [vp]
    L.scal_sc_destroy.restype = None
    L.scal_sc_size.argtypes = [vp]
    L.scal_sc_insert_cloud.argtypes = [vp, _f32p, C.c_int]
    L.scal_sc_insert_cloud_device.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.scal_sc_insert_descriptor.argtypes = [vp, _f64p]
    L.scal_sc_get_descriptor.argtypes = [vp, C.c_int, _f64p, _f32p]
    L.scal_sc_make_descriptor.argtypes = [vp, _f32p, C.c_int, _f64p]
    L.scal_sc_detect.argtypes = [vp, C.POINTER(SCResult)]
    L.scal_sc_detect_enqueue.argtypes = [vp]
    L.scal_sc_detect_collect.argtypes = [vp, C.POINTER(SCResult)]
    L.scal_sc_distance_pairs.argtypes = [vp, _i32p, _i32p, C.c_int, _f64p, _i32p]
    L.scal_sc_distance_matrix.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, _i32p]
    L.scal_sc_distance_matrix_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.scal_sc_shard_query.argtypes = [vp, _f64p, C.c_int, C.POINTER(SCCand)]
    L.scal_sc_merge_candidates.argtypes = [C.POINTER(SCCand), C.c_int, C.c_double, C.POINTER(SCResult)]
    L.scal_sc_insert_features.argtypes = [vp, vp]
    L.scal_sc_make_features.argtypes = [vp, vp, vp]
    L.scal_sc_insert_descriptor_device.argtypes = [vp, vp]
    L.scal_sc_shard_query_device.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.scal_sc_shard_query_batch_device.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), vp]
    L.scal_sc_insert_descriptors_device.argtypes = [vp, vp, C.c_int]
    L.scal_sc_sync.argtypes = [vp]
    L.scal_sc_make_features_enqueue.argtypes = [vp, vp, vp]
    L.scal_sc_wait_descriptor.argtypes = [vp]
    L.scal_prof_enable.argtypes = [C.c_int]
    L.scal_prof_filter.argtypes = [C.c_char_p]
    L.scal_prof_read.argtypes = [C.c_char_p, _f64p, C.POINTER(C.c_long)]
    L.scal_prof_names.argtypes = [C.c_char_p, C.c_int]
    L.scal_map_create.argtypes = [C.POINTER(MapConfig), C.POINTER(vp)]
    L.scal_map_destroy.argtypes = [vp]
    L.scal_map_destroy.restype = None
    L.scal_map_step.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f64p, _f64p, _f64p, _f64p, _f32p, C.POINTER(MapStats)]
    L.scal_map_step_features.argtypes = [vp, vp, _f64p, _f64p, _f64p, _f64p, C.POINTER(MapStats)]
    L.scal_map_export.argtypes = [vp, C.c_int, _f32p, C.c_int]
    L.scal_map_export_all.argtypes = [vp, C.c_int, _f32p, C.c_int]
    L.scal_map_get_wmap_wodom.argtypes = [vp, _f64p, _f64p]
    L.scal_map_set_merge_insert.argtypes = [vp, C.c_int]
    L.scal_map_get_path_counters.argtypes = [vp, C.POINTER(C.c_int)]
    L.scal_map_adapter_begin.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f64p, _f64p, _f64p, _f64p]
    L.scal_map_associate.argtypes = [vp, _f64p, _f64p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.scal_map_get_blocks.argtypes = [vp, vp, C.c_int]
    L.scal_map_eval_blocks.argtypes = [vp, _f64p, C.c_int, _f64p, _f64p]
    L.scal_map_adapter_finish.argtypes = [vp, _f64p, _f64p, _f32p, C.POINTER(MapStats)]
    L.scal_odom_adapter_begin.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f64p, _f64p, C.POINTER(C.c_int)]
    L.scal_odom_associate.argtypes = [vp, _f64p, _f64p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.scal_odom_get_blocks.argtypes = [vp, vp, C.c_int]
    L.scal_odom_eval_blocks.argtypes = [vp, _f64p, C.c_int, _f64p, _f64p]
    L.scal_odom_adapter_finish.argtypes = [vp, _f64p, _f64p, _f64p, _f64p]
    L.scal_map_set_poll.argtypes = [vp, C.c_int]
    L.scal_map_debug_set_lm_polls.argtypes = [vp, C.c_int]
    if hasattr(L, "scal_map_debug_set_grid_cap"):  # absent from older builds compared through SCALOAM_LIB (tools/gpu_ab.sh)
        L.scal_map_debug_set_grid_cap.argtypes = [vp, C.c_int, C.c_int]
    L.scal_map_prefetch_features.argtypes = [vp, vp]
    L.scal_map_prefetch_begin.argtypes = [vp, vp]
    L.scal_map_prefetch_finish.argtypes = [vp, vp]
    L.scal_map_enqueue_features.argtypes = [vp, vp, _f64p, _f64p]
    L.scal_map_collect.argtypes = [vp, _f64p, _f64p, C.POINTER(MapStats)]
    L.scal_map_finish.argtypes = [vp]
    L.scal_set_stream_mode.argtypes = [C.c_int]
    L.scal_icp_create.argtypes = [C.POINTER(ICPConfig), C.POINTER(vp)]
    L.scal_icp_destroy.argtypes = [vp]
    L.scal_icp_destroy.restype = None
    L.scal_icp_align.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, C.POINTER(ICPResult)]
    L.scal_icp_set_search.argtypes = [vp, C.c_int]
    L.scal_icp_align_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(ICPResult)]
    if hasattr(L, "scal_refine_create"):  # absent from older builds compared through SCALOAM_LIB
        L.scal_refine_create.argtypes = [C.POINTER(RefineConfig), C.POINTER(vp)]
        L.scal_refine_destroy.argtypes = [vp]
        L.scal_refine_destroy.restype = None
        for fn in (L.scal_refine_run_device, L.scal_refine_run):
            fn.argtypes = [vp, vp, _i32p, C.c_int, _f64p, C.c_char_p, C.c_double, C.c_int, C.POINTER(RefineFrameResult), _i32p]
    if hasattr(L, "scal_refine_run_plane"):  # absent from older builds compared through SCALOAM_LIB
        for fn in (L.scal_refine_run_plane_device, L.scal_refine_run_plane):
            fn.argtypes = [vp, vp, vp, _i32p, C.c_int, _f64p, C.c_char_p, C.c_double, C.c_int, C.POINTER(RefinePlaneFrameResult), _i32p]
    L.scal_mapmerge_create.argtypes = [C.POINTER(MapMergeConfig), C.POINTER(vp)]
    L.scal_mapmerge_destroy.argtypes = [vp]
    L.scal_mapmerge_destroy.restype = None
    L.scal_mapmerge_reset.argtypes = [vp]
    L.scal_mapmerge_add.argtypes = [vp, _f32p, C.c_int, _f64p, C.c_double]
    L.scal_mapmerge_add_batch_device.argtypes = [vp, vp, C.POINTER(C.c_int), _f64p, C.c_int, C.c_double]
    L.scal_mapmerge_size.argtypes = [vp]
    L.scal_mapmerge_size.restype = C.c_longlong
    L.scal_mapmerge_download.argtypes = [vp, _f32p, C.c_longlong]
    L.scal_mapmerge_downsample.argtypes = [vp, C.c_float, _f32p, C.c_longlong, C.POINTER(C.c_longlong)]
    L.scal_mapmerge_device_points.argtypes = [vp]
    L.scal_mapmerge_device_points.restype = vp
    L.scal_odom_create.argtypes = [C.POINTER(OdomConfig), C.POINTER(vp)]
    L.scal_odom_destroy.argtypes = [vp]
    L.scal_odom_destroy.restype = None
    L.scal_odom_step.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.c_int, _f64p, _f64p, _f64p, _f64p,
                                 C.POINTER(OdomStats)]
    L.scal_odom_step_features.argtypes = [vp, vp, _f64p, _f64p, _f64p, _f64p, C.POINTER(OdomStats)]
    L.scal_odom_enqueue_features.argtypes = [vp, vp]
    L.scal_odom_collect.argtypes = [vp, _f64p, _f64p, _f64p, _f64p, C.POINTER(OdomStats)]
    L.scal_factors_eval.argtypes = [C.c_int, C.c_int, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]
    L.scal_pipeline_create.argtypes = [C.POINTER(PipelineConfig), C.POINTER(vp)]
    L.scal_pipeline_destroy.argtypes = [vp]
    L.scal_pipeline_destroy.restype = None
    L.scal_pipeline_push_device.argtypes = [vp, vp, C.c_int, C.c_int]
    L.scal_pipeline_push_host.argtypes = [vp, vp, C.c_int, C.c_int]
    L.scal_pipeline_pop.argtypes = [vp, C.POINTER(PipelineResult)]
    L.scal_pipeline_drain.argtypes = [vp]
    L.scal_pipeline_in_flight.argtypes = [vp]
    for fn in ("scal_pipeline_sc", "scal_pipeline_map", "scal_pipeline_odom"):
        getattr(L, fn).restype = C.c_void_p
        getattr(L, fn).argtypes = [vp]
    L.scal_pipeline_features.restype = C.c_void_p
    L.scal_pipeline_features.argtypes = [vp, C.c_int]
    L.scal_pipeline_create_multi.argtypes = [C.POINTER(PipelineConfig), C.c_int, C.POINTER(vp)]
    L.scal_pipeline_seqs.argtypes = [vp]
    L.scal_pipeline_push_device_multi.argtypes = [vp, C.POINTER(C.c_void_p), _i32p, C.c_int]
    L.scal_pipeline_pop_multi.argtypes = [vp, C.POINTER(PipelineResult)]
    L.scal_pipeline_pop_loop.argtypes = [vp, C.POINTER(PipelineLoop), C.c_int]
    L.scal_pipeline_keyframe.argtypes = [vp, C.c_int, _f64p, _f32p, C.c_int, _i32p]
    L.scal_pipeline_update_keyframe_poses.argtypes = [vp, _i32p, _f64p, C.c_int]
    L.scal_pipeline_pgo_map.argtypes = [vp, C.c_int, C.c_int, C.c_float, _f32p, C.c_longlong, C.POINTER(C.c_longlong)]
    L.scal_pipeline_pgo_map_device.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.scal_pipeline_pgo_map_device.restype = C.c_void_p
    if hasattr(L, "scal_posegraph_create"):  # absent from older builds compared through SCALOAM_LIB
        L.scal_pipeline_optimize_keyframes.argtypes = [vp, C.c_int, C.c_int, _i32p, _f64p, C.c_int, C.POINTER(PipelinePgoResult)]
        L.scal_posegraph_create.argtypes = [C.POINTER(PoseGraphConfig), C.POINTER(vp)]
        L.scal_posegraph_destroy.argtypes = [vp]
        L.scal_posegraph_destroy.restype = None
        L.scal_posegraph_set_nodes.argtypes = [vp, _f64p, C.c_int]
        L.scal_posegraph_set_prior.argtypes = [vp, C.c_int, _f64p, _f64p]
        L.scal_posegraph_add_between.argtypes = [vp, C.c_int, _i32p, _i32p, _f64p, _f64p, _f64p]
        L.scal_posegraph_clear_edges.argtypes = [vp]
        L.scal_posegraph_optimize.argtypes = [vp, C.POINTER(PoseGraphParams), C.POINTER(PoseGraphStats)]
        L.scal_posegraph_get_nodes.argtypes = [vp, _f64p, C.c_int]
        L.scal_posegraph_get_edge_weights.argtypes = [vp, _f64p, C.c_int]
    if hasattr(L, "scal_reloc_create"):  # absent from older builds compared through SCALOAM_LIB
        L.scal_sc_detect_between.argtypes = [vp, _f64p, C.c_int, C.POINTER(SCResult)]
        L.scal_sc_detect_between_device.argtypes = [vp, vp, C.c_int, C.POINTER(SCResult)]
        L.scal_sc_cross_matrix.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, _i32p]
        L.scal_sc_cross_search.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _f64p, _i32p]
        L.scal_icp_align_guess.argtypes = [vp, _f32p, C.c_int, _f32p, C.c_int, _f32p, C.POINTER(ICPResult)]
        L.scal_icp_align_guess_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, _f32p, C.POINTER(ICPResult)]
        L.scal_reloc_create.argtypes = [C.POINTER(RelocConfig), C.POINTER(vp)]
        L.scal_reloc_destroy.argtypes = [vp]
        L.scal_reloc_destroy.restype = None
        L.scal_reloc_size.argtypes = [vp]
        L.scal_reloc_add_keyframe.argtypes = [vp, _f32p, C.c_int, _f64p, _f64p]
        L.scal_reloc_query.argtypes = [vp, _f32p, C.c_int, C.POINTER(RelocResult)]
        L.scal_reloc_query_batch.argtypes = [vp, _f32p, _i32p, C.c_int, C.POINTER(RelocResult)]
        L.scal_reloc_sc.argtypes = [vp]
        L.scal_reloc_sc.restype = C.c_void_p
    if hasattr(L, "scal_removert_create"):  # absent from older builds compared through SCALOAM_LIB
        L.scal_removert_create.argtypes = [C.POINTER(RemovertConfig), C.POINTER(vp)]
        L.scal_removert_destroy.argtypes = [vp]
        L.scal_removert_destroy.restype = None
        L.scal_removert_set_map.argtypes = [vp, _f32p, C.c_int]
        L.scal_removert_set_map_device.argtypes = [vp, vp, C.c_int]
        L.scal_removert_run.argtypes = [vp, _f32p, _i32p, C.c_int, _f64p, _f64p, C.c_int, _f64p, C.c_int, C.POINTER(C.c_ubyte),
                                        C.POINTER(C.c_ushort), C.POINTER(RemovertStats)]
        L.scal_removert_compact.argtypes = [vp, C.c_int, _f32p, C.c_int, _i32p]
        L.scal_removert_scan_image.argtypes = [vp, C.c_int, C.c_int, _f32p, C.c_int, C.c_int]
    if hasattr(L, "scal_nbr_create"):  # absent from older builds compared through SCALOAM_LIB
        _u16p = C.POINTER(C.c_ushort)
        L.scal_nbr_create.argtypes = [C.POINTER(NbrConfig), C.POINTER(vp)]
        L.scal_nbr_destroy.argtypes = [vp]
        L.scal_nbr_destroy.restype = None
        L.scal_nbr_set_index.argtypes = [vp, _f32p, C.c_int, C.c_double]
        L.scal_nbr_set_index_device.argtypes = [vp, vp, C.c_int, C.c_double]
        L.scal_nbr_query.argtypes = [vp, _f32p, C.c_int, _u16p, _f32p]
        L.scal_nbr_query_device.argtypes = [vp, vp, C.c_int, vp, vp]
        L.scal_nbr_query_self.argtypes = [vp, _u16p, _f32p]
        L.scal_nbr_stats.argtypes = [vp, C.POINTER(C.c_longlong), _i32p]
    if hasattr(L, "scal_nbr_knn"):
        L.scal_nbr_knn.argtypes = [vp, _f32p, C.c_int, C.c_int, _i32p, _f32p]
        L.scal_nbr_knn_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
        L.scal_nbr_knn_self.argtypes = [vp, C.c_int, _i32p, _f32p]
    if hasattr(L, "scal_nbr_normals"):
        L.scal_nbr_normals.argtypes = [vp, _f32p, C.c_int, C.c_int, _f64p, _f32p, _f32p]
        L.scal_nbr_normals_device.argtypes = [vp, vp, C.c_int, C.c_int, _f64p, vp, vp]
        L.scal_nbr_normals_self.argtypes = [vp, C.c_int, _f64p, _f32p, _f32p]
    if hasattr(L, "scal_icp_align_plane"):  # absent from older builds compared through SCALOAM_LIB
        L.scal_icp_align_plane.argtypes = [vp, _f32p, C.c_int, _f32p, _f32p, C.c_int, _f32p, C.POINTER(ICPPlaneResult)]
        L.scal_icp_align_plane_device.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, _f32p, C.POINTER(ICPPlaneResult)]
    L.scal_keyframe_gate_init.argtypes =[C.POINTER(KeyframeGateState), C.c_double, C.c_double]
    L.scal_keyframe_gate.argtypes = [C.POINTER(KeyframeGateState), _f64p, _f64p, _i32p]
    for fn in ("scal_pipeline_sc_of", "scal_pipeline_map_of"):
        getattr(L, fn).restype = C.c_void_p
        getattr(L, fn).argtypes = [vp, C.c_int]
    _lib = L
    return L


def _check(rc):
    if rc != OK:
        raise ScalError(rc, lib().scal_last_error().decode())


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def set_stream_mode(mode):
    _check(lib().scal_set_stream_mode(int(mode)))


def device_count():
    return lib().scal_device_count()


def prof_enable(on, kernel=None):
    lib().scal_prof_filter(kernel.encode() if kernel else None)
    lib().scal_prof_enable(1 if on else 0)


def prof_reset():
    lib().scal_prof_reset()


def prof_timeline(on):
    lib().scal_prof_timeline(1 if on else 0)


def prof_timeline_dump(path):
    lib().scal_prof_timeline_dump(path.encode())


def prof_read_all():
    """{kernel name: (total_ms, launches)} measured with HIP events on the launching stream."""
    buf = C.create_string_buffer(4096)
    lib().scal_prof_names(buf, 4096)
    out = {}
    for name in buf.value.decode().split(";"):
        if not name:
            continue
        ms = C.c_double(0)
        cnt = C.c_long(0)
        lib().scal_prof_read(name.encode(), C.byref(ms), C.byref(cnt))
        out[name] = (ms.value, cnt.value)
    return out


# ---------------------------------------------------------------------------------------------- stage A
class ScanRegistration:
    """Mirror of the reference's scanRegistration node state (scan_line, lidar_type, minimum_range rosparams,
    scanRegistration.cpp:480-482) with laserCloudHandler as a method."""

    def __init__(self, lidar_type, minimum_range, max_points=400000, float_math=0, check_finite=1, device=0, n_scans=None):
        self.cfg = FeaturesConfig(lidar_type, SCAN_LINES.get(lidar_type, 0) if n_scans is None else n_scans, float(minimum_range),
                                  max_points, float_math, check_finite, device)
        self.h = C.c_void_p()
        _check(lib().scal_features_create(C.byref(self.cfg), C.byref(self.h)))
        self.n_scans = self.cfg.n_scans
        m = max_points
        ns = self.n_scans
        self._b = dict(cloud=np.zeros((m, 4), np.float32), src_index=np.zeros(m, np.int32), curvature=np.zeros(m, np.float32),
                       label=np.zeros(m, np.int32), ring_start=np.zeros(ns, np.int32), ring_end=np.zeros(ns, np.int32),
                       sharp=np.zeros(12 * ns, np.int32), less_sharp=np.zeros(120 * ns, np.int32), flat=np.zeros(24 * ns, np.int32),
                       less_flat=np.zeros((m, 4), np.float32))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_features_destroy(self.h)
        self.h = None

    __del__ = close

    def _out(self):
        b = self._b
        return FeaturesOut(_p(b["cloud"], _f32p), _p(b["src_index"], _i32p), _p(b["curvature"], _f32p), _p(b["label"], _i32p),
                           _p(b["ring_start"], _i32p), _p(b["ring_end"], _i32p), _p(b["sharp"], _i32p), _p(b["less_sharp"], _i32p),
                           _p(b["flat"], _i32p), _p(b["less_flat"], _f32p))

    def _pack(self, o):
        b = self._b
        k = o.n_kept
        return dict(n_kept=k, cloud=b["cloud"][:k].copy(), src_index=b["src_index"][:k].copy(), curvature=b["curvature"][:k].copy(),
                    label=b["label"][:k].copy(), ring_start=b["ring_start"].copy(), ring_end=b["ring_end"].copy(),
                    sharp=b["sharp"][:o.n_sharp].copy(), less_sharp=b["less_sharp"][:o.n_less_sharp].copy(),
                    flat=b["flat"][:o.n_flat].copy(), less_flat=b["less_flat"][:o.n_less_flat].copy(), n_tied_segments=o.n_tied_segments)

    def laserCloudHandler(self, xyz):
        xyz = _f32(xyz)
        o = self._out()
        stride = xyz.strides[0] if xyz.shape[0] > 0 else 4 * xyz.shape[1]
        _check(lib().scal_features_run(self.h, xyz.ctypes.data, xyz.shape[0], stride, C.byref(o)))
        return self._pack(o)

    def enqueue_host(self, xyz):
        """asynchronous laserCloudHandler: pinned staging + upload + stage A on the context's stream, results stay on the GPU"""
        xyz = _f32(xyz)
        stride = xyz.strides[0] if xyz.shape[0] > 0 else 4 * xyz.shape[1]
        _check(lib().scal_features_enqueue_host(self.h, xyz.ctypes.data, xyz.shape[0], stride))

    def run_device(self, d_ptr, n, stride_floats):
        _check(lib().scal_features_run_device(self.h, d_ptr, n, stride_floats))

    def fetch(self):
        o = self._out()
        _check(lib().scal_features_fetch(self.h, C.byref(o)))
        return self._pack(o)

    def sync(self):
        _check(lib().scal_features_sync(self.h))


# ---------------------------------------------------------------------------------------------- voxel grid
class VoxelGrid:
    def __init__(self, max_points=400000, device=0):
        self.h = C.c_void_p()
        _check(lib().scal_voxel_create(max_points, device, C.byref(self.h)))
        self.cap = max_points

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_voxel_destroy(self.h)
        self.h = None

    __del__ = close

    def filter(self, xyzi, leaf):
        xyzi = _f32(xyzi).reshape(-1, 4)
        out = np.zeros((max(1, xyzi.shape[0]), 4), np.float32)
        n = C.c_int(0)
        _check(lib().scal_voxel_downsample(self.h, _p(xyzi, _f32p), xyzi.shape[0], C.c_float(leaf), _p(out, _f32p), C.byref(n)))
        return out[:n.value].copy()

    def stream_ptr(self):
        """the context's hipStream_t (to order it against the caller's streams, e.g. torch.cuda.ExternalStream(ptr))"""
        return lib().scal_voxel_stream(self.h)

    def filter_device(self, d_in_ptr, n, leaf, d_out_ptr):
        """16-byte xyzi records in device memory in, centroids to d_out_ptr (room for n records); returns their number."""
        m = C.c_int(0)
        _check(lib().scal_voxel_downsample_device(self.h, d_in_ptr, n, C.c_float(leaf), d_out_ptr, C.byref(m)))
        return m.value


# ---------------------------------------------------------------------------------------------- stage D
class SCManager:
    """Mirror of the reference's SCManager public API (Scancontext.h:62-79, :107-108).  Descriptors cross this
    boundary as [ring, sector] numpy arrays; the C-ABI itself uses Eigen's column-major layout."""

    def __init__(self, max_radius=80.0, dist_thres=0.2, max_keyframes=8192, float_math=0, device=0, n_shards=1, shard=0, side_stream=0):
        self.cfg = SCConfig(max_radius, dist_thres, max_keyframes, float_math, device, n_shards, shard, side_stream)
        self.h = C.c_void_p()
        _check(lib().scal_sc_create(C.byref(self.cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_sc_destroy(self.h)
        self.h = None

    __del__ = close

    def size(self):
        return lib().scal_sc_size(self.h)

    def makeScancontext(self, xyzi):
        xyzi = _f32(xyzi).reshape(-1, 4)
        d = np.zeros(1200)
        _check(lib().scal_sc_make_descriptor(self.h, _p(xyzi, _f32p), xyzi.shape[0], _p(d, _f64p)))
        return d.reshape(60, 20).T.copy()

    def makeAndSaveScancontextAndKeys(self, xyzi):
        xyzi = _f32(xyzi).reshape(-1, 4)
        _check(lib().scal_sc_insert_cloud(self.h, _p(xyzi, _f32p), xyzi.shape[0]))

    def saveScancontextAndKeys(self, desc_ring_sector):
        d = _f64(np.asarray(desc_ring_sector).T.reshape(-1))
        _check(lib().scal_sc_insert_descriptor(self.h, _p(d, _f64p)))

    def get(self, idx):
        d = np.zeros(1200)
        k = np.zeros(20, np.float32)
        _check(lib().scal_sc_get_descriptor(self.h, idx, _p(d, _f64p), _p(k, _f32p)))
        return d.reshape(60, 20).T.copy(), k

    def stream_ptr(self):
        """the context's hipStream_t (to order it against the caller's streams, e.g. torch.cuda.ExternalStream(ptr))"""
        return lib().scal_sc_stream(self.h)

    def insert_features(self, feat):
        """keyframe cloud of a ScanRegistration context -> VoxelGrid(0.4) -> makeAndSaveScancontextAndKeys, all on the GPU"""
        _check(lib().scal_sc_insert_features(self.h, feat.h))

    def make_features(self, feat, d_desc_ptr):
        _check(lib().scal_sc_make_features(self.h, feat.h, d_desc_ptr))

    def make_features_enqueue(self, feat, d_desc_ptr):
        _check(lib().scal_sc_make_features_enqueue(self.h, feat.h, d_desc_ptr))

    def wait_descriptor(self):
        _check(lib().scal_sc_wait_descriptor(self.h))

    def insert_descriptor_device(self, d_desc_ptr):
        _check(lib().scal_sc_insert_descriptor_device(self.h, d_desc_ptr))

    def shard_query_batch_device(self, d_queries_ptr, limits, d_out_ptr):
        lim = (C.c_int * len(limits))(*[int(v) for v in limits])
        _check(lib().scal_sc_shard_query_batch_device(self.h, d_queries_ptr, len(limits), lim, d_out_ptr))

    def insert_descriptors_device(self, d_descs_ptr, n):
        _check(lib().scal_sc_insert_descriptors_device(self.h, d_descs_ptr, n))

    def sync(self):
        _check(lib().scal_sc_sync(self.h))

    def shard_query_device(self, d_queries_ptr, nq, global_size_at_rebuild, d_out_ptr):
        _check(lib().scal_sc_shard_query_device(self.h, d_queries_ptr, nq, global_size_at_rebuild, d_out_ptr))

    def detect_enqueue(self):
        _check(lib().scal_sc_detect_enqueue(self.h))

    def detect_collect(self):
        r = SCResult()
        _check(lib().scal_sc_detect_collect(self.h, C.byref(r)))
        return self._result(r)

    def detectLoopClosureID(self):
        r = SCResult()
        _check(lib().scal_sc_detect(self.h, C.byref(r)))
        return self._result(r)

    @staticmethod
    def _result(r):
        return dict(loop_id=r.loop_id, yaw=r.yaw_rad, min_dist=r.min_dist, nn_idx=r.nn_idx, nn_shift=r.nn_shift,
                    cand=np.array(r.cand_idx[:]), cand_d=np.array(r.cand_keydist[:], np.float32), cand_sc=np.array(r.cand_scdist[:]),
                    cand_shift=np.array(r.cand_shift[:]))

    def distance_pairs(self, ia, ib):
        ia = np.ascontiguousarray(ia, np.int32)
        ib = np.ascontiguousarray(ib, np.int32)
        d = np.zeros(ia.shape[0])
        s = np.zeros(ia.shape[0], np.int32)
        _check(lib().scal_sc_distance_pairs(self.h, _p(ia, _i32p), _p(ib, _i32p), ia.shape[0], _p(d, _f64p), _p(s, _i32p)))
        return d, s

    def distance_matrix(self, q0, q1, d0, d1, mode=0):
        d = np.zeros((max(0, q1 - q0), max(0, d1 - d0)))  # inverted ranges are the library's to refuse
        s = np.zeros((max(0, q1 - q0), max(0, d1 - d0)), np.int32)
        _check(lib().scal_sc_distance_matrix(self.h, q0, q1, d0, d1, mode, _p(d, _f64p), _p(s, _i32p)))
        return d, s

    def batch_loop_search(self, q0, q1, exclude_recent=30, k=3, mode=2):
        """(idx, dist, shift) arrays [q1-q0][k]: the k best older keyframes of every query keyframe, exhaustive over the database"""
        n = max(0, q1 - q0)
        idx, dist, shift = np.zeros((n, k), np.int32), np.zeros((n, k)), np.zeros((n, k), np.int32)
        _check(lib().scal_sc_batch_loop_search(self.h, q0, q1, exclude_recent, k, mode, _p(idx, _i32p), _p(dist, _f64p), _p(shift, _i32p)))
        return idx, dist, shift

    def detect_between(self, query_descs):
        """detectLoopClosureIDBetweenSession for every [ring, sector] descriptor of `query_descs` (a list or an [nq, 20, 60] array) against
        the whole database; a list of detectLoopClosureID-style dicts"""
        q = [np.asarray(d) for d in query_descs]
        flat = _f64(np.stack([d.T.reshape(-1) for d in q])) if q else np.zeros((0, 1200))
        res = (SCResult * max(1, len(q)))()
        _check(lib().scal_sc_detect_between(self.h, _p(flat, _f64p), len(q), res))
        return [self._result(r) for r in res[:len(q)]]

    def detect_between_device(self, d_query_descs_ptr, nq):
        """the same with nq column-major descriptors back to back in device memory"""
        res = (SCResult * max(1, nq))()
        _check(lib().scal_sc_detect_between_device(self.h, d_query_descs_ptr, nq, res))
        return [self._result(r) for r in res[:nq]]

    def cross_matrix(self, queries, q0, q1, d0, d1, mode=0):
        """distance_matrix with the query rows taken from entries [q0, q1) of another SCManager on the same device"""
        d = np.zeros((max(0, q1 - q0), max(0, d1 - d0)))
        s = np.zeros((max(0, q1 - q0), max(0, d1 - d0)), np.int32)
        _check(lib().scal_sc_cross_matrix(self.h, queries.h, q0, q1, d0, d1, mode, _p(d, _f64p), _p(s, _i32p)))
        return d, s

    def cross_search(self, queries, q0, q1, k=3, mode=2):
        """(idx, dist, shift) arrays [q1-q0][k]: the k best entries of this database for every entry [q0, q1) of `queries`"""
        n = max(0, q1 - q0)
        idx, dist, shift = np.zeros((n, max(k, 1)), np.int32), np.zeros((n, max(k, 1))), np.zeros((n, max(k, 1)), np.int32)
        _check(lib().scal_sc_cross_search(self.h, queries.h, q0, q1, k, mode, _p(idx, _i32p), _p(dist, _f64p), _p(shift, _i32p)))
        return idx, dist, shift

    def distance_matrix_device(self, q0, q1, d0, d1, mode, d_dist_ptr, d_shift_ptr):
        """Device outputs ((q1-q0)*(d1-d0) doubles / int32), enqueued on the context's stream; sync() before reading."""
        _check(lib().scal_sc_distance_matrix_device(self.h, q0, q1, d0, d1, mode, d_dist_ptr, d_shift_ptr))

    def shard_query(self, query_desc_ring_sector, global_size_at_rebuild):
        d = _f64(np.asarray(query_desc_ring_sector).T.reshape(-1))
        out = (SCCand * 3)()
        _check(lib().scal_sc_shard_query(self.h, _p(d, _f64p), global_size_at_rebuild, out))
        return out


def merge_candidates(cands, dist_thres):
    arr = (SCCand * len(cands))(*cands)
    r = SCResult()
    _check(lib().scal_sc_merge_candidates(arr, len(cands), dist_thres, C.byref(r)))
    return dict(loop_id=r.loop_id, yaw=r.yaw_rad, min_dist=r.min_dist, nn_idx=r.nn_idx, nn_shift=r.nn_shift,
                cand=np.array(r.cand_idx[:]), cand_d=np.array(r.cand_keydist[:], np.float32))


class _CeresAdapter:
    """Ceres-adapter mode of stages B and C, between the class's adapter_begin and adapter_finish: per outer iteration
    associate() at the solver's pose, then blocks() / eval_blocks().  `_prefix` names the context's entry points."""

    def associate(self, q, t):
        nb, nr = C.c_int(0), C.c_int(0)
        _check(getattr(lib(), self._prefix + "_associate")(self.h, _p(_f64(q), _f64p), _p(_f64(t), _f64p), C.byref(nb), C.byref(nr)))
        self._adapter_n = (nb.value, nr.value)
        return nb.value, nr.value

    def blocks(self, cap=None):
        """(kind [n], cp [n][3], pa [n][3], pb [n][3]) of the residual blocks of the last associate(), the first `cap` if given"""
        nb = self._adapter_n[0] if cap is None else cap
        raw = np.zeros((max(nb, 1), 10), np.float64)
        n = getattr(lib(), self._prefix + "_get_blocks")(self.h, raw.ctypes.data, nb)
        if n < 0:
            _check(n)
        raw = raw[:n]
        kind = raw[:, 0].copy().view(np.int32)[::2].copy()
        return kind, raw[:, 1:4].copy(), raw[:, 4:7].copy(), raw[:, 7:10].copy()

    def eval_blocks(self, x7, want_jac=True):
        nr = self._adapter_n[1]
        r, J = np.zeros(max(nr, 1)), np.zeros((max(nr, 1), 7))
        _check(getattr(lib(), self._prefix + "_eval_blocks")(self.h, _p(_f64(x7), _f64p), 1 if want_jac else 0, _p(r, _f64p), _p(J, _f64p)))
        return r[:nr], (J[:nr] if want_jac else None)


# ---------------------------------------------------------------------------------------------- stage C
class LaserMapping(_CeresAdapter):
    """Mirror of the reference's laserMapping node state (mapping_line_resolution / mapping_plane_resolution,
    laserMapping.cpp:915-916) with one process() pass as `process`."""
    _prefix = "scal_map"

    def __init__(self, line_res=0.4, plane_res=0.8, max_scan_points=400000, max_map_points=4000000, device=0):
        self.cfg = MapConfig(line_res, plane_res, max_scan_points, max_map_points, device)
        self.h = C.c_void_p()
        _check(lib().scal_map_create(C.byref(self.cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_map_destroy(self.h)
        self.h = None

    __del__ = close

    def process(self, corner_last, surf_last, full_res, q_wodom, t_wodom, want_registered=False):
        c = _f32(corner_last).reshape(-1, 4)
        s = _f32(surf_last).reshape(-1, 4)
        f = _f32(full_res).reshape(-1, 4) if full_res is not None else None
        q = _f64(q_wodom)
        t = _f64(t_wodom)
        qo = np.zeros(4)
        to = np.zeros(3)
        reg = np.zeros_like(f) if (want_registered and f is not None) else None
        st = MapStats()
        _check(lib().scal_map_step(self.h, _p(c, _f32p), c.shape[0], _p(s, _f32p), s.shape[0], _p(f, _f32p), 0 if f is None else f.shape[0],
                                   _p(q, _f64p), _p(t, _f64p), _p(qo, _f64p), _p(to, _f64p), _p(reg, _f32p), C.byref(st)))
        return qo, to, st, reg

    def process_features(self, feat, q_wodom, t_wodom):
        q = _f64(q_wodom)
        t = _f64(t_wodom)
        qo = np.zeros(4)
        to = np.zeros(3)
        st = MapStats()
        _check(lib().scal_map_step_features(self.h, feat.h, _p(q, _f64p), _p(t, _f64p), _p(qo, _f64p), _p(to, _f64p), C.byref(st)))
        return qo, to, st

    def export(self, which):
        n = lib().scal_map_export(self.h, which, None, 0)
        if n < 0:
            _check(n)
        out = np.zeros((max(n, 1), 4), np.float32)
        m = lib().scal_map_export(self.h, which, _p(out, _f32p), n)
        return out[:m]

    def export_all(self, which):
        """every point of the 21x21x11 cube grid, one feature class: the content of /laser_cloud_map (laserMapping.cpp:824-837)"""
        n = lib().scal_map_export_all(self.h, which, None, 0)
        if n < 0:
            _check(n)
        out = np.zeros((max(n, 1), 4), np.float32)
        m = lib().scal_map_export_all(self.h, which, _p(out, _f32p), n)
        if m < 0:
            _check(m)
        return out[:m]

    def enqueue_features(self, feat, q_wodom, t_wodom):
        _check(lib().scal_map_enqueue_features(self.h, feat.h, _p(_f64(q_wodom), _f64p), _p(_f64(t_wodom), _f64p)))

    def collect(self):
        qo, to, st = np.zeros(4), np.zeros(3), MapStats()
        _check(lib().scal_map_collect(self.h, _p(qo, _f64p), _p(to, _f64p), C.byref(st)))
        return qo, to, st

    def finish(self):
        _check(lib().scal_map_finish(self.h))

    def prefetch_features(self, feat):
        _check(lib().scal_map_prefetch_features(self.h, feat.h))

    # ---- Ceres-adapter mode (the caller owns the solver): begin -> per outer iteration associate / blocks / eval (_CeresAdapter) -> finish
    def adapter_begin(self, corner_last, surf_last, full_res, q_wodom, t_wodom):
        c = _f32(corner_last).reshape(-1, 4)
        s = _f32(surf_last).reshape(-1, 4)
        f = _f32(full_res).reshape(-1, 4) if full_res is not None else None
        self._adapter_full = f
        q, t = np.zeros(4), np.zeros(3)
        _check(lib().scal_map_adapter_begin(self.h, _p(c, _f32p), c.shape[0], _p(s, _f32p), s.shape[0], _p(f, _f32p), 0 if f is None else f.shape[0],
                                            _p(_f64(q_wodom), _f64p), _p(_f64(t_wodom), _f64p), _p(q, _f64p), _p(t, _f64p)))
        return q, t

    def adapter_finish(self, q_w_curr, t_w_curr, want_registered=False):
        f = self._adapter_full
        reg = np.zeros_like(f) if (want_registered and f is not None) else None
        st = MapStats()
        _check(lib().scal_map_adapter_finish(self.h, _p(_f64(q_w_curr), _f64p), _p(_f64(t_w_curr), _f64p), _p(reg, _f32p), C.byref(st)))
        return st, reg

    def path_counters(self):
        """(queued speculatively, general path, redone after a moved window, insertion redone with the full sort)"""
        out = (C.c_int * 4)()
        _check(lib().scal_map_get_path_counters(self.h, out))
        return tuple(out)

    def debug_set_lm_polls(self, polls):
        _check(lib().scal_map_debug_set_lm_polls(self.h, polls))

    def debug_set_grid_cap(self, cap_corner, cap_surf):
        _check(lib().scal_map_debug_set_grid_cap(self.h, cap_corner, cap_surf))

    def set_poll(self, enable):
        _check(lib().scal_map_set_poll(self.h, 1 if enable else 0))

    def set_merge_insert(self, enable):
        _check(lib().scal_map_set_merge_insert(self.h, 1 if enable else 0))

    def wmap_wodom(self):
        q = np.zeros(4)
        t = np.zeros(3)
        _check(lib().scal_map_get_wmap_wodom(self.h, _p(q, _f64p), _p(t, _f64p)))
        return q, t


# ---------------------------------------------------------------------------------------------- stage B
class LaserOdometry(_CeresAdapter):
    _prefix = "scal_odom"

    def __init__(self, max_points=400000, device=0):
        self.cfg = OdomConfig(max_points, device)
        self.h = C.c_void_p()
        _check(lib().scal_odom_create(C.byref(self.cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_odom_destroy(self.h)
        self.h = None

    __del__ = close

    def step(self, sharp, less_sharp, flat, less_flat):
        a = [_f32(x).reshape(-1, 4) for x in (sharp, less_sharp, flat, less_flat)]
        qlc, tlc, qw, tw = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        st = OdomStats()
        _check(lib().scal_odom_step(self.h, _p(a[0], _f32p), a[0].shape[0], _p(a[1], _f32p), a[1].shape[0], _p(a[2], _f32p), a[2].shape[0],
                                    _p(a[3], _f32p), a[3].shape[0], _p(qlc, _f64p), _p(tlc, _f64p), _p(qw, _f64p), _p(tw, _f64p), C.byref(st)))
        return qlc, tlc, qw, tw, st

    def enqueue_features(self, feat):
        _check(lib().scal_odom_enqueue_features(self.h, feat.h))

    def collect(self):
        qlc, tlc, qw, tw = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        st = OdomStats()
        _check(lib().scal_odom_collect(self.h, _p(qlc, _f64p), _p(tlc, _f64p), _p(qw, _f64p), _p(tw, _f64p), C.byref(st)))
        return qlc, tlc, qw, tw, st

    # ---- Ceres-adapter mode (the caller owns the solver)
    def adapter_begin(self, sharp, less_sharp, flat, less_flat):
        a = [_f32(x).reshape(-1, 4) for x in (sharp, less_sharp, flat, less_flat)]
        q, t, need = np.zeros(4), np.zeros(3), C.c_int(0)
        _check(lib().scal_odom_adapter_begin(self.h, _p(a[0], _f32p), a[0].shape[0], _p(a[1], _f32p), a[1].shape[0], _p(a[2], _f32p), a[2].shape[0],
                                             _p(a[3], _f32p), a[3].shape[0], _p(q, _f64p), _p(t, _f64p), C.byref(need)))
        return q, t, bool(need.value)

    def adapter_finish(self, q_lc, t_lc):
        qw, tw = np.zeros(4), np.zeros(3)
        _check(lib().scal_odom_adapter_finish(self.h, _p(_f64(q_lc), _f64p), _p(_f64(t_lc), _f64p), _p(qw, _f64p), _p(tw, _f64p)))
        return qw, tw

    def step_features(self, feat):
        qlc, tlc, qw, tw = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        st = OdomStats()
        _check(lib().scal_odom_step_features(self.h, feat.h, _p(qlc, _f64p), _p(tlc, _f64p), _p(qw, _f64p), _p(tw, _f64p), C.byref(st)))
        return qlc, tlc, qw, tw, st


class LoopICP:
    """pcl::IterativeClosestPoint as doICPVirtualRelative configures it (laserPosegraphOptimization.cpp:518-531)."""

    def __init__(self, max_source=200000, max_target=2000000, max_corr_dist=150.0, max_iterations=100, transformation_epsilon=1e-6,
                 fitness_epsilon=1e-6, device=0):
        self.h = C.c_void_p()
        cfg = ICPConfig(max_corr_dist, transformation_epsilon, fitness_epsilon, max_iterations, max_source, max_target, device)
        _check(lib().scal_icp_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_icp_destroy(self.h)
        self.h = None

    __del__ = close

    def align_device(self, d_src_ptr, n_src, d_tgt_ptr, n_tgt, guess=None):
        """the clouds as 16-byte xyzi records in device memory; guess as in align (scal_icp_align_guess_device)"""
        r = ICPResult()
        if guess is None:
            _check(lib().scal_icp_align_device(self.h, d_src_ptr, n_src, d_tgt_ptr, n_tgt, C.byref(r)))
        else:
            g = self._guess(guess)
            _check(lib().scal_icp_align_guess_device(self.h, d_src_ptr, n_src, d_tgt_ptr, n_tgt, _p(g, _f32p), C.byref(r)))
        return dict(converged=bool(r.converged), iterations=r.iterations, state=r.state, n_correspondences=r.n_correspondences,
                    fitness=r.fitness, T=np.array(r.T[:]).reshape(4, 4))

    def set_search(self, mode):
        """1 (default): cell grid + dense sweep for unresolved queries; 0: dense sweep only.  Same result."""
        _check(lib().scal_icp_set_search(self.h, mode))

    def align(self, src, tgt, guess=None):
        """guess: a 4x4 initial transformation (pcl's align(output, guess)); None = the identity"""
        s, t = _f32(src), _f32(tgt)
        r = ICPResult()
        if guess is None:
            _check(lib().scal_icp_align(self.h, _p(s, _f32p), s.shape[0], _p(t, _f32p), t.shape[0], C.byref(r)))
        else:
            g = _f32(np.asarray(guess).reshape(16))
            _check(lib().scal_icp_align_guess(self.h, _p(s, _f32p), s.shape[0], _p(t, _f32p), t.shape[0], _p(g, _f32p), C.byref(r)))
        return dict(converged=bool(r.converged), iterations=r.iterations, state=r.state, n_correspondences=r.n_correspondences,
                    fitness=r.fitness, T=np.array(r.T[:]).reshape(4, 4))

    @staticmethod
    def _plane_dict(r):
        return dict(converged=bool(r.converged), iterations=r.iterations, state=r.state, n_correspondences=r.n_correspondences,
                    fitness=r.fitness, plane_fitness=r.plane_fitness, T=np.array(r.T[:]).reshape(4, 4), normal_eq=np.array(r.normal_eq[:]),
                    first_eq=np.array(r.first_eq[:]))

    @staticmethod
    def _guess(guess):
        if guess is None:
            return None
        g = np.asarray(guess)
        if g.size != 16:
            raise ValueError("the guess is a 4x4 matrix")
        return _f32(g.reshape(16))

    def align_plane(self, src, tgt, tgt_nc, guess=None):
        """Point-to-plane ICP (scal_icp_align_plane): tgt_nc [n_tgt, 4] is the target's normals and curvatures as
        RadiusIndex.normals* returns them.  The CPU restatement is scaloam.icp_plane.align_plane."""
        s, t, nc = _f32(src), _f32(tgt), _f32(tgt_nc)
        if nc.shape != (t.shape[0], 4):
            raise ValueError("tgt_nc is [n_tgt, 4]: one normal and curvature per target point")
        g = self._guess(guess)
        r = ICPPlaneResult()
        _check(lib().scal_icp_align_plane(self.h, _p(s, _f32p), s.shape[0], _p(t, _f32p), _p(nc, _f32p), t.shape[0], _p(g, _f32p), C.byref(r)))
        return self._plane_dict(r)

    def align_plane_device(self, d_src_ptr, n_src, d_tgt_ptr, d_nc_ptr, n_tgt, guess=None):
        g = self._guess(guess)
        r = ICPPlaneResult()
        _check(lib().scal_icp_align_plane_device(self.h, d_src_ptr, n_src, d_tgt_ptr, d_nc_ptr, n_tgt, _p(g, _f32p), C.byref(r)))
        return self._plane_dict(r)


class MultiviewRefine:
    """scal_refine: all keyframes of a session aligned at once, each by point-to-point ICP against the points of all the others, in
    Jacobi rounds (include/scaloam_hip.h).  The ICP settings are the reference's (laserPosegraphOptimization.cpp:518-531) except
    max_corr_dist: 2 m instead of 150 m, which across a whole session pairs every point with something however far (the header has
    the numbers)."""

    def __init__(self, max_frames, max_points, max_corr_dist=2.0, max_iterations=100, transformation_epsilon=1e-6, fitness_epsilon=1e-6,
                 fitness_gate=0.3, device=0):
        self.h = C.c_void_p()
        cfg = RefineConfig(max_corr_dist, transformation_epsilon, fitness_epsilon, fitness_gate, max_iterations, int(max_frames),
                           int(max_points), device)
        _check(lib().scal_refine_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_refine_destroy(self.h)
        self.h = None

    __del__ = close

    def _run(self, fn, ptr, offsets, poses12, fixed, rounds, near_thres, nc_ptr=None):
        """nc_ptr: the normals beside the records - fn is one of the scal_refine_run_plane* calls"""
        plane = nc_ptr is not None
        off = np.ascontiguousarray(offsets, np.int32)
        k = off.shape[0] - 1
        P = np.array(poses12, np.float64).reshape(-1, 12).copy()
        if k < 0 or P.shape[0] != k:
            raise ValueError("one pose12 row per frame and offsets of n_frames + 1 entries are needed")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
            if fx.shape[0] != k:
                raise ValueError("one fixed flag per frame is needed")
        res = ((RefinePlaneFrameResult if plane else RefineFrameResult) * max(k, 1))()
        run = C.c_int(0)
        tail = (_p(off, _i32p), k, _p(P, _f64p), fx.ctypes.data_as(C.c_char_p) if fx is not None else None, float(near_thres), int(rounds),
                res, C.byref(run))
        _check(fn(self.h, ptr, nc_ptr, *tail) if plane else fn(self.h, ptr, *tail))
        out = [dict(converged=bool(r.converged), iterations=r.iterations, state=r.state, n_correspondences=r.n_correspondences,
                    accepted=bool(r.accepted), fitness=r.fitness, T=np.array(r.T[:]).reshape(4, 4)) for r in res[:k]]
        if plane:
            for d, r in zip(out, res[:k]):
                d.update(plane_fitness=r.plane_fitness, normal_eq=np.array(r.normal_eq[:]), first_eq=np.array(r.first_eq[:]))
        return P, out, run.value

    def refine(self, frames, poses12, fixed=None, rounds=1, near_thres=2.0):
        """frames: a list of [n, 4] xyzi arrays in their local frames; returns (poses12 [K, 12], per-frame dicts, rounds_run)"""
        fs = [_f32(f).reshape(-1, 4) for f in frames]
        off = np.zeros(len(fs) + 1, np.int64)
        off[1:] = np.cumsum([f.shape[0] for f in fs])
        if off[-1] > 2**31 - 1:
            raise ValueError("more points than 32-bit offsets hold")
        cat = np.ascontiguousarray(np.concatenate(fs, 0)) if fs else np.zeros((0, 4), np.float32)
        return self._run(lib().scal_refine_run, cat.ctypes.data_as(C.c_void_p), off, poses12, fixed, rounds, near_thres)

    def refine_device(self, d_xyzi_ptr, offsets, poses12, fixed=None, rounds=1, near_thres=2.0):
        """the frames as 16-byte xyzi records back to back in device memory, frame f = records [offsets[f], offsets[f+1])"""
        return self._run(lib().scal_refine_run_device, d_xyzi_ptr, offsets, poses12, fixed, rounds, near_thres)

    def refine_plane(self, frames, normals, poses12, fixed=None, rounds=1, near_thres=2.0):
        """The refine with the point-to-plane metric (scal_refine_run_plane).  normals: per frame the [n, 4] normals and curvatures of
        its points among themselves, in the frame's local coordinates, as RadiusIndex.normals_self or
        scaloam.refine_plane.frame_normals give them; computed once, they serve every round and every pose.  The dicts carry
        plane_fitness, normal_eq and first_eq besides refine's fields.  The CPU restatement is scaloam.refine_plane.refine_plane."""
        fs, ns = [_f32(f).reshape(-1, 4) for f in frames], [_f32(a).reshape(-1, 4) for a in normals]
        if len(ns) != len(fs) or any(a.shape[0] != f.shape[0] for a, f in zip(ns, fs)):
            raise ValueError("one [n, 4] array of normals per frame, one row per point, is needed")
        off = np.zeros(len(fs) + 1, np.int64)
        off[1:] = np.cumsum([f.shape[0] for f in fs])
        if off[-1] > 2**31 - 1:
            raise ValueError("more points than 32-bit offsets hold")
        cat = np.ascontiguousarray(np.concatenate(fs, 0)) if fs else np.zeros((0, 4), np.float32)
        ncat = np.ascontiguousarray(np.concatenate(ns, 0)) if ns else np.zeros((0, 4), np.float32)
        return self._run(lib().scal_refine_run_plane, cat.ctypes.data_as(C.c_void_p), off, poses12, fixed, rounds, near_thres,
                         ncat.ctypes.data_as(C.c_void_p))

    def refine_plane_device(self, d_xyzi_ptr, d_nc_ptr, offsets, poses12, fixed=None, rounds=1, near_thres=2.0):
        """records and normals back to back in device memory, frame f = rows [offsets[f], offsets[f+1]) of both"""
        return self._run(lib().scal_refine_run_plane_device, d_xyzi_ptr, offsets, poses12, fixed, rounds, near_thres, C.c_void_p(d_nc_ptr))


def yaw_guess(yaw_rad):
    """Rz(-yaw) as scal_reloc builds it from a search's f32 yaw: cos and sin in double, rounded to f32"""
    y = float(np.float32(yaw_rad))
    c, s = np.float32(np.cos(y)), np.float32(np.sin(y))
    return np.array([[c, s, 0, 0], [-s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)


def relative_transform(pose12_c, pose12_j):
    """M = P_c^-1 P_j as scal_reloc computes it for a submap keyframe: f64, every sum left to right, rounded to an f32 3x4"""
    Pc, Pj = np.asarray(pose12_c, np.float64).reshape(3, 4), np.asarray(pose12_j, np.float64).reshape(3, 4)
    Ri = Pc[:, :3].T
    ti = -((Ri[:, 0] * Pc[0, 3] + Ri[:, 1] * Pc[1, 3]) + Ri[:, 2] * Pc[2, 3])
    M = (Ri[:, 0:1] * Pj[0:1, :] + Ri[:, 1:2] * Pj[1:2, :]) + Ri[:, 2:3] * Pj[2:3, :]
    M[:, 3] += ti
    return M.astype(np.float32)


class Relocalizer:
    """scal_reloc: one saved session (per keyframe its Scans/ cloud, its optimized pose, its descriptor) in device memory; query() finds
    the place of a new scan by the between-session ScanContext search and verifies it by ICP from the search's yaw against a submap of
    the keyframes around the candidate (include/scaloam_hip.h has the steps).  0 = the reference's default for every setting."""

    def __init__(self, max_keyframes, max_points, max_query_points=400000, sc_max_radius=0.0, sc_dist_thres=0.0, float_math=0, leaf=0.0,
                 submap_half=0, fitness_thres=0.0, max_corr_dist=0.0, transformation_epsilon=0.0, fitness_epsilon=0.0, max_iterations=0,
                 no_yaw_guess=False, device=0):
        self.h = C.c_void_p()
        cfg = RelocConfig(int(max_keyframes), int(max_points), int(max_query_points), sc_max_radius, sc_dist_thres, float_math, leaf,
                          int(submap_half), fitness_thres, max_corr_dist, transformation_epsilon, fitness_epsilon, int(max_iterations),
                          1 if no_yaw_guess else 0, device)
        _check(lib().scal_reloc_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_reloc_destroy(self.h)
        self.h = None

    __del__ = close

    def size(self):
        return lib().scal_reloc_size(self.h)

    def sc(self):
        """the session's ScanContext database as a borrowed SCManager (valid while this object lives)"""
        return _borrow(SCManager, lib().scal_reloc_sc(self.h))

    def add_keyframe(self, xyzi, pose12, desc=None):
        """one keyframe in its local frame with its row of optimized_poses.txt; desc: a reloaded [ring, sector] descriptor (formats.read_scd),
        None = built from the filtered cloud.  Returns the keyframe index."""
        x = _f32(xyzi).reshape(-1, 4)
        P = _f64(np.asarray(pose12).reshape(-1)[:12])
        d = _f64(np.asarray(desc).T.reshape(-1)) if desc is not None else None
        j = lib().scal_reloc_add_keyframe(self.h, _p(x, _f32p), x.shape[0], _p(P, _f64p), _p(d, _f64p))
        if j < 0:
            _check(j)
        return j

    @staticmethod
    def _result(r):
        return dict(status=r.status, sc=SCManager._result(r.sc), n_src=r.n_src, n_tgt=r.n_tgt,
                    icp=dict(converged=bool(r.icp.converged), iterations=r.icp.iterations, state=r.icp.state,
                             n_correspondences=r.icp.n_correspondences, fitness=r.icp.fitness, T=np.array(r.icp.T[:]).reshape(4, 4)),
                    pose12=np.array(r.pose12[:]))

    def query(self, xyzi):
        x = _f32(xyzi).reshape(-1, 4)
        r = RelocResult()
        _check(lib().scal_reloc_query(self.h, _p(x, _f32p), x.shape[0], C.byref(r)))
        return self._result(r)

    def query_batch(self, clouds):
        cs = [_f32(c).reshape(-1, 4) for c in clouds]
        off = np.zeros(len(cs) + 1, np.int64)
        off[1:] = np.cumsum([c.shape[0] for c in cs])
        if off[-1] > 2**31 - 1:
            raise ValueError("more points than 32-bit offsets hold")
        off = off.astype(np.int32)
        cat = np.ascontiguousarray(np.concatenate(cs, 0)) if cs else np.zeros((0, 4), np.float32)
        res = (RelocResult * max(1, len(cs)))()
        _check(lib().scal_reloc_query_batch(self.h, _p(cat, _f32p), _p(off, _i32p), len(cs), res))
        return [self._result(r) for r in res[:len(cs)]]


class Removert:
    """scal_removert: dynamic-point removal from a merged keyframe map.  A keyframe whose ray passes through the place of a map point
    hits it; a point is dynamic when some remove resolution has min_hits hits and every revert resolution has one
    (include/scaloam_hip.h has the projection, scaloam/removert.py the CPU restatement the device equals bit for bit).  A session
    longer than max_keyframes, or with more scan points than max_scan_points, is run in chunks with the same result."""

    def __init__(self, max_points, max_keyframes, max_scan_points, max_resolutions=4, fov_up_deg=25.0, fov_down_deg=-25.0, min_range=0.5,
                 max_range=80.0, diff_thres=0.1, min_hits=1, min_res_deg=0.0, cell_size=0.0, device=0):
        self.h = C.c_void_p()
        self.fov = (float(fov_up_deg), float(fov_down_deg))
        cfg = RemovertConfig(int(max_points), int(max_keyframes), int(max_scan_points), int(max_resolutions), int(min_hits), device,
                             fov_up_deg, fov_down_deg, min_range, max_range, diff_thres, min_res_deg, cell_size)
        _check(lib().scal_removert_create(C.byref(cfg), C.byref(self.h)))
        self.n = 0
        self.res = ()

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_removert_destroy(self.h)
        self.h = None

    __del__ = close

    def set_map(self, map_xyzi):
        m = _f32(map_xyzi).reshape(-1, 4)
        _check(lib().scal_removert_set_map(self.h, _p(m, _f32p), m.shape[0]))
        self.n = m.shape[0]

    def set_map_device(self, d_xyzi_ptr, n):
        """n 16-byte xyzi records in device memory; they are used in place and must stay valid until the next set_map"""
        _check(lib().scal_removert_set_map_device(self.h, d_xyzi_ptr, int(n)))
        self.n = int(n)

    def run(self, scans, poses12, remove_res=(2.5, 2.0, 1.5), revert_res=(5.0,), want_hits=False):
        """on the map set last; returns (mask uint8 [n], stats dict[, hits uint16 [n] at the finest remove resolution])"""
        cs = [_f32(s).reshape(-1, 4) for s in scans]
        off = np.zeros(len(cs) + 1, np.int64)
        off[1:] = np.cumsum([s.shape[0] for s in cs])
        if off[-1] > 2**31 - 1:
            raise ValueError("more points than 32-bit offsets hold")
        off = off.astype(np.int32)
        P = _f64(np.asarray(poses12, np.float64).reshape(-1, 12))
        if P.shape[0] != len(cs):
            raise ValueError("one pose12 row per scan is needed")
        cat = np.ascontiguousarray(np.concatenate(cs, 0)) if cs else np.zeros((0, 4), np.float32)
        rm, rv = _f64(np.asarray(remove_res, np.float64).reshape(-1)), _f64(np.asarray(revert_res, np.float64).reshape(-1))
        mask = np.zeros(max(self.n, 1), np.uint8)
        hits = np.zeros(max(self.n, 1), np.uint16) if want_hits else None
        st = RemovertStats()
        _check(lib().scal_removert_run(self.h, _p(cat, _f32p), _p(off, _i32p), len(cs), _p(P, _f64p), _p(rm, _f64p), rm.shape[0], _p(rv, _f64p),
                                       rv.shape[0], _p(mask, C.POINTER(C.c_ubyte)), _p(hits, C.POINTER(C.c_ushort)), C.byref(st)))
        self.res = tuple(rm) + tuple(rv)
        stats = dict(points=st.points, keyframes=st.keyframes, dynamic=st.dynamic, pairs_tested=st.pairs_tested,
                     pairs_bruteforce=st.pairs_bruteforce)
        return (mask[:self.n], stats, hits[:self.n]) if want_hits else (mask[:self.n], stats)

    def remove(self, map_xyzi, scans, poses12, remove_res=(2.5, 2.0, 1.5), revert_res=(5.0,), want_hits=False):
        self.set_map(map_xyzi)
        return self.run(scans, poses12, remove_res, revert_res, want_hits)

    def remove_device(self, mapmerge, scans, poses12, remove_res=(2.5, 2.0, 1.5), revert_res=(5.0,), want_hits=False):
        """on the points a MapMerge holds in device memory (they never leave it); size() waits for the merge"""
        self.set_map_device(mapmerge.device_points(), mapmerge.size())
        return self.run(scans, poses12, remove_res, revert_res, want_hits)

    def scan_image(self, k, i):
        """keyframe k's [H, W] range image at resolution i of the last run (remove resolutions first), +inf where empty"""
        if not 0 <= i < len(self.res):
            raise ValueError("no such resolution in the last run")
        from . import removert as _rv
        H, W = _rv.image_shape(self.res[i], *self.fov)
        out = np.zeros((H, W), np.float32)
        _check(lib().scal_removert_scan_image(self.h, int(k), int(i), _p(out, _f32p), H, W))
        return out

    def compact(self, which):
        """the static (0) or dynamic (1) points of the last run, in input order"""
        m = C.c_int(0)
        out = np.zeros((max(self.n, 1), 4), np.float32)
        _check(lib().scal_removert_compact(self.h, int(which), _p(out, _f32p), self.n, C.byref(m)))
        return out[:m.value].copy()


class RadiusIndex:
    """scal_nbr: per query the number of index records within r (uint16, saturating) and the smallest f32 d^2 among them (+inf when
    none) - include/scaloam_hip.h has the definition, scaloam/nbr.py the CPU restatement the device equals bit for bit.  A query
    set larger than max_query_points goes through in chunks; the result does not depend on the chunking.  knn / knn_self / knn_device
    give the k nearest of those records per query, ordered by (d2, input position), on the same index (scaloam.nbr.knn_within);
    normals / normals_self / normals_device the plane through them - normal, curvature, signed distance (scaloam.nbr.normals_within)."""

    def __init__(self, max_index_points, max_query_points, device=0):
        self.h = C.c_void_p()
        self.max_query_points = int(max_query_points)
        cfg = NbrConfig(device, int(max_index_points), int(max_query_points))
        _check(lib().scal_nbr_create(C.byref(cfg), C.byref(self.h)))
        self.n = 0

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_nbr_destroy(self.h)
        self.h = None

    __del__ = close

    def set_index(self, xyzi, r):
        a = _f32(xyzi).reshape(-1, 4)
        _check(lib().scal_nbr_set_index(self.h, _p(a, _f32p), a.shape[0], float(r)))
        self.n = a.shape[0]

    def set_index_device(self, mapmerge, r):
        """the points a MapMerge holds in device memory; size() waits for the merge"""
        n = mapmerge.size()
        _check(lib().scal_nbr_set_index_device(self.h, mapmerge.device_points(), n, float(r)))
        self.n = n

    def _chunked(self, n, call):
        """call(i, m) for every chunk [i, i + m) of n queries, at most max_query_points each (one empty chunk when n is 0); stats()
        afterwards covers all chunks"""
        pairs, items = 0, 0
        for i in range(0, max(n, 1), self.max_query_points):
            m = min(self.max_query_points, n - i)
            _check(call(i, m))
            st = self._stats()
            pairs, items = pairs + st[0], items + st[1]
        self._sum = (pairs, items)

    def _single(self, rc):
        """after a call that is not chunked (self and device queries): stats() is that call's"""
        _check(rc)
        self._sum = self._stats()

    def query(self, xyzi):
        """(count uint16 [n], min_d2 float32 [n]); stats() afterwards covers all chunks"""
        q = _f32(xyzi).reshape(-1, 4)
        n = q.shape[0]
        count, d2 = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.float32)
        self._chunked(n, lambda i, m: lib().scal_nbr_query(self.h, _p(q[i:i + m], _f32p), m, _p(count[i:], C.POINTER(C.c_ushort)), _p(d2[i:], _f32p)))
        return count[:n], d2[:n]

    def query_self(self):
        count, d2 = np.zeros(max(self.n, 1), np.uint16), np.zeros(max(self.n, 1), np.float32)
        self._single(lib().scal_nbr_query_self(self.h, _p(count, C.POINTER(C.c_ushort)), _p(d2, _f32p)))
        return count[:self.n], d2[:self.n]

    def query_device(self, d_xyzi_ptr, n, d_count_ptr, d_min_d2_ptr):
        """queries and outputs in device memory (either output may be None); at most max_query_points"""
        self._single(lib().scal_nbr_query_device(self.h, d_xyzi_ptr, int(n), d_count_ptr, d_min_d2_ptr))

    @staticmethod
    def _rows(n, k):
        kk = min(max(k, 1), NBR_MAX_K)   # the buffers' width; a k out of range is the library's to refuse
        return np.zeros((max(n, 1), kk), np.int32), np.zeros((max(n, 1), kk), np.float32)

    def knn(self, xyzi, k):
        """(idx int32 [n, k], d2 float32 [n, k]): per query its k nearest index records within r by (d2, input position), padded with
        -1 / +inf; chunked by max_query_points, and stats() afterwards covers all chunks"""
        q = _f32(xyzi).reshape(-1, 4)
        n, k = q.shape[0], int(k)
        idx, d2 = self._rows(n, k)
        self._chunked(n, lambda i, m: lib().scal_nbr_knn(self.h, _p(q[i:i + m], _f32p), m, k, _p(idx[i:], _i32p), _p(d2[i:], _f32p)))
        return idx[:n], d2[:n]

    def knn_self(self, k):
        """the index records as the queries, rows in the order the index was given in"""
        idx, d2 = self._rows(self.n, int(k))
        self._single(lib().scal_nbr_knn_self(self.h, int(k), _p(idx, _i32p), _p(d2, _f32p)))
        return idx[:self.n], d2[:self.n]

    def knn_device(self, d_xyzi_ptr, n, k, d_idx_ptr, d_d2_ptr):
        """queries and the [n, k] outputs in device memory (either output may be None); at most max_query_points"""
        self._single(lib().scal_nbr_knn_device(self.h, d_xyzi_ptr, int(n), int(k), d_idx_ptr, d_d2_ptr))

    @staticmethod
    def _viewpoint(viewpoint):
        if viewpoint is None:
            return None, None
        v = np.ascontiguousarray(viewpoint, np.float64).reshape(3)
        return v, _p(v, _f64p)

    def normals(self, xyzi, k, viewpoint=None):
        """(nc float32 [n, 4], dist float32 [n]): per query the unit normal and the curvature of the plane through its k nearest index
        records within r, and the query's signed distance to that plane (scaloam.nbr.normals_within); NaN where fewer than 3 records
        are within r.  viewpoint: three numbers the normals are turned towards, or None.  Chunked by max_query_points, and stats()
        afterwards covers all chunks"""
        q = _f32(xyzi).reshape(-1, 4)
        n, k = q.shape[0], int(k)
        nc, dist = np.zeros((max(n, 1), 4), np.float32), np.zeros(max(n, 1), np.float32)
        v, vptr = self._viewpoint(viewpoint)
        self._chunked(n, lambda i, m: lib().scal_nbr_normals(self.h, _p(q[i:i + m], _f32p), m, k, vptr, _p(nc[i:], _f32p), _p(dist[i:], _f32p)))
        return nc[:n], dist[:n]

    def normals_self(self, k, viewpoint=None):
        """the index records as the queries, outputs in the order the index was given in"""
        nc, dist = np.zeros((max(self.n, 1), 4), np.float32), np.zeros(max(self.n, 1), np.float32)
        v, vptr = self._viewpoint(viewpoint)
        self._single(lib().scal_nbr_normals_self(self.h, int(k), vptr, _p(nc, _f32p), _p(dist, _f32p)))
        return nc[:self.n], dist[:self.n]

    def normals_device(self, d_xyzi_ptr, n, k, d_nc_ptr, d_dist_ptr, viewpoint=None):
        """queries and the [n, 4] / [n] outputs in device memory (either output may be None); at most max_query_points"""
        v, vptr = self._viewpoint(viewpoint)
        self._single(lib().scal_nbr_normals_device(self.h, d_xyzi_ptr, int(n), int(k), vptr, d_nc_ptr, d_dist_ptr))

    def _stats(self):
        pairs, items = C.c_longlong(0), C.c_int(0)
        _check(lib().scal_nbr_stats(self.h, C.byref(pairs), C.byref(items)))
        return pairs.value, items.value

    def stats(self):
        """of the last query: dict(pairs_tested, work_items)"""
        pairs, items = getattr(self, "_sum", (0, 0))
        return dict(pairs_tested=pairs, work_items=items)


class MapMerge:
    """Offline dense map merge (utils/python/makeMergedMap.py:83-133): transform, near-range removal, concatenation."""

    def __init__(self, max_points=40000000, max_frame_points=400000, device=0):
        self.h = C.c_void_p()
        cfg = MapMergeConfig(max_points, max_frame_points, device)
        _check(lib().scal_mapmerge_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_mapmerge_destroy(self.h)
        self.h = None

    __del__ = close

    def reset(self):
        _check(lib().scal_mapmerge_reset(self.h))

    def add(self, xyzi, pose12, near_thres=2.0):
        a = _f32(xyzi)
        p = _f64(np.asarray(pose12).reshape(-1))
        _check(lib().scal_mapmerge_add(self.h, _p(a, _f32p), a.shape[0], _p(p, _f64p), float(near_thres)))

    def add_batch_device(self, d_ptr, offsets, poses12, near_thres=2.0):
        off = (C.c_int * len(offsets))(*[int(v) for v in offsets])
        p = _f64(np.asarray(poses12).reshape(-1))
        _check(lib().scal_mapmerge_add_batch_device(self.h, d_ptr, off, _p(p, _f64p), len(offsets) - 1, float(near_thres)))

    def size(self):
        n = lib().scal_mapmerge_size(self.h)
        if n < 0:
            _check(int(n))
        return int(n)

    def download(self):
        n = self.size()
        out = np.zeros((max(n, 1), 4), np.float32)
        _check(lib().scal_mapmerge_download(self.h, _p(out, _f32p), n))
        return out[:n]

    def downsample(self, leaf):
        n = self.size()
        out = np.zeros((max(n, 1), 4), np.float32)
        m = C.c_longlong(0)
        _check(lib().scal_mapmerge_downsample(self.h, C.c_float(leaf), _p(out, _f32p), n, C.byref(m)))
        return out[:m.value].copy()

    def device_points(self):
        return lib().scal_mapmerge_device_points(self.h)


def factors_eval(kind, cp, pa, pb, x7, device=0):
    kind = np.ascontiguousarray(kind, np.int32)
    cp, pa, pb, x7 = _f64(cp), _f64(pa), _f64(pb), _f64(x7)
    cost = np.zeros(1)
    g = np.zeros(6)
    H = np.zeros((6, 6))
    _check(lib().scal_factors_eval(device, kind.shape[0], _p(kind, _i32p), _p(cp, _f64p), _p(pa, _f64p), _p(pb, _f64p), _p(x7, _f64p),
                                   _p(cost, _f64p), _p(g, _f64p), _p(H, _f64p)))
    return cost[0], g, H


def _pg_stats(s):
    return dict(iterations=s.iterations, converged=s.converged, initial_cost=s.initial_cost, final_cost=s.final_cost,
                linear_iterations=s.linear_iterations, linear_status=s.linear_status, last_step_max=s.last_step_max)


class PoseGraph:
    """scal_posegraph: batch pose-graph optimisation on the GPU (one prior, between edges, Cauchy-robust where cauchy_k > 0); poses are
    pose7 rows qx qy qz qw tx ty tz.  scaloam.pgo.optimize_pose_graph is its CPU restatement."""

    def __init__(self, max_nodes, max_edges, device=0):
        self.h = C.c_void_p()
        cfg = PoseGraphConfig(device, int(max_nodes), int(max_edges))
        _check(lib().scal_posegraph_create(C.byref(cfg), C.byref(self.h)))
        self.n_nodes, self.n_edges = 0, 0

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_posegraph_destroy(self.h)
        self.h = None

    __del__ = close

    def set_nodes(self, pose7):
        P = _f64(np.asarray(pose7, np.float64).reshape(-1, 7))
        _check(lib().scal_posegraph_set_nodes(self.h, _p(P, _f64p), P.shape[0]))
        self.n_nodes = P.shape[0]

    def set_prior(self, node, pose7, variances6):
        P, V = _f64(np.asarray(pose7, np.float64).reshape(7)), _f64(np.asarray(variances6, np.float64).reshape(6))
        _check(lib().scal_posegraph_set_prior(self.h, int(node), _p(P, _f64p), _p(V, _f64p)))

    def add_between(self, i, j, pose7_rel, variances6, cauchy_k=None):
        i = np.ascontiguousarray(np.asarray(i, np.int32).reshape(-1))
        j = np.ascontiguousarray(np.asarray(j, np.int32).reshape(-1))
        m = i.shape[0]
        Z = _f64(np.asarray(pose7_rel, np.float64).reshape(-1, 7))
        V = _f64(np.broadcast_to(np.asarray(variances6, np.float64), (m, 6)))
        K = None if cauchy_k is None else _f64(np.broadcast_to(np.asarray(cauchy_k, np.float64), (m,)))
        if j.shape[0] != m or Z.shape[0] != m:
            raise ValueError("one j and one pose7 per edge")
        _check(lib().scal_posegraph_add_between(self.h, m, _p(i, _i32p), _p(j, _i32p), _p(Z, _f64p), _p(V, _f64p), _p(K, _f64p)))
        self.n_edges += m

    def add_edges(self, edges):
        """edges as scaloam.pgo.make_edges builds them"""
        self.add_between(edges["i"], edges["j"], edges["z"], edges["var"], edges["k"])

    def clear_edges(self):
        _check(lib().scal_posegraph_clear_edges(self.h))
        self.n_edges = 0

    def optimize(self, max_iterations=0, step_tol=0.0, max_linear_iterations=0, linear_rtol=0.0):
        """0 = the library's default; returns the statistics as a dict"""
        prm = PoseGraphParams(int(max_iterations), float(step_tol), int(max_linear_iterations), float(linear_rtol))
        st = PoseGraphStats()
        _check(lib().scal_posegraph_optimize(self.h, C.byref(prm), C.byref(st)))
        return _pg_stats(st)

    def nodes(self):
        out = np.zeros((self.n_nodes, 7))
        _check(lib().scal_posegraph_get_nodes(self.h, _p(out, _f64p), self.n_nodes))
        return out

    def edge_weights(self):
        out = np.zeros(max(self.n_edges, 1))
        _check(lib().scal_posegraph_get_edge_weights(self.h, _p(out, _f64p), self.n_edges))
        return out[:self.n_edges]


# ---------------------------------------------------------------------------------------------- the four stages as one object
SC_OFF, SC_EVERY_SCAN, SC_DESCRIPTOR, SC_KEYFRAME = 0, 1, 2, 3


class KeyframeGate:
    """scal_keyframe_gate: the pose-graph node's keyframe gate (laserPosegraphOptimization.cpp:598-617) in the library, host only (no GPU
    needed); the same decisions as scaloam.pgo.KeyframeGate.  gate(q_xyzw, t_xyz) -> True for a keyframe."""

    def __init__(self, meter_gap=2.0, deg_gap=10.0):
        self.st = KeyframeGateState()
        _check(lib().scal_keyframe_gate_init(C.byref(self.st), float(meter_gap), float(deg_gap)))

    def __call__(self, q_xyzw, t_xyz):
        q, t = _f64(np.asarray(q_xyzw, np.float64).reshape(4)), _f64(np.asarray(t_xyz, np.float64).reshape(3))
        k = C.c_int(0)
        _check(lib().scal_keyframe_gate(C.byref(self.st), q.ctypes.data_as(_f64p), t.ctypes.data_as(_f64p), C.byref(k)))
        return bool(k.value)


def _borrow(cls, handle):
    """A wrapper of `cls` around a context that somebody else (a Pipeline) owns: same methods, close() does nothing."""
    sub = type(cls.__name__ + "Borrowed", (cls,), {"close": lambda self: None, "__del__": lambda self: None})
    o = sub.__new__(sub)
    o.h = C.c_void_p(handle)
    return o


class Pipeline:
    """scal_pipeline: the reference's four nodes (scanRegistration, laserOdometry, laserMapping, laserPosegraphOptimization's
    ScanContext part) working on consecutive scans at the same time, scheduled inside the library.  push() a scan, pop() poses in order."""

    def __init__(self, lidar_type, minimum_range, max_points=400000, line_res=0.4, plane_res=0.8, max_map_points=4000000, sc_mode=SC_EVERY_SCAN,
                 sc_max_radius=80.0, sc_dist_thres=0.2, sc_max_keyframes=8192, device=0, ring=0, depth=0, float_math=0, check_finite=1, d_desc_ring=None,
                 n_seqs=1, keyframe_meter_gap=0, keyframe_deg_gap=0, kf_max_points=0, loop_fitness_thres=0, pgo_map_max_points=0):
        """sc_mode=SC_KEYFRAME: the pose-graph node's keyframe path - keyframe gate (0 = 2 m / 10 deg), keyframe clouds kept in a store of
        kf_max_points points (0 = none, no loop is verified), loops verified by ICP (loop_fitness_thres 0 = 0.3): pop_loop(), keyframe();
        the caller's optimized poses go in with update_keyframe_poses(), the pose-graph map of up to pgo_map_max_points points (before
        its filter; 0 = no map) comes out of pgo_map()."""
        self.cfg = PipelineConfig(lidar_type, SCAN_LINES.get(lidar_type, 0), float(minimum_range), max_points, float_math, check_finite, line_res,
                                  plane_res, max_map_points, sc_max_radius, sc_dist_thres, sc_max_keyframes, sc_mode, device, ring, depth, d_desc_ring,
                                  float(keyframe_meter_gap), float(keyframe_deg_gap), int(kf_max_points), float(loop_fitness_thres),
                                  int(pgo_map_max_points))
        self.h = C.c_void_p()
        self._kf_end = 0  # 1 + the largest keyframe_id popped so far
        self._map_buf = np.zeros((0, 4), np.float32)
        self.n_seqs = n_seqs
        _check(lib().scal_pipeline_create_multi(C.byref(self.cfg), n_seqs, C.byref(self.h)))
        self.scs = [_borrow(SCManager, lib().scal_pipeline_sc_of(self.h, q)) if sc_mode != SC_OFF else None for q in range(n_seqs)]
        self.maps = [_borrow(LaserMapping, lib().scal_pipeline_map_of(self.h, q)) for q in range(n_seqs)]
        self.sc, self.map = self.scs[0], self.maps[0]
        self.odom = _borrow(LaserOdometry, lib().scal_pipeline_odom(self.h))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.scal_pipeline_destroy(self.h)
        self.h = None

    __del__ = close

    def push_device(self, d_ptr, n, stride_floats=3):
        _check(lib().scal_pipeline_push_device(self.h, C.c_void_p(d_ptr), n, stride_floats))

    def push(self, xyz):
        a = _f32(xyz)
        _check(lib().scal_pipeline_push_host(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], a.strides[0]))

    @staticmethod
    def _res(r):
        return dict(seq=r.seq, q=np.array(r.q_w_curr[:]), t=np.array(r.t_w_curr[:]), q_odom=np.array(r.q_odom[:]), t_odom=np.array(r.t_odom[:]),
                    odom=r.odom, map=r.map, loop=SCManager._result(r.loop) if r.have_loop else None, d_descriptor=r.d_descriptor,
                    is_keyframe=bool(r.is_keyframe), keyframe_id=r.keyframe_id)

    def pop(self):
        r = PipelineResult()
        _check(lib().scal_pipeline_pop(self.h, C.byref(r)))
        self._kf_end = max(self._kf_end, r.keyframe_id + 1)
        return self._res(r)

    def push_device_multi(self, d_ptrs, ns, stride_floats=3):
        """one scan of EVERY sequence (device pointers, point counts)"""
        pa = (C.c_void_p * self.n_seqs)(*[C.c_void_p(int(v)) for v in d_ptrs])
        na = (C.c_int * self.n_seqs)(*[int(v) for v in ns])
        _check(lib().scal_pipeline_push_device_multi(self.h, pa, na, stride_floats))

    def pop_multi(self):
        """the sequences' results of the oldest scan step not yet popped: a list of n_seqs dicts"""
        ra = (PipelineResult * self.n_seqs)()
        _check(lib().scal_pipeline_pop_multi(self.h, ra))
        return [self._res(ra[q]) for q in range(self.n_seqs)]

    def drain(self):
        _check(lib().scal_pipeline_drain(self.h))

    def pop_loop(self, wait=True):
        """sc_mode 3: the oldest verified / rejected loop record (dict), or None when none is ready (wait=False) or none is pending"""
        r = PipelineLoop()
        rc = lib().scal_pipeline_pop_loop(self.h, C.byref(r), 1 if wait else 0)
        _check(min(rc, 0))
        if rc == 0:
            return None
        return dict(seq=r.seq, curr_kf=r.curr_kf, loop_kf=r.loop_kf, yaw=r.yaw_rad, min_dist=r.min_dist, verified=r.verified,
                    converged=r.converged, iterations=r.iterations, state=r.state, fitness=r.fitness, T=np.array(r.T[:]).reshape(4, 4),
                    n_src=r.n_src, n_tgt=r.n_tgt, q_rel=np.array(r.q_rel[:]), t_rel=np.array(r.t_rel[:]))

    def keyframe(self, kf):
        """sc_mode 3, drained: (pose6 x y z roll pitch yaw, stored 0.4 m xyzi cloud) of keyframe kf (database index)"""
        pose = np.zeros(6)
        n = C.c_int(0)
        _check(lib().scal_pipeline_keyframe(self.h, kf, pose.ctypes.data_as(_f64p), None, 0, C.byref(n)))
        cloud = np.zeros((max(n.value, 1), 4), np.float32)
        _check(lib().scal_pipeline_keyframe(self.h, kf, pose.ctypes.data_as(_f64p), cloud.ctypes.data_as(_f32p), n.value, C.byref(n)))
        return pose, cloud[:n.value].copy()

    def update_keyframe_poses(self, ids, poses6):
        """sc_mode 3: the caller's optimized poses (x y z roll pitch yaw) of keyframes `ids` (database indices), as updatePoses writes
        them into keyframePosesUpdated; loops of scans pushed from now on are verified with them"""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        P = _f64(np.asarray(poses6, np.float64).reshape(-1, 6))
        if P.shape[0] != ids.shape[0]:
            raise ValueError("one pose6 per keyframe id")
        _check(lib().scal_pipeline_update_keyframe_poses(self.h, ids.ctypes.data_as(_i32p), P.ctypes.data_as(_f64p), ids.shape[0]))

    def pgo_map(self, kf_end=None, skip=2, leaf=0.4):
        """sc_mode 3: the pose-graph map (pubMap): every skip-th own keyframe with database index < kf_end (None: 1 + the largest
        keyframe_id popped so far) moved by its current pose, concatenated and filtered at `leaf`; an (n, 4) float32 xyzi array"""
        kf_end = self._kf_end if kf_end is None else int(kf_end)
        n = C.c_longlong(0)
        for _ in range(2):  # a map larger than the buffer: grow it and build the map again
            buf = self._map_buf
            _check(lib().scal_pipeline_pgo_map(self.h, kf_end, int(skip), float(leaf), buf.ctypes.data_as(_f32p) if buf.shape[0] else None,
                                               buf.shape[0], C.byref(n)))
            if n.value <= buf.shape[0]:
                break
            self._map_buf = np.zeros((n.value, 4), np.float32)
        return self._map_buf[:n.value].copy()

    def optimize_keyframes(self, kf_end=None, apply=True):
        """sc_mode 3: optimise the pose graph of the own keyframes with database index < kf_end (None: 1 + the largest keyframe_id popped
        so far) and the accepted loops among them on the GPU; apply=True also does update_keyframe_poses(ids, poses6).  Returns ids,
        poses6 (x y z roll pitch yaw), stats (n_nodes, n_odom_edges, n_loop_edges, applied + the solver's statistics)"""
        kf_end = self._kf_end if kf_end is None else int(kf_end)
        cap = max(int(self.cfg.sc_max_keyframes), 1)
        ids, P = np.zeros(cap, np.int32), np.zeros((cap, 6))
        res = PipelinePgoResult()
        _check(lib().scal_pipeline_optimize_keyframes(self.h, kf_end, 1 if apply else 0, _p(ids, _i32p), _p(P, _f64p), cap, C.byref(res)))
        st = dict(n_nodes=res.n_nodes, n_odom_edges=res.n_odom_edges, n_loop_edges=res.n_loop_edges, applied=res.applied)
        st.update(_pg_stats(res.solver))
        return ids[:res.n_nodes].copy(), P[:res.n_nodes].copy(), st

    def pgo_map_device(self):
        """(device pointer, n) of the last map pgo_map built; (None, 0) before the first"""
        n = C.c_longlong(0)
        ptr = lib().scal_pipeline_pgo_map_device(self.h, C.byref(n))
        return ptr, n.value

    def in_flight(self):
        return lib().scal_pipeline_in_flight(self.h)

    def features(self, i):
        return _borrow(ScanRegistration, lib().scal_pipeline_features(self.h, i))
