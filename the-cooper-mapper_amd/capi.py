"""ctypes binding of include/lslam_c.h (one declaration per exported symbol)."""
import ctypes as C
import enum
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_NAME = "liblslam_hip.so"

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class LslamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lslam status %d: %s" % (code, msg))
        self.code = code


class Status(enum.IntEnum):
    OK = 0
    TOO_FEW_REF = 1
    NOT_CONVERGED = 2
    LOW_SCORE = 3
    LOW_PERCENT = 4
    TOO_FEW_MATCHES = 5
    ERR_INVALID = -1
    ERR_HIP = -2
    ERR_NO_MAP = -3
    ERR_NO_SCAN = -4
    ERR_TREE_DEPTH = -5
    ERR_TREE_BUILD = -6
    ERR_COMM = -7


class LslamOpts(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("delta_t_abort", C.c_float),
        ("delta_r_abort", C.c_float),
        ("use_score", C.c_int32),
        ("fine_score", C.c_int32),
        ("score_threshold", C.c_double),
        ("match_percentage_threshold", C.c_double),
        ("jtj_mode", C.c_int32),
        ("profile", C.c_int32),
        ("scans_in_flight", C.c_int32),
        ("search_mode", C.c_int32),
        ("knn_cert", C.c_int32),
        ("cert_try_m", C.c_float),
        ("cert_track_m", C.c_float),
        ("grid_cell", C.c_float),
        ("debug_stats", C.c_int32),
        ("ab_switches", C.c_int32),
    ]


class LslamRegParams(C.Structure):
    """lslam_reg_params (include/lslam_c.h)."""
    _fields_ = [("n_feature_regions", C.c_int32), ("curvature_region", C.c_int32), ("max_corner_sharp", C.c_int32),
                ("max_surface_flat", C.c_int32), ("less_flat_filter_size", C.c_float),
                ("surface_curvature_threshold", C.c_float), ("blind_threshold", C.c_float), ("reserved", C.c_int32)]


class LslamStereoCam(C.Structure):
    """lslam_stereo_cam (include/lslam_c.h)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("T_cl", C.c_float * 12), ("weight", C.c_float), ("huber_stereo", C.c_float),
                ("huber_mono", C.c_float), ("gate_outliers", C.c_int32), ("min_depth", C.c_float)]


class LslamStats(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("iterations", C.c_int32),
        ("n_line", C.c_int32),
        ("n_plane", C.c_int32),
        ("n_rows", C.c_int32),
        ("degenerate", C.c_int32),
        ("converged", C.c_int32),
        ("delta_r", C.c_float),
        ("delta_t", C.c_float),
        ("score", C.c_double),
        ("percent", C.c_double),
        ("point_residuals", C.c_int64),
        ("sweeps", C.c_int32),
        ("sweep_launches", C.c_int32),
        ("gpu_ms_total", C.c_float),
        ("gpu_ms_sweep", C.c_float),
        ("score2", C.c_double),
        ("percent2", C.c_double),
    ]


class LslamMapInfo(C.Structure):
    _fields_ = [
        ("n_corner", C.c_uint64),
        ("n_surf", C.c_uint64),
        ("nodes_corner", C.c_uint32),
        ("nodes_surf", C.c_uint32),
        ("depth_corner", C.c_int32),
        ("depth_surf", C.c_int32),
        ("build_ms", C.c_float),
        ("upload_ms", C.c_float),
        ("built_on_device", C.c_int32),
        ("build_attempts", C.c_int32),
    ]


class LslamPgStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("lm_trials", C.c_int32),
        ("cg_iterations", C.c_int32),
        ("status", C.c_int32),
        ("chi2_initial", C.c_double),
        ("chi2_final", C.c_double),
        ("lambda_", C.c_double),
        ("gpu_ms_total", C.c_float),
        ("fused_solves", C.c_int32),
    ]


class LslamPgMarginalOpts(C.Structure):
    """lslam_pg_marginal_opts (include/lslam_c.h)."""
    _fields_ = [("rel_tol", C.c_double), ("max_iters", C.c_int32), ("coarse", C.c_int32)]


class LslamPgMarginalStats(C.Structure):
    """lslam_pg_marginal_stats (include/lslam_c.h)."""
    _fields_ = [("columns", C.c_int32), ("panels", C.c_int32), ("iters_max", C.c_int32), ("iters_sum", C.c_int32),
                ("coarse_used", C.c_int32), ("worst_rel_residual", C.c_double)]


class LslamOdomStats(C.Structure):
    """lslam_odom_stats (include/lslam_c.h)."""
    _fields_ = [("matched", C.c_int32), ("tree_fallbacks", C.c_int32), ("searches", C.c_int32), ("reserved", C.c_int32),
                ("sweeps", C.c_uint64), ("n_last_corner", C.c_size_t), ("n_last_surf", C.c_size_t)]


class LslamOdomStep(C.Structure):
    """lslam_odom_step (include/lslam_c.h)."""
    _fields_ = [("pose", C.c_float * 6), ("x", C.c_float * 6), ("n_rows", C.c_int32), ("n_line", C.c_int32), ("n_plane", C.c_int32),
                ("degenerate", C.c_int32), ("converged", C.c_int32), ("done", C.c_int32), ("loop_iter", C.c_int32),
                ("solves", C.c_int32), ("tie", C.c_int32), ("refreshed", C.c_int32)]


class LslamIcpStep(C.Structure):
    """lslam_icp_step (include/lslam_c.h)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("W", C.c_double * 3), ("det_sign", C.c_int32), ("fitted", C.c_int32),
                ("overflow_stack", C.c_int32), ("blocks", C.c_int32)]


class LslamOregStats(C.Structure):
    """lslam_oreg_stats (include/lslam_c.h)."""
    _fields_ = [("sweeps", C.c_uint64), ("n_cells", C.c_size_t), ("n_points", C.c_size_t), ("imu_states", C.c_int32),
                ("launches", C.c_int32), ("bytes_up", C.c_size_t), ("bytes_down", C.c_size_t)]


class LslamSregStats(C.Structure):
    """lslam_sreg_stats (include/lslam_c.h)."""
    _fields_ = [("sweeps", C.c_uint64), ("n_points", C.c_size_t), ("imu_states", C.c_int32), ("launches", C.c_int32),
                ("bytes_up", C.c_size_t), ("bytes_down", C.c_size_t)]


class LslamLocMapStats(C.Structure):
    """lslam_loc_map_stats (include/lslam_c.h)."""
    _fields_ = [("cubes_loaded", C.c_int64 * 2), ("cubes_with_tree", C.c_int64 * 2), ("n_points", C.c_uint64 * 2),
                ("structure_builds", C.c_int64), ("grid_builds", C.c_int64), ("grid_cube", C.c_int32 * 3),
                ("grid_reach", C.c_int32), ("grid_on", C.c_int32 * 2), ("tree_depth", C.c_int32), ("reserved", C.c_int32)]


class LslamLocSearchCounts(C.Structure):
    """lslam_loc_search_counts (include/lslam_c.h): [0] the last sweep, [1] since creation."""
    _fields_ = [("swept", C.c_uint64 * 2), ("grid_proven", C.c_uint64 * 2), ("cube_refused", C.c_uint64 * 2),
                ("to_trees", C.c_uint64 * 2), ("fallback_sweeps", C.c_uint64 * 2), ("host_waits", C.c_uint64 * 2),
                ("bytes_up", C.c_uint64 * 2), ("bytes_down", C.c_uint64 * 2)]


class LslamRelocOpts(C.Structure):
    """lslam_reloc_opts (include/lslam_c.h)."""
    _fields_ = [("voxel", C.c_float), ("max_points", C.c_int32), ("top_m", C.c_int32), ("max_candidates", C.c_int32),
                ("nms_m", C.c_float), ("nms_rot", C.c_int32), ("rot_cyclic", C.c_int32), ("refine_rounds", C.c_int32),
                ("min_fraction", C.c_float), ("apply", C.c_int32)]


class LslamRelocCandidate(C.Structure):
    """lslam_reloc_candidate (include/lslam_c.h)."""
    _fields_ = [("hypothesis", C.c_int32), ("coarse_score", C.c_int32), ("status", C.c_int32), ("rounds", C.c_int32),
                ("n_rows", C.c_int32), ("pose", C.c_float * 6)]


class LslamRelocResult(C.Structure):
    """lslam_reloc_result (include/lslam_c.h)."""
    _fields_ = [("accepted", C.c_int32), ("winner", C.c_int32), ("runner_up", C.c_int32), ("fraction", C.c_float),
                ("T", C.c_float * 16), ("n_hypotheses", C.c_int64), ("skipped", C.c_int64), ("n_points", C.c_int32 * 2),
                ("n_scored", C.c_int32 * 2), ("occupied_voxels", C.c_int64 * 2), ("n_selected", C.c_int32),
                ("n_candidates", C.c_int32), ("candidates", LslamRelocCandidate * 64), ("ms_coarse", C.c_float),
                ("ms_refine", C.c_float)]


class LslamRelocMapStats(C.Structure):
    """lslam_reloc_map_stats (include/lslam_c.h)."""
    _fields_ = [("occupied_voxels", C.c_int64 * 2), ("table_slots", C.c_uint64), ("builds", C.c_int64), ("voxel", C.c_float),
                ("valid", C.c_int32)]


class LslamLocWindowStats(C.Structure):
    """lslam_loc_window_stats (include/lslam_c.h): the paged window of the localisation node."""
    _fields_ = [("paged", C.c_int32), ("have_window", C.c_int32), ("centre", C.c_int32 * 3), ("dims", C.c_int32 * 3),
                ("steps", C.c_int64), ("refused_steps", C.c_int64), ("resident", C.c_int64 * 2),
                ("resident_with_tree", C.c_int64 * 2), ("staged", C.c_int64 * 2), ("entered", C.c_int64 * 2),
                ("left", C.c_int64 * 2), ("adopted", C.c_int64 * 2), ("entered_total", C.c_int64 * 2),
                ("left_total", C.c_int64 * 2), ("adopted_total", C.c_int64 * 2), ("staged_dropped_total", C.c_int64 * 2),
                ("files_read", C.c_int64), ("files_read_total", C.c_int64), ("files_missing", C.c_int64),
                ("files_missing_total", C.c_int64), ("trees_built", C.c_int64), ("trees_built_total", C.c_int64),
                ("forest_builds_total", C.c_int64), ("bytes_uploaded", C.c_uint64), ("bytes_uploaded_total", C.c_uint64),
                ("step_kernels", C.c_int32), ("step_filter_runs", C.c_int32), ("step_forest_builds", C.c_int32),
                ("step_host_waits", C.c_int32), ("arena_points_used", C.c_uint64), ("arena_points_capacity", C.c_uint64),
                ("arena_nodes_used", C.c_uint64), ("arena_nodes_capacity", C.c_uint64), ("active_cubes", C.c_uint64)]


class LslamSurveyParams(C.Structure):
    """lslam_survey_params (include/lslam_c.h)."""
    _fields_ = [("boundary_angle", C.c_double), ("partition_leaf", C.c_float), ("partition_min_points", C.c_int32),
                ("filter_leaf", C.c_float), ("filter_min_points", C.c_int32), ("normal_radius", C.c_float), ("knn_k", C.c_int32),
                ("smoothness_angle", C.c_float), ("curvature_threshold", C.c_float), ("cluster_min", C.c_int32),
                ("cluster_max", C.c_int32), ("boundary_radius", C.c_float), ("feature_leaf", C.c_float),
                ("feature_min_points", C.c_int32), ("cube_size", C.c_float), ("cube_dims", C.c_int32 * 3),
                ("cube_origin", C.c_int32 * 3), ("knn_cell", C.c_float), ("reserved", C.c_int32)]


class LslamSurveyStats(C.Structure):
    """lslam_survey_stats (include/lslam_c.h)."""
    _fields_ = [(k, C.c_int64) for k in ("points_in", "points_nonfinite", "blocks_kept", "blocks_dropped", "max_block_points",
                                         "filtered_points", "undefined_normals", "clusters_kept", "clusters_dropped",
                                         "label_sweeps", "planar_points", "boundary_points", "n_corner", "n_surf")]


class LslamEdgeInfo(C.Structure):
    """lslam_edge_info (include/lslam_c.h): the match Hessian of a pose-graph edge, order [t, q]."""
    _fields_ = [("H", C.c_double * 36), ("eig", C.c_double * 6), ("evec", C.c_double * 36), ("sum_b2", C.c_double),
                ("n_rows", C.c_int32), ("n_line", C.c_int32), ("n_plane", C.c_int32)]

    def as_dict(self):
        import numpy as np
        return dict(H=np.array(self.H, np.float64).reshape(6, 6), eig=np.array(self.eig, np.float64),
                    evec=np.array(self.evec, np.float64).reshape(6, 6), sum_b2=float(self.sum_b2), n_rows=int(self.n_rows),
                    n_line=int(self.n_line), n_plane=int(self.n_plane))


class LslamKfsStats(C.Structure):
    """lslam_kfs_stats (include/lslam_c.h)."""
    _fields_ = [("n_keyframes", C.c_int64), ("n_points", C.c_uint64 * 2), ("n_slabs", C.c_int64), ("bytes_held", C.c_uint64),
                ("cloud_bytes_uploaded", C.c_uint64), ("cloud_bytes_downloaded", C.c_uint64)]


class LslamScParams(C.Structure):
    """lslam_sc_params (include/lslam_c.h)."""
    _fields_ = [("n_ring", C.c_int32), ("n_sector", C.c_int32), ("max_range", C.c_float), ("height_offset", C.c_float),
                ("up_axis", C.c_int32)]


class LslamScStats(C.Structure):
    """lslam_sc_stats (include/lslam_c.h)."""
    _fields_ = [("params", LslamScParams), ("is_set", C.c_int32), ("n_described", C.c_int64), ("descriptor_bytes", C.c_uint64),
                ("describe_launches", C.c_int64), ("query_launches", C.c_int64)]


class LslamVisParams(C.Structure):
    """lslam_vis_params (include/lslam_c.h)."""
    _fields_ = [("n_row", C.c_int32), ("n_col", C.c_int32), ("fov_down_deg", C.c_float), ("fov_up_deg", C.c_float),
                ("min_range", C.c_float), ("max_range", C.c_float), ("window", C.c_int32), ("abs_margin", C.c_float),
                ("rel_margin", C.c_float), ("min_free_votes", C.c_int32), ("up_axis", C.c_int32)]


class LslamVisStats(C.Structure):
    """lslam_vis_stats (include/lslam_c.h)."""
    _fields_ = [("params", LslamVisParams), ("is_set", C.c_int32), ("n_images", C.c_int64), ("image_bytes", C.c_uint64),
                ("image_launches", C.c_int64), ("vote_launches", C.c_int64)]


class LslamOccParams(C.Structure):
    """lslam_occ_params (include/lslam_c.h)."""
    _fields_ = [("origin", C.c_double * 2), ("resolution", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("up_axis", C.c_int32), ("min_range", C.c_float), ("max_range", C.c_float), ("obstacle_min", C.c_float),
                ("obstacle_max", C.c_float), ("ground_band", C.c_float), ("sensor_height", C.c_float),
                ("ground_clears", C.c_int32), ("hit_weight", C.c_int32), ("min_observations", C.c_int32), ("reserved", C.c_int32)]


class LslamOccStats(C.Structure):
    """lslam_occ_stats (include/lslam_c.h)."""
    _fields_ = [("params", LslamOccParams), ("is_set", C.c_int32), ("n_integrated", C.c_int32), ("rays_cast", C.c_int64),
                ("rays_dropped", C.c_int64), ("rays_obstacle", C.c_int64), ("rays_ground", C.c_int64), ("grid_bytes", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("ray_launches", C.c_int64), ("merge_launches", C.c_int64),
                ("value_launches", C.c_int64)]


class LslamMapqParams(C.Structure):
    """lslam_mapq_params (include/lslam_c.h)."""
    _fields_ = [("radius", C.c_float), ("min_neighbors", C.c_int32), ("lambda_floor", C.c_double), ("reserved", C.c_int32 * 4)]


class LslamMapqStats(C.Structure):
    """lslam_mapq_stats (include/lslam_c.h)."""
    _fields_ = [("n_surface", C.c_int64), ("n_query", C.c_int64), ("n_nonfinite", C.c_int64), ("n_sparse", C.c_int64),
                ("n_defined", C.c_int64), ("sum_entropy_q32", C.c_int64), ("sum_plane_var_q30", C.c_int64),
                ("sum_neighbors", C.c_int64), ("max_neighbors", C.c_int64), ("mean_entropy", C.c_double),
                ("mean_plane_variance", C.c_double), ("mean_neighbors", C.c_double), ("ms_sort", C.c_float),
                ("ms_kernel", C.c_float), ("ms_reduce", C.c_float), ("reserved", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class LslamTrajParams(C.Structure):
    """lslam_traj_params (include/lslam_c.h)."""
    _fields_ = [("gate", C.c_double), ("align", C.c_int32), ("reserved", C.c_int32 * 3)]


class LslamTrajStats(C.Structure):
    """lslam_traj_stats (include/lslam_c.h)."""
    _fields_ = [("n_used", C.c_int64), ("n_gated", C.c_int64), ("mean", C.c_double * 4), ("var", C.c_double * 4),
                ("max", C.c_double * 4), ("mean_dt", C.c_double), ("aligned", C.c_int32), ("reserved", C.c_int32),
                ("ate_rmse", C.c_double), ("T_align", C.c_double * 16)]


class LslamFloorParams(C.Structure):
    """lslam_floor_params (include/lslam_c.h)."""
    _fields_ = [("up", C.c_float * 3), ("sensor_height", C.c_float), ("height_clip_range", C.c_float), ("max_range", C.c_float),
                ("n_hypotheses", C.c_int32), ("inlier_threshold", C.c_float), ("min_inliers", C.c_int32),
                ("max_normal_angle_deg", C.c_float), ("refit_iterations", C.c_int32), ("seed", C.c_uint32)]


class LslamFloorResult(C.Structure):
    """lslam_floor_result (include/lslam_c.h)."""
    _fields_ = [("plane", C.c_double * 4), ("rms_distance", C.c_double), ("n_candidates", C.c_int32), ("n_inliers", C.c_int32),
                ("best_hypothesis", C.c_int32), ("best_count", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        import numpy as np
        return dict(plane=np.array(self.plane, np.float64), rms_distance=float(self.rms_distance),
                    n_candidates=int(self.n_candidates), n_inliers=int(self.n_inliers), best_hypothesis=int(self.best_hypothesis),
                    best_count=int(self.best_count), status=int(self.status))


ALLREDUCE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)
ALLGATHERV_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32)
c_double_p = C.POINTER(C.c_double)

# every symbol include/lslam_c.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "lslam_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "lslam_ctx_destroy": (None, [C.c_void_p]),
    "lslam_last_error": (C.c_char_p, []),
    "lslam_default_opts": (None, [C.POINTER(LslamOpts)]),
    "lslam_abi_version": (C.c_int, []),
    "lslam_sizeof_opts": (C.c_size_t, []),
    "lslam_sizeof_stats": (C.c_size_t, []),
    "lslam_map_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]),
    "lslam_map_epoch": (C.c_uint64, [C.c_void_p]),
    "lslam_map_info_get": (C.c_int, [C.c_void_p, C.POINTER(LslamMapInfo)]),
    "lslam_cubemap_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                    C.c_float, c_int32_p, c_int32_p]),
    "lslam_scan_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]),
    "lslam_scan_set_batch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t]),
    "lslam_scanmatch_run_batch": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, C.POINTER(LslamOpts),
                                            C.POINTER(LslamStats)]),
    "lslam_scanmatch_run": (C.c_int, [C.c_void_p, c_float_p, C.POINTER(LslamOpts), C.POINTER(LslamStats)]),
    "lslam_scanmatch_run_sharded": (C.c_int, [C.c_void_p, c_float_p, C.POINTER(LslamOpts), ALLREDUCE_FN,
                                              C.c_void_p, C.c_void_p, C.POINTER(LslamStats)]),
    "lslam_stereo_default_cam": (None, [C.POINTER(LslamStereoCam)]),
    "lslam_stereo_set": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_float_p, C.c_size_t, C.POINTER(LslamStereoCam)]),
    "lslam_stereo_clear": (C.c_int, [C.c_void_p]),
    "lslam_stereo_sums": (C.c_int, [C.c_void_p, c_float_p, c_double_p]),
    "lslam_stereo_set_batch": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_float_p, c_float_p, C.POINTER(C.c_size_t),
                                         C.POINTER(LslamStereoCam)]),
    "lslam_stereo_sums_batch": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_double_p]),
    "lslam_scanmatch_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_size_t, c_float_p, C.POINTER(LslamOpts), C.POINTER(LslamStats)]),
    "lslam_scanmatch_full": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                       c_float_p, C.POINTER(LslamOpts), C.POINTER(LslamStats)]),
    "lslam_odometry_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_int32,
                                       C.c_float, C.c_float, C.POINTER(LslamStats)]),
    "lslam_odometry_match_trees": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_int32,
                                             C.c_float, C.c_float, C.POINTER(LslamStats)]),
    "lslam_transform_to_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p]),
    "lslam_isometry_to_pose": (None, [c_float_p, c_float_p]),
    "lslam_pose_to_isometry": (None, [c_float_p, c_float_p]),
    "lslam_transform_associate": (None, [c_float_p, c_float_p, c_float_p, c_float_p]),
    "lslam_knn5": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, c_int32_p, c_float_p]),
    "lslam_sweep": (C.c_int, [C.c_void_p, c_float_p, C.c_int32, c_int32_p, c_float_p, c_float_p,
                              c_uint8_p, c_float_p]),
    "lslam_knn5_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, c_int32_p, c_float_p,
                                c_int32_p]),
    "lslam_sweep_ex": (C.c_int, [C.c_void_p, c_float_p, C.c_int32, C.c_int32, c_int32_p, c_float_p, c_float_p,
                                 c_uint8_p, c_float_p]),
    "lslam_residuals": (C.c_int, [C.c_void_p, c_float_p, c_float_p, c_uint8_p, c_float_p]),
    "lslam_scanmatch_batch": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, C.POINTER(LslamOpts), C.POINTER(LslamStats)]),
    "lslam_posegraph_optimize": (C.c_int, [C.c_int, C.c_int32, c_double_p, C.c_int32, c_int32_p, c_double_p, c_double_p,
                                           C.c_int32, C.c_int32, C.POINTER(LslamPgStats)]),
    "lslam_gn_step": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_int32, c_float_p, c_float_p,
                                c_int32_p, C.c_float, C.c_float, c_float_p, c_float_p, c_float_p,
                                c_int32_p]),
    "lslam_stream": (C.c_void_p, [C.c_void_p]),
    "lslam_debug_sweep_launches": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lslam_debug_cert_stats": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lslam_debug_grid_stats": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lslam_debug_knn5_wide": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, c_int32_p, c_float_p,
                                        C.POINTER(C.c_uint8)]),
    "lslam_debug_sort_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32)]),
    "lslam_debug_cert_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]),
    "lslam_pg_create": (C.c_int, [C.c_int, C.c_int32, c_double_p, C.c_int32, c_int32_p, c_double_p, c_double_p,
                                  C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_pg_destroy": (None, [C.c_void_p]),
    "lslam_pg_last_error": (C.c_char_p, []),
    "lslam_fmap_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_fmap_destroy": (None, [C.c_void_p]),
    "lslam_fmap_setup_filter_size": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "lslam_fmap_setup_world_origin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lslam_fmap_setup_world_cube_size": (C.c_int, [C.c_void_p, C.c_float]),
    "lslam_fmap_setup_lidar_valid_distance": (C.c_int, [C.c_void_p, C.c_float]),
    "lslam_fmap_update": (C.c_int, [C.c_void_p, c_float_p]),
    "lslam_fmap_add_feature_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_size_t, c_float_p]),
    "lslam_fmap_add_feature_cloud_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_size_t, c_float_p]),
    "lslam_fmap_wait": (C.c_int, [C.c_void_p]),
    "lslam_fmap_surround_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lslam_fmap_get_surround": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p, C.c_size_t]),
    "lslam_fmap_surround_to_map": (C.c_int, [C.c_void_p]),
    "lslam_fmap_surround_to_map_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lslam_fmap_to_cubemap": (C.c_int, [C.c_void_p]),
    "lslam_fmap_cubemap_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lslam_fmap_rebuild_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lslam_fmap_cubemap_invalidate": (C.c_int, [C.c_void_p]),
    "lslam_fmap_get_full_map": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_fmap_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_fmap_load": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_fmap_info": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, C.c_size_t,
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lslam_lmap_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_lmap_destroy": (None, [C.c_void_p]),
    "lslam_lmap_setup_queue_distance": (C.c_int, [C.c_void_p, C.c_double]),
    "lslam_lmap_setup_filter_size": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "lslam_lmap_add_data_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p]),
    "lslam_lmap_add_data_frame_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_float_p]),
    "lslam_lmap_surround_to_map_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lslam_lmap_get_surround": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t), c_float_p, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    "lslam_lmap_info": (C.c_int, [C.c_void_p, c_int32_p, C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "lslam_lmap_get_frames": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.POINTER(C.c_double), c_int32_p, c_float_p, C.c_size_t,
                                        c_float_p, C.c_size_t]),
    "lslam_lmap_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lslam_lmap_clear": (C.c_int, [C.c_void_p]),
    "lslam_kfs_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_size_t, C.POINTER(C.c_void_p)]),
    "lslam_kfs_destroy": (None, [C.c_void_p]),
    "lslam_kfs_clear": (C.c_int, [C.c_void_p]),
    "lslam_kfs_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_int32_p]),
    "lslam_kfs_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_int32_p]),
    "lslam_kfs_counts": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lslam_kfs_get": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_float_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_kfs_view": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_size_t)]),
    "lslam_kfs_info": (C.c_int, [C.c_void_p, C.POINTER(LslamKfsStats)]),
    "lslam_kfs_debug_local_clouds": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, c_float_p, C.c_size_t,
                                               C.POINTER(C.c_size_t), c_float_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_kfs_loop_match": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_int32, c_float_p, C.c_int32,
                                       C.POINTER(LslamOpts), c_int32_p, C.POINTER(C.c_double), c_int32_p, C.POINTER(LslamStats)]),
    "lslam_kfs_scanmatch": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, c_float_p, C.POINTER(LslamOpts),
                                      C.POINTER(LslamStats)]),
    "lslam_kfs_add_to_fmap": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, c_float_p]),
    "lslam_floor_default_params": (None, [C.POINTER(LslamFloorParams)]),
    "lslam_sizeof_floor_params": (C.c_size_t, []),
    "lslam_sizeof_floor_result": (C.c_size_t, []),
    "lslam_floor_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(LslamFloorParams),
                                     C.POINTER(LslamFloorResult)]),
    "lslam_floor_detect_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(LslamFloorParams),
                                            C.POINTER(LslamFloorResult)]),
    "lslam_floor_detect_keyframes": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.POINTER(LslamFloorParams),
                                               C.POINTER(LslamFloorResult)]),
    "lslam_debug_floor_score": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_debug_floor_hypotheses": (C.c_int, [C.c_void_p, c_int32_p, C.c_size_t, C.POINTER(C.c_size_t), c_int32_p, c_float_p,
                                               c_int32_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_sizeof_edge_info": (C.c_size_t, []),
    "lslam_match_information": (C.c_int, [C.c_void_p, c_float_p, C.c_int32, C.POINTER(LslamEdgeInfo)]),
    "lslam_keyframe_edge_information": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_int32, c_float_p, C.c_float, C.c_float,
                                             C.c_float, C.c_float, C.POINTER(LslamEdgeInfo)]),
    "lslam_sc_default_params": (None, [C.POINTER(LslamScParams)]),
    "lslam_sc_setup": (C.c_int, [C.c_void_p, C.POINTER(LslamScParams)]),
    "lslam_sc_descriptor": (C.c_int, [C.c_void_p, C.c_int32, c_float_p]),
    "lslam_sc_query": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, C.c_int32, c_int32_p, c_int32_p, c_float_p,
                                     c_int32_p]),
    "lslam_sc_distances": (C.c_int, [C.c_void_p, C.c_int32, c_float_p, c_int32_p]),
    "lslam_sc_info": (C.c_int, [C.c_void_p, C.POINTER(LslamScStats)]),
    "lslam_vis_default_params": (None, [C.POINTER(LslamVisParams)]),
    "lslam_sizeof_vis_params": (C.c_size_t, []),
    "lslam_sizeof_vis_stats": (C.c_size_t, []),
    "lslam_vis_setup": (C.c_int, [C.c_void_p, C.POINTER(LslamVisParams)]),
    "lslam_vis_info": (C.c_int, [C.c_void_p, C.POINTER(LslamVisStats)]),
    "lslam_vis_range_image": (C.c_int, [C.c_void_p, C.c_int32, c_float_p]),
    "lslam_vis_votes": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                  C.POINTER(C.c_uint32)]),
    "lslam_vis_votes_device": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lslam_vis_filter_device": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_size_t)]),
    "lslam_vis_add_to_fmap": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, c_float_p, C.c_int32, c_int32_p, c_float_p,
                                        C.POINTER(C.c_size_t)]),
    "lslam_debug_vis_votes": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_occ_default_params": (None, [C.POINTER(LslamOccParams)]),
    "lslam_sizeof_occ_params": (C.c_size_t, []),
    "lslam_sizeof_occ_stats": (C.c_size_t, []),
    "lslam_occ_setup": (C.c_int, [C.c_void_p, C.POINTER(LslamOccParams)]),
    "lslam_occ_info": (C.c_int, [C.c_void_p, C.POINTER(LslamOccStats)]),
    "lslam_occ_clear": (C.c_int, [C.c_void_p]),
    "lslam_occ_integrate": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.POINTER(C.c_double), c_int32_p]),
    "lslam_occ_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "lslam_occ_values": (C.c_int, [C.c_void_p, C.POINTER(C.c_int8)]),
    "lslam_occ_view": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "lslam_occ_fit_bounds": (C.c_int, [C.c_int32, c_float_p, C.POINTER(LslamOccParams)]),
    "lslam_debug_occ_integrate": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_mapq_default_params": (None, [C.POINTER(LslamMapqParams)]),
    "lslam_sizeof_mapq_params": (C.c_size_t, []),
    "lslam_sizeof_mapq_stats": (C.c_size_t, []),
    "lslam_mapq_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                  C.POINTER(LslamMapqParams), C.POINTER(LslamMapqStats), c_double_p, c_double_p, c_int32_p]),
    "lslam_mapq_eval_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(LslamMapqParams),
                                         C.POINTER(LslamMapqStats), C.c_void_p, C.c_void_p, C.c_void_p]),
    "lslam_mapq_fmap": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LslamMapqParams), C.POINTER(LslamMapqStats)]),
    "lslam_mapq_keyframes": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_float_p, C.c_int32, C.POINTER(LslamMapqParams),
                                       C.POINTER(LslamMapqStats)]),
    "lslam_traj_default_params": (None, [C.POINTER(LslamTrajParams)]),
    "lslam_sizeof_traj_params": (C.c_size_t, []),
    "lslam_sizeof_traj_stats": (C.c_size_t, []),
    "lslam_traj_eval": (C.c_int, [c_double_p, c_double_p, C.c_size_t, c_double_p, c_double_p, C.c_size_t, C.POINTER(LslamTrajParams),
                                  C.POINTER(LslamTrajStats)]),
    "lslam_voxel_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, c_float_p,
                                   C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_voxel_grid2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, c_float_p,
                                    C.c_size_t, C.POINTER(C.c_size_t), c_float_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_reg_default_params": (None, [C.POINTER(LslamRegParams)]),
    "lslam_extract_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, c_int32_p,
                                         C.c_size_t, C.POINTER(LslamRegParams), c_float_p, c_float_p, c_float_p,
                                         c_float_p, C.POINTER(C.c_size_t), c_float_p, C.POINTER(C.c_int8),
                                         C.POINTER(C.c_int8)]),
    "lslam_multiscan_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_float,
                                           C.c_int32, C.c_float, c_float_p, C.c_size_t, C.POINTER(C.c_size_t),
                                           c_int32_p]),
    "lslam_fset_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "lslam_fset_destroy": (None, [C.c_void_p]),
    "lslam_fset_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lslam_fset_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_size_t, C.c_size_t]),
    "lslam_fset_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_float_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_extract_features_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, c_int32_p, C.c_size_t,
                                             C.POINTER(LslamRegParams), C.c_void_p, C.POINTER(C.c_size_t)]),
    "lslam_odom_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "lslam_odom_destroy": (None, [C.c_void_p]),
    "lslam_odom_process": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, c_float_p, C.POINTER(LslamStats), C.POINTER(LslamOdomStats),
                                     c_float_p, C.c_size_t, c_float_p, C.c_size_t]),
    "lslam_odom_last_clouds": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p, C.c_size_t]),
    "lslam_odom_reset": (C.c_int, [C.c_void_p]),
    "lslam_debug_odom_search": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t]),
    "lslam_debug_odom_step": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_float_p,
                                        c_float_p, C.POINTER(C.c_uint8), c_double_p, C.POINTER(LslamOdomStep)]),
    "lslam_debug_odom_runs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lslam_odom_set_publish": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_odom_last_view": (C.c_int, [C.c_void_p, C.POINTER(c_float_p), C.POINTER(C.c_size_t), C.POINTER(c_float_p),
                                       C.POINTER(C.c_size_t)]),
    "lslam_sreg_create": (C.c_int, [C.c_void_p, C.POINTER(LslamRegParams), C.c_float, C.c_float, C.c_int32, C.c_float, C.c_int32,
                                    C.POINTER(C.c_void_p)]),
    "lslam_sreg_destroy": (None, [C.c_void_p]),
    "lslam_sreg_imu_push": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, c_double_p]),
    "lslam_sreg_imu_info": (C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_double_p]),
    "lslam_sreg_imu_clear": (C.c_int, [C.c_void_p]),
    "lslam_sreg_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64, C.c_void_p, C.POINTER(C.c_size_t),
                                     c_float_p, C.POINTER(LslamSregStats)]),
    "lslam_sreg_cloud": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t), c_int32_p]),
    "lslam_oreg_create": (C.c_int, [C.c_void_p, C.POINTER(LslamRegParams), C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_oreg_destroy": (None, [C.c_void_p]),
    "lslam_oreg_imu_push": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double, c_double_p]),
    "lslam_oreg_imu_info": (C.c_int, [C.c_void_p, c_int32_p, c_double_p, c_double_p]),
    "lslam_oreg_imu_clear": (C.c_int, [C.c_void_p]),
    "lslam_oreg_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int64, C.c_void_p,
                                     C.POINTER(C.c_size_t), c_float_p, C.POINTER(LslamOregStats)]),
    "lslam_oreg_cloud": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t), c_int32_p]),
    "lslam_loc_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_loc_destroy": (None, [C.c_void_p]),
    "lslam_loc_setup_scan_filter_size": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "lslam_loc_setup_map_filter_size": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "lslam_loc_setup_world_origin": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "lslam_loc_setup_world_cube_size": (C.c_int, [C.c_void_p, C.c_float]),
    "lslam_loc_setup_lidar_valid_distance": (C.c_int, [C.c_void_p, C.c_float]),
    "lslam_loc_setup_search": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_loc_load": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_loc_set_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32]),
    "lslam_loc_set_map_from_fmap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lslam_loc_info": (C.c_int, [C.c_void_p, C.POINTER(LslamLocMapStats)]),
    "lslam_loc_set_initial_pose": (C.c_int, [C.c_void_p, c_float_p]),
    "lslam_loc_process": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_int64,
                                    c_float_p, c_float_p, c_int32_p, C.POINTER(LslamStats)]),
    "lslam_loc_process_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, c_float_p, C.c_int64,
                                           c_float_p, c_float_p, c_int32_p, C.POINTER(LslamStats)]),
    "lslam_loc_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p,
                                  C.POINTER(LslamStats)]),
    "lslam_loc_get_surround": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t), c_float_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "lslam_loc_search_stats": (C.c_int, [C.c_void_p, C.POINTER(LslamLocSearchCounts)]),
    "lslam_loc_debug_knn5": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, c_float_p, c_uint8_p]),
    "lslam_reloc_relocalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_size_t,
                                         c_float_p, C.c_size_t, C.POINTER(LslamRelocOpts), C.POINTER(LslamRelocResult)]),
    "lslam_reloc_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_size_t,
                                     c_float_p, C.c_size_t, C.POINTER(LslamRelocOpts), c_int32_p, c_int32_p, c_int32_p, c_int32_p,
                                     C.POINTER(LslamRelocResult)]),
    "lslam_reloc_nms": (C.c_int, [c_int32_p, C.c_int32, c_float_p, C.c_size_t, C.c_size_t, C.POINTER(LslamRelocOpts), c_int32_p]),
    "lslam_reloc_occupied": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_size_t, c_uint8_p]),
    "lslam_reloc_info": (C.c_int, [C.c_void_p, C.POINTER(LslamRelocMapStats)]),
    "lslam_pmap_open": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_pmap_setup_capacity": (C.c_int, [C.c_void_p, C.c_size_t]),
    "lslam_pmap_update": (C.c_int, [C.c_void_p, c_float_p]),
    "lslam_pmap_stage": (C.c_int, [C.c_void_p, c_float_p]),
    "lslam_pmap_get_surround": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.POINTER(C.c_size_t), c_float_p, C.c_size_t,
                                                C.POINTER(C.c_size_t)]),
    "lslam_pmap_window_info": (C.c_int, [C.c_void_p, C.POINTER(LslamLocWindowStats)]),
    "lslam_index_convert": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p]),
    "lslam_survey_default_params": (None, [C.POINTER(LslamSurveyParams)]),
    "lslam_survey_extract": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(LslamSurveyParams),
                                       C.POINTER(C.c_void_p)]),
    "lslam_survey_extract_file": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(LslamSurveyParams), C.POINTER(C.c_void_p)]),
    "lslam_survey_info": (C.c_int, [C.c_void_p, C.POINTER(LslamSurveyStats)]),
    "lslam_survey_get": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p, C.c_size_t]),
    "lslam_survey_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_survey_destroy": (None, [C.c_void_p]),
    "lslam_voxel_grid_min": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int32, c_float_p,
                                       C.c_size_t, C.POINTER(C.c_size_t)]),
    "lslam_debug_survey_normals": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_float_p, C.c_size_t, C.c_float, c_float_p,
                                             c_int32_p]),
    "lslam_debug_survey_knn": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, C.c_int32, C.c_float, c_int32_p]),
    "lslam_debug_survey_region": (C.c_int, [C.c_void_p, c_float_p, C.c_size_t, c_int32_p, C.c_int32, C.c_float, c_int32_p,
                                            c_int32_p]),
    "lslam_debug_survey_boundary": (C.c_int, [C.c_void_p, c_float_p, c_float_p, C.c_size_t, C.c_float, C.c_double, c_uint8_p,
                                              C.POINTER(C.c_double)]),
    "lslam_pg_save_g2o": (C.c_int, [C.c_void_p, C.c_char_p]),
    "lslam_g2o_read": (C.c_int, [C.c_char_p, c_int32_p, c_double_p, c_int32_p, c_int32_p, c_double_p, c_double_p,
                                 c_int32_p]),
    "lslam_pg_set_shard": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, ALLREDUCE_FN, C.c_void_p, C.c_void_p]),
    "lslam_pg_system_doubles": (C.c_size_t, [C.c_void_p]),
    "lslam_pg_row_shard_range": (None, [C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "lslam_pg_set_row_shard": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "lslam_pg_row_sharded_solves": (C.c_int32, [C.c_void_p]),
    "lslam_pg_set_solve_tolerance": (C.c_int, [C.c_void_p, C.c_double]),
    "lslam_pg_row_gathered_solves": (C.c_int32, [C.c_void_p]),
    "lslam_pg_set_row_gather": (C.c_int, [C.c_void_p, ALLGATHERV_FN, C.c_void_p, C.c_int32, C.c_int32]),
    "lslam_pg_num_offdiag": (C.c_int32, [C.c_void_p]),
    "lslam_pg_optimize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LslamPgStats)]),
    "lslam_pg_get_poses": (C.c_int, [C.c_void_p, c_double_p]),
    "lslam_pg_linearize": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_int32_p, c_double_p, c_double_p]),
    "lslam_pg_solve": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_int32_p]),
    "lslam_pg_set_robust_kernels": (C.c_int, [C.c_void_p, c_int32_p, c_double_p]),
    "lslam_pg_edge_robust": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "lslam_pg_robust_info": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_double_p]),
    "lslam_pg_set_priors": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_int32_p, c_double_p, c_double_p, c_int32_p,
                                      c_double_p]),
    "lslam_pg_num_priors": (C.c_int32, [C.c_void_p]),
    "lslam_pg_prior_robust": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "lslam_g2o_read_priors": (C.c_int, [C.c_char_p, c_int32_p, c_int32_p, c_int32_p, c_double_p, c_double_p]),
    "lslam_pg_set_plane_priors": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, c_double_p, c_double_p, c_double_p, c_int32_p,
                                            c_double_p]),
    "lslam_pg_num_plane_priors": (C.c_int32, [C.c_void_p]),
    "lslam_pg_plane_prior_robust": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "lslam_g2o_read_plane_priors": (C.c_int, [C.c_char_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_double_p]),
    "lslam_pg_marginals": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.POINTER(LslamPgMarginalOpts), c_double_p, c_double_p,
                                     C.POINTER(LslamPgMarginalStats)]),
    "lslam_pg_relative_covariances": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_int32_p, C.POINTER(LslamPgMarginalOpts),
                                                c_double_p, C.POINTER(LslamPgMarginalStats)]),
    "lslam_debug_pg_marginal_columns": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LslamPgMarginalOpts), c_double_p,
                                                  C.POINTER(LslamPgMarginalStats)]),
    "lslam_pg_stream": (C.c_void_p, [C.c_void_p]),
    "lslam_pg_kernel_from_name": (C.c_int, [C.c_char_p]),
    "lslam_icp_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_int32,
                                  C.c_double, C.c_double, c_double_p, c_int32_p, c_int32_p]),
    "lslam_debug_icp_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, c_float_p, C.c_double,
                                       c_int32_p, c_float_p, c_double_p, C.POINTER(LslamIcpStep)]),
    "lslam_debug_icp_fit": (C.c_int, [c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "lslam_comm_unique_id": (C.c_int, [c_uint8_p]),
    "lslam_comm_create": (C.c_int, [C.c_int, c_uint8_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lslam_comm_destroy": (None, [C.c_void_p]),
    "lslam_comm_version": (C.c_int, [c_int32_p]),
    "lslam_comm_info": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p]),
    "lslam_debug_grid_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_grid_lean_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_queue_lean_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_fit_inrange_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_fit_inrange_ops": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float)]),
    "lslam_debug_fit_inrange_fits": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.c_int32,
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "lslam_debug_fit_stage": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t, C.c_int32,
                              C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "lslam_debug_grid_fine_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_grid_fine_info": (None, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    "lslam_debug_grid_fine_table": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, c_int32_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32),
                                              C.c_size_t, C.POINTER(C.c_float), C.c_size_t]),
    "lslam_debug_grid_wide_launches": (C.c_uint64, [C.c_void_p]),
    "lslam_debug_grid_cells": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lslam_map_defer_trees": (C.c_int, [C.c_void_p, C.c_int32]),
    "lslam_debug_lazy_trees": (None, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "lslam_comm_allreduce_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lslam_ctx_set_comm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lslam_pg_set_comm": (C.c_int, [C.c_void_p, C.c_void_p]),
}

COMM_ID_BYTES = 128
SC_POINT_CHUNK, SC_CAND_TILE, SC_MAX_TOP_K = 256, 64, 32  # LSLAM_SC_* of include/lslam_c.h: the scan-context kernels' shape
# lslam_floor_result.status (LSLAM_FLOOR_*)
FLOOR_OK, FLOOR_FEW_CANDIDATES, FLOOR_NO_HYPOTHESIS, FLOOR_FEW_INLIERS, FLOOR_STEEP = 0, 1, 2, 3, 4
SEARCH_AUTO, SEARCH_LANE, SEARCH_PACKET, SEARCH_GRID = 0, 1, 2, 3
AB_WIDE_NF_MARGIN, AB_NO_COMPACT = 16, 64  # lslam_opts.ab_switches (LSLAM_AB_*); any other bit is refused
AB_GRID_GENERAL = 256
AB_GRID_CUBIC = 512
STACK_AUTO, STACK_DEEP, STACK_SHALLOW = 0, 0x100, 0x200  # ORed into a search mode (LSLAM_STACK_*)
# lslam_debug_sweep_launches: index of each sweep-kernel instantiation ("persistent", "deep_fused": retired, always 0)
SWEEP_VARIANTS = ("deep", "deep_ovf", "shallow", "cubes", "cubes_ovf", "packet", "persistent", "deep_fused")


def lib_path():
    # LSLAM_LIB lets profiling scripts load an experimental build of the same ABI
    return os.environ.get("LSLAM_LIB") or os.path.join(HERE, LIB_NAME)


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC], stdout=subprocess.DEVNULL)
    return lib_path()


_lib = None


def _preload_torch_runtime():
    """The PyTorch-ROCm wheel ships its own libamdhip64 / libhsa-runtime64 (same SONAMEs as /opt/rocm's).
    A process gets whichever copy is loaded first: this library runs on either, torch only on its own
    ("No HIP GPUs are available" otherwise).  So when torch is installed and not loaded yet, load it
    before liblslam_hip.so -- harnesses (tests, bench.py) use both in one process.  A C/C++ host that
    links liblslam_hip.so never sees this.  LSLAM_NO_TORCH_PRELOAD=1 skips it."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("LSLAM_NO_TORCH_PRELOAD"):
        return
    try:
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    except Exception:  # a broken torch install must not take the backend down
        pass


def load_library():
    """dlopen liblslam_hip.so and bind every declared symbol.  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            "%s not found: build it with `make -C %s` (hipcc --offload-arch=gfx950). "
            "This backend has no CPU fallback." % (path, CSRC))
    _preload_torch_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.lslam_abi_version() < 0:
        raise ImportError("%s was built with LSLAM_EXP_* timing-experiment macros (wrong results on purpose): not a product library; "
                          "LSLAM_ALLOW_EXPERIMENT_BUILD=1 lets the A/B scripts load it" % path)
    # the ctypes mirrors of the ABI's structs must be the library's: a stale .so (or a stale mirror) fails here, loudly
    if lib.lslam_sizeof_opts() != C.sizeof(LslamOpts) or lib.lslam_sizeof_stats() != C.sizeof(LslamStats):
        raise ImportError("%s does not match this package's struct layouts (lslam_opts %d vs %d bytes, lslam_stats %d vs %d): rebuild it"
                          % (path, lib.lslam_sizeof_opts(), C.sizeof(LslamOpts), lib.lslam_sizeof_stats(), C.sizeof(LslamStats)))
    _lib = lib
    return lib
