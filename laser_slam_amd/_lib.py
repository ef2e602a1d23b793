"""ctypes loader for liblsgpu_icp.so (C ABI: include/lsgpu_icp.h).

There is no CPU fallback: if the shared library is missing or a HIP call fails the error is raised
to the caller (the reference's own fallback -- keep the odometry guess on ConvergenceError,
laser_slam/src/laser_track.cpp:499-502 -- lives in the LaserTrack mirror, not here).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("LSGPU_SO") or os.path.join(_HERE, "liblsgpu_icp.so")   # (LSGPU_SO: another build of the same library)

OK, NO_CONVERGENCE, BAD_CONFIG, HIP_ERROR, BAD_ARG = 0, 1, 2, 3, 4

# lsgpu_icp_config.error_minimizer (LSGPU_MINIMIZER_*)
MINIMIZER_POINT_TO_PLANE, MINIMIZER_POINT_TO_POINT = 0, 1

# lsgpu_icp_config.matcher_knn: the largest k of KDTreeMatcher (LSGPU_MATCHER_KNN_MAX)
MATCHER_KNN_MAX = 8

# every symbol include/lsgpu_icp.h declares (tests/test_abi.py checks the export table against this)
ABI_SYMBOLS = [
    "lsgpu_icp_config_yaml", "lsgpu_icp_config_default", "lsgpu_icp_create", "lsgpu_icp_destroy",
    "lsgpu_icp_set_reference", "lsgpu_icp_align", "lsgpu_icp_align_batch", "lsgpu_icp_get_trace",
    "lsgpu_chain_config_yaml", "lsgpu_chain_config_default", "lsgpu_icp_filter_reference",
    "lsgpu_icp_filter_reading", "lsgpu_icp_compute", "lsgpu_cloud_upload", "lsgpu_cloud_release",
    "lsgpu_cloud_size", "lsgpu_icp_compute_clouds", "lsgpu_icp_compute_clouds_upload", "lsgpu_filter_cylinder", "lsgpu_filter_voxel_grid",
    "lsgpu_icp_get_reference_mean", "lsgpu_icp_get_info", "lsgpu_icp_get_policy_info", "lsgpu_comm_get_unique_id", "lsgpu_icp_comm_init", "lsgpu_knn", "lsgpu_knn_k", "lsgpu_trim_limit", "lsgpu_normal_eq",
    "lsgpu_point_to_point", "lsgpu_point_to_point_solve",
    "lsgpu_transform_points", "lsgpu_rotate_descriptors", "lsgpu_filter_random_sampling",
    "lsgpu_filter_sampling_surface_normal", "lsgpu_check_rigid", "lsgpu_correct_rigid", "lsgpu_rotation_distance",
    "lsgpu_strerror", "lsgpu_last_error", "lsgpu_abi_version", "lsgpu_apply_point_filters",
    "lsgpu_cloud_from_pointcloud2", "lsgpu_cloud_to_pointxyz",
    "lsgpu_icp_filter_reference_normals", "lsgpu_filter_surface_normal", "lsgpu_chain_config_check",
    "lsgpu_robust_config_default", "lsgpu_robust_config_check", "lsgpu_icp_set_robust_filter", "lsgpu_robust_scale",
    "lsgpu_robust_weights", "lsgpu_icp_get_robust_trace", "lsgpu_point_to_plane_solve",
    "lsgpu_normals_config_default", "lsgpu_normals_config_check", "lsgpu_icp_set_normals", "lsgpu_icp_reading_normals",
    "lsgpu_icp_align_normals", "lsgpu_icp_get_reference_normals", "lsgpu_orient_normals", "lsgpu_normal_angle_weights",
    "lsgpu_icp_get_normal_angle_trace",
    "lsgpu_chain_load", "lsgpu_robust_config_why", "lsgpu_normals_config_why",
    "lsgpu_filter_voxel_grid_points", "lsgpu_filter_octree_grid_points",
    "lsgpu_covariance_config_default", "lsgpu_icp_set_covariance", "lsgpu_icp_get_quality", "lsgpu_point_to_plane_cov",
    "lsgpu_point_to_plane_cov_solve", "lsgpu_loaded_chain_covariance",
    "lsgpu_icp_set_chain_cuts", "lsgpu_icp_filter_section", "lsgpu_chain_load_cuts",
    "lsgpu_max_density_config_default", "lsgpu_max_density_config_check", "lsgpu_max_density_config_why",
    "lsgpu_icp_set_max_density", "lsgpu_icp_filter_reference_normals_densities", "lsgpu_icp_filter_reference_max_density",
    "lsgpu_filter_surface_normal_densities", "lsgpu_filter_max_density", "lsgpu_loaded_chain_max_density",
    "lsgpu_shadow_config_default", "lsgpu_shadow_config_check", "lsgpu_shadow_config_why", "lsgpu_icp_set_shadow",
    "lsgpu_icp_filter_shadow", "lsgpu_filter_shadow", "lsgpu_chain_load_shadow",
    "lsgpu_motion_config_default", "lsgpu_motion_config_check", "lsgpu_motion_config_why", "lsgpu_icp_set_motion",
    "lsgpu_point_to_plane_solve_dof", "lsgpu_bound_first_violation", "lsgpu_chain_load_motion",
    "lsgpu_icp_filter_cov_sampling", "lsgpu_icp_cov_sampling_phase_ms", "lsgpu_filter_cov_sampling", "lsgpu_cov_sampling_eigen",
    "lsgpu_cov_sampling_config_default", "lsgpu_cov_sampling_config_check", "lsgpu_cov_sampling_config_why",
    "lsgpu_icp_set_cov_sampling", "lsgpu_chain_load_cov_sampling",
    "lsgpu_cloud_upload_normals", "lsgpu_cloud_has_normals", "lsgpu_icp_compute_normals",
    "lsgpu_icp_compute_clouds_upload_normals", "lsgpu_chain_load_carried", "lsgpu_chain_load_parts_carried",
    "lsgpu_surface_normal_params_check", "lsgpu_chain_load_modules", "lsgpu_icp_set_modules",
    "lsgpu_cloud_ingest", "lsgpu_cloud_download",
]

# lsgpu_chain_load_carried: which of a caller's clouds carry normals (LSGPU_CARRIED_*)
CARRIED_READING, CARRIED_REFERENCE = 1, 2

# lsgpu_motion_config.dof (LSGPU_MOTION_DOF_*): the free step, force2D, force4DOF
MOTION_DOF_6, MOTION_DOF_3, MOTION_DOF_4 = 0, 3, 4

# lsgpu_robust_config: RobustOutlierFilter's robustFct / scaleEstimator / distanceType names -> LSGPU_ROBUST_*
ROBUST_FCT = {"cauchy": 0, "huber": 1, "tukey": 2, "gm": 3, "sc": 4, "L1": 5, "welsch": 6, "student": 7}
ROBUST_SCALE = {"none": 0, "mad": 1, "berg": 2, "std": 3}
ROBUST_DIST = {"point2point": 0, "point2plane": 1}


class RobustCfg(C.Structure):
    """lsgpu_robust_config (include/lsgpu_icp.h): RobustOutlierFilter's parameters."""
    _fields_ = [("robust_fct", C.c_int), ("tuning", C.c_float), ("scale_estimator", C.c_int),
                ("nb_iteration_for_scale", C.c_int), ("distance_type", C.c_int), ("approximation", C.c_float),
                ("reserved", C.c_int * 2)]


class NormalsCfg(C.Structure):
    """lsgpu_normals_config (include/lsgpu_icp.h): SurfaceNormalOutlierFilter, reading normals, oriented normals."""
    _fields_ = [("max_angle", C.c_float), ("reading_sn_knn", C.c_int), ("reading_orient", C.c_int),
                ("reference_orient", C.c_int), ("reading_sensor", C.c_float * 3), ("reference_sensor", C.c_float * 3),
                ("reading_normals_given", C.c_int), ("reserved", C.c_int * 1)]


class NormalAngleTrace(C.Structure):
    """lsgpu_normal_angle_trace: one record per iteration of an align that applied SurfaceNormalOutlierFilter."""
    _fields_ = [("rejected", C.c_int64), ("eps", C.c_float), ("reserved", C.c_int)]


class RobustTrace(C.Structure):
    """lsgpu_robust_trace: one record per iteration of a handle with RobustOutlierFilter."""
    _fields_ = [("median", C.c_float), ("scale", C.c_float), ("w_sum", C.c_double), ("recomputed", C.c_int),
                ("reserved", C.c_int)]



class CovarianceCfg(C.Structure):
    """lsgpu_covariance_config: PointToPlaneWithCovErrorMinimizer's parameter."""
    _fields_ = [("sensor_std_dev", C.c_float), ("reserved", C.c_int * 3)]


class MaxDensityCfg(C.Structure):
    """lsgpu_max_density_config: MaxDensityDataPointsFilter's parameter."""
    _fields_ = [("max_density", C.c_float), ("reserved", C.c_int * 3)]


class CovSamplingCfg(C.Structure):
    """lsgpu_cov_sampling_config: CovarianceSamplingDataPointsFilter's nbSample (0: no module on that side) and torqueNorm of the
    two filter sections."""
    _fields_ = [("reading_nb_sample", C.c_int), ("reference_nb_sample", C.c_int), ("reading_torque_norm", C.c_int),
                ("reference_torque_norm", C.c_int), ("reserved", C.c_int * 4)]


class ShadowCfg(C.Structure):
    """lsgpu_shadow_config: ShadowDataPointsFilter's eps of the two filter sections (< 0: no module on that side)."""
    _fields_ = [("reading_eps", C.c_float), ("reference_eps", C.c_float), ("reserved", C.c_int * 2)]


class MotionCfg(C.Structure):
    """lsgpu_motion_config: PointToPlaneErrorMinimizer's force2D / force4DOF (dof) and BoundTransformationChecker."""
    _fields_ = [("dof", C.c_int), ("bound", C.c_int), ("max_rotation_norm", C.c_float), ("max_translation_norm", C.c_float),
                ("bound_before_counter", C.c_int), ("reserved", C.c_int * 3)]


class IcpQuality(C.Structure):
    """lsgpu_icp_quality: the covariance (6x6 row major: x y z alpha beta gamma) and the pair statistics of the last alignment."""
    _fields_ = [("covariance", C.c_double * 36), ("residual", C.c_double), ("n_pairs", C.c_int64),
                ("used_ratio", C.c_float), ("reserved", C.c_int * 3)]


class ChainCfg(C.Structure):
    _fields_ = [
        ("reading_prob", C.c_float),
        ("ssn_knn", C.c_int),
        ("ssn_ratio", C.c_float),
        ("sn_knn", C.c_int),           # SurfaceNormalDataPointsFilter knn (3..32); 0: absent.  Not with ssn_knn > 0
        ("seed", C.c_int64),
    ]


class IcpConfig(C.Structure):
    _fields_ = [
        ("trim_ratio", C.c_float),
        ("max_iterations", C.c_int),
        ("min_diff_rot", C.c_float),
        ("min_diff_trans", C.c_float),
        ("smooth_length", C.c_int),
        ("cell_size", C.c_float),
        ("profile_kernels", C.c_int),
        ("reserved", C.c_int * 1),          # reserved[0] = 1 disables the trimmed-radius cap (debug)
        ("error_minimizer", C.c_int),       # MINIMIZER_*
        ("matcher_knn", C.c_int),           # KDTreeMatcher knn: 0 / 1 one neighbour, 2..MATCHER_KNN_MAX k nearest matches
        ("matcher_max_dist", C.c_float),        # KDTreeMatcher maxDist [m]; 0 / inf: absent
        ("outlier_max_dist", C.c_float),        # MaxDistOutlierFilter maxDist [m]; 0 / inf: absent
        ("outlier_min_dist", C.c_float),        # MinDistOutlierFilter minDist [m]; 0: absent
        ("outlier_median_factor", C.c_float),   # MedianDistOutlierFilter factor; 0: absent
        ("reserved_", C.c_int * 1),
    ]


class YamlParam(C.Structure):
    """lsgpu_yaml_param: one parameter of a module, the value as the scalar's text."""
    _fields_ = [("key", C.c_char_p), ("value", C.c_char_p)]


class YamlModule(C.Structure):
    """lsgpu_yaml_module: one module of a YAML chain document, as lsgpu_chain_load takes it."""
    _fields_ = [("section", C.c_char_p), ("name", C.c_char_p), ("params", C.POINTER(YamlParam)), ("n_params", C.c_int),
                ("reserved", C.c_int)]


class LoadedChain(C.Structure):
    """lsgpu_loaded_chain: what lsgpu_chain_load makes of a document."""
    _fields_ = [("icp", IcpConfig), ("chain", ChainCfg), ("robust", RobustCfg), ("has_robust", C.c_int),
                ("normals", NormalsCfg), ("has_normals", C.c_int), ("reserved", C.c_int * 6)]


class IcpStats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("converged", C.c_int),
        ("final_limit", C.c_float),
        ("final_n_used", C.c_int64),
        ("stragglers", C.c_int64),
        ("t_total_ms", C.c_double),
        ("t_knn_ms", C.c_double),
        ("knn_launches", C.c_int),
        ("t_knn_main_ms", C.c_double),
        ("t_knn_fallback_ms", C.c_double),
        ("cap_retries", C.c_int),
        ("pad_", C.c_int),
        ("t_reserved", C.c_double * 1),
        ("t_select_ms", C.c_double),
        ("t_ne_ms", C.c_double),
        ("committed_select_iterations", C.c_int),
        ("spread_tiles", C.c_int),
        ("reference_reused", C.c_int),
        ("comm_calls", C.c_int),
        ("t_comm_ms", C.c_double),
        ("direction_index_launches", C.c_int),
        ("direction_index_occupancy", C.c_float),
        ("direction_index_heavy_share", C.c_float),
    ]


class PolicyInfo(C.Structure):
    """lsgpu_policy_info: what the handle's launch policy remembers across calls."""
    _fields_ = [("index_rest", C.c_int), ("pay_voxel_us", C.c_float), ("pay_index_us", C.c_float),
                ("ssn_sort_fallbacks", C.c_int), ("ssn_calls", C.c_int), ("reserved", C.c_int * 3)]


class IterTrace(C.Structure):
    _fields_ = [
        ("T_iter", C.c_float * 16),
        ("limit", C.c_float),
        ("n_used", C.c_int64),
        ("A", C.c_double * 36),
        ("b", C.c_double * 6),
        ("x", C.c_double * 6),
        ("knn_main_us", C.c_float),
        ("knn_fallback_us", C.c_float),
        ("stragglers", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class IcpInfo(C.Structure):
    _fields_ = [
        ("n_reference", C.c_int64),
        ("bits_per_axis", C.c_int),
        ("fine_bits", C.c_int),
        ("cell_size", C.c_float),
        ("n_chunks", C.c_uint32),
        ("cells", C.c_uint32 * 17),
        ("table_bytes", C.c_uint64),
    ]


class PointFilter(C.Structure):
    """lsgpu_point_filter (include/lsgpu_icp.h): one module of the input filter chain."""
    _fields_ = [("type", C.c_int), ("dim", C.c_int), ("flag", C.c_int), ("pad_", C.c_int), ("v", C.c_float * 6),
                ("state", C.c_double)]


# the cut modules of an ICP chain's filter sections (LSGPU_CHAIN_CUT_MAX, lsgpu_chain_cuts)
CHAIN_CUT_MAX = 8


class ChainCuts(C.Structure):
    """lsgpu_chain_cuts: MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter of the two filter sections."""
    _fields_ = [("n_reading", C.c_int), ("n_reference", C.c_int), ("reading_sampling_at", C.c_int), ("reserved", C.c_int),
                ("reading", PointFilter * CHAIN_CUT_MAX), ("reference", PointFilter * CHAIN_CUT_MAX)]


class ChainModules(C.Structure):
    """lsgpu_chain_modules: a document's whole module set (lsgpu_chain_load_modules), as lsgpu_icp_set_modules applies it."""
    _fields_ = [("chain", LoadedChain), ("cuts", ChainCuts), ("shadow", ShadowCfg), ("motion", MotionCfg),
                ("cov_sampling", CovSamplingCfg), ("carried", C.c_uint), ("reserved", C.c_int * 3)]


FILTER_MAX_DIST, FILTER_MIN_DIST, FILTER_BOUNDING_BOX, FILTER_FIX_STEP_SAMPLING, FILTER_RANDOM_SAMPLING, FILTER_REMOVE_NAN = 1, 2, 3, 4, 5, 6
FILTER_VOXEL_GRID = 7   # VoxelGridDataPointsFilter: v[0..2] = vSizeX/Y/Z, flag = useCentroid, dim = averageExistingDescriptors
# OctreeGridDataPointsFilter: v[0] = maxSizeByNode, v[1] = maxPointByNode, dim = samplingMethod (OCTREE_*), flag = buildParallel
FILTER_OCTREE_GRID = 8
OCTREE_FIRST_PTS, OCTREE_RANDOM_PTS, OCTREE_CENTROID, OCTREE_MEDOID = 0, 1, 2, 3


class LsgpuError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str = ""):
        self.code = code
        super().__init__(f"{what}: {strerror(code)}" + (f" [{detail}]" if detail else ""))


class ConvergenceError(LsgpuError):
    """PointMatcher::ConvergenceError equivalent (LSGPU_NO_CONVERGENCE)."""


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C laser_slam_amd/csrc`.  There is no CPU fallback for the ICP hot path.")
    L = C.CDLL(SO_PATH)
    vp, i64, fp = C.c_void_p, C.c_int64, C.c_void_p  # data pointers passed as raw addresses
    L.lsgpu_icp_config_yaml.argtypes = [C.POINTER(IcpConfig)]
    L.lsgpu_icp_config_yaml.restype = None
    L.lsgpu_icp_config_default.argtypes = [C.POINTER(IcpConfig)]
    L.lsgpu_icp_config_default.restype = None
    L.lsgpu_icp_create.argtypes = [C.POINTER(IcpConfig), C.c_int, C.POINTER(vp)]
    L.lsgpu_icp_destroy.argtypes = [vp]
    L.lsgpu_icp_destroy.restype = None
    L.lsgpu_icp_set_reference.argtypes = [vp, fp, fp, i64]
    L.lsgpu_icp_align.argtypes = [vp, fp, i64, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(IcpStats)]
    L.lsgpu_icp_align_batch.argtypes = [C.POINTER(vp), C.c_int, i64, C.POINTER(fp), C.POINTER(fp),
                                        C.POINTER(i64), C.POINTER(fp), C.POINTER(i64),
                                        C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(IcpStats), C.POINTER(C.c_int)]
    L.lsgpu_chain_config_yaml.argtypes = [C.POINTER(ChainCfg)]
    L.lsgpu_chain_config_yaml.restype = None
    L.lsgpu_chain_config_default.argtypes = [C.POINTER(ChainCfg)]
    L.lsgpu_chain_config_default.restype = None
    L.lsgpu_icp_filter_reference.argtypes = [vp, fp, i64, C.c_int, C.c_float, i64, fp, fp, C.POINTER(i64)]
    L.lsgpu_chain_config_check.argtypes = [C.POINTER(ChainCfg), C.c_int]
    L.lsgpu_icp_filter_reference_normals.argtypes = [vp, fp, i64, C.c_int, fp, fp, fp]
    L.lsgpu_filter_surface_normal.argtypes = [fp, i64, C.c_int, fp, fp, fp]
    L.lsgpu_icp_filter_reading.argtypes = [vp, fp, i64, C.c_float, i64, fp, C.POINTER(i64)]
    L.lsgpu_icp_compute.argtypes = [vp, fp, i64, fp, i64, C.POINTER(C.c_float), C.POINTER(ChainCfg),
                                    C.POINTER(C.c_float), C.POINTER(IcpStats)]
    L.lsgpu_filter_cylinder.argtypes = [vp, fp, i64, C.POINTER(C.c_float), C.c_double, C.c_double, C.c_int, fp,
                                        C.POINTER(i64)]
    L.lsgpu_filter_voxel_grid.argtypes = [vp, fp, i64, C.POINTER(C.c_float), C.c_int, fp, C.POINTER(i64)]
    L.lsgpu_apply_point_filters.argtypes = [vp, C.POINTER(PointFilter), C.c_int, fp, i64, i64, fp, C.POINTER(i64)]
    L.lsgpu_cloud_from_pointcloud2.argtypes = [vp, fp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp,
                                               C.POINTER(i64)]
    L.lsgpu_cloud_to_pointxyz.argtypes = [vp, fp, i64, fp]
    L.lsgpu_cloud_upload.argtypes = [vp, C.c_int, fp, i64]
    L.lsgpu_cloud_release.argtypes = [vp, C.c_int]
    L.lsgpu_cloud_size.argtypes = [vp, C.c_int, C.POINTER(i64)]
    L.lsgpu_icp_compute_clouds.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                           C.POINTER(C.c_float), C.POINTER(ChainCfg), C.POINTER(C.c_float),
                                           C.POINTER(IcpStats)]
    L.lsgpu_icp_compute_clouds_upload.argtypes = [vp, C.c_int, fp, i64, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                                  C.POINTER(C.c_float), C.POINTER(ChainCfg), C.POINTER(C.c_float),
                                                  C.POINTER(IcpStats)]
    L.lsgpu_icp_get_trace.argtypes = [vp, C.POINTER(IterTrace), C.c_int]
    L.lsgpu_icp_get_reference_mean.argtypes = [vp, C.POINTER(C.c_float)]
    L.lsgpu_icp_get_info.argtypes = [vp, C.POINTER(IcpInfo)]
    L.lsgpu_icp_get_policy_info.argtypes = [vp, C.POINTER(PolicyInfo)]
    L.lsgpu_icp_get_policy_info.restype = C.c_int
    L.lsgpu_comm_get_unique_id.argtypes = [C.c_char_p]
    L.lsgpu_icp_comm_init.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.lsgpu_knn.argtypes = [vp, fp, i64, C.POINTER(C.c_float), fp, fp]
    L.lsgpu_knn_k.argtypes = [vp, fp, i64, C.POINTER(C.c_float), C.c_int, fp, fp]
    L.lsgpu_trim_limit.argtypes = [vp, fp, i64, C.c_float, C.POINTER(C.c_float)]
    L.lsgpu_normal_eq.argtypes = [vp, fp, i64, C.POINTER(C.c_float), fp, fp, C.c_float,
                                  C.POINTER(C.c_double)]
    L.lsgpu_point_to_point.argtypes = [vp, fp, i64, C.POINTER(C.c_float), fp, fp, C.c_float,
                                       C.POINTER(C.c_double)]
    L.lsgpu_point_to_point_solve.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.lsgpu_transform_points.argtypes = [vp, C.POINTER(C.c_float), fp, i64, fp]
    L.lsgpu_rotate_descriptors.argtypes = [vp, C.POINTER(C.c_float), fp, i64, fp]
    L.lsgpu_filter_random_sampling.argtypes = [i64, C.c_float, i64, C.POINTER(C.c_int64)]
    L.lsgpu_filter_random_sampling.restype = i64
    L.lsgpu_filter_sampling_surface_normal.argtypes = [fp, i64, C.c_int, C.c_float, i64, fp, fp]
    L.lsgpu_filter_sampling_surface_normal.restype = i64
    L.lsgpu_filter_voxel_grid_points.argtypes = [fp, i64, C.POINTER(C.c_float), C.c_int, fp]
    L.lsgpu_filter_voxel_grid_points.restype = i64
    L.lsgpu_filter_octree_grid_points.argtypes = [fp, i64, C.c_float, C.c_int, C.c_int, i64, fp]
    L.lsgpu_filter_octree_grid_points.restype = i64
    L.lsgpu_check_rigid.argtypes = [C.POINTER(C.c_float)]
    L.lsgpu_rotation_distance.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.lsgpu_rotation_distance.restype = C.c_float
    L.lsgpu_correct_rigid.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.lsgpu_correct_rigid.restype = None
    L.lsgpu_strerror.argtypes = [C.c_int]
    L.lsgpu_strerror.restype = C.c_char_p
    L.lsgpu_last_error.argtypes = [vp]
    L.lsgpu_last_error.restype = C.c_char_p
    L.lsgpu_abi_version.restype = C.c_int
    L.lsgpu_robust_config_default.argtypes = [C.POINTER(RobustCfg)]
    L.lsgpu_robust_config_default.restype = None
    L.lsgpu_robust_config_check.argtypes = [C.POINTER(RobustCfg), C.c_int, C.c_int]
    L.lsgpu_icp_set_robust_filter.argtypes = [vp, C.POINTER(RobustCfg)]
    L.lsgpu_robust_scale.argtypes = [fp, i64, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.lsgpu_robust_weights.argtypes = [C.POINTER(RobustCfg), C.c_float, fp, i64, fp]
    L.lsgpu_icp_get_robust_trace.argtypes = [vp, C.POINTER(RobustTrace), C.c_int]
    L.lsgpu_point_to_plane_solve.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.lsgpu_normals_config_default.argtypes = [C.POINTER(NormalsCfg)]
    L.lsgpu_normals_config_default.restype = None
    L.lsgpu_normals_config_check.argtypes = [C.POINTER(NormalsCfg), C.c_int, C.c_int]
    L.lsgpu_icp_set_normals.argtypes = [vp, C.POINTER(NormalsCfg)]
    L.lsgpu_icp_reading_normals.argtypes = [vp, fp, i64, C.c_int, C.c_int, C.POINTER(C.c_float), fp]
    L.lsgpu_icp_align_normals.argtypes = [vp, fp, i64, fp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(IcpStats)]
    L.lsgpu_icp_get_reference_normals.argtypes = [vp, fp, i64]
    L.lsgpu_orient_normals.argtypes = [fp, i64, C.POINTER(C.c_float), C.c_int, fp]
    L.lsgpu_normal_angle_weights.argtypes = [C.POINTER(C.c_float), fp, i64, fp, vp, C.c_int, C.c_float, fp]
    L.lsgpu_icp_get_normal_angle_trace.argtypes = [vp, C.POINTER(NormalAngleTrace), C.c_int]
    L.lsgpu_chain_load.argtypes = [C.POINTER(YamlModule), C.c_int, C.POINTER(LoadedChain), C.c_char_p, C.c_int]
    L.lsgpu_robust_config_why.argtypes = [C.POINTER(RobustCfg), C.c_int, C.c_int]
    L.lsgpu_robust_config_why.restype = C.c_char_p
    L.lsgpu_normals_config_why.argtypes = [C.POINTER(NormalsCfg), C.c_int, C.c_int]
    L.lsgpu_normals_config_why.restype = C.c_char_p
    L.lsgpu_covariance_config_default.argtypes = [C.POINTER(CovarianceCfg)]
    L.lsgpu_covariance_config_default.restype = None
    L.lsgpu_icp_set_covariance.argtypes = [vp, C.POINTER(CovarianceCfg)]
    L.lsgpu_icp_get_quality.argtypes = [vp, C.POINTER(IcpQuality)]
    L.lsgpu_point_to_plane_cov.argtypes = [vp, fp, i64, C.POINTER(C.c_float), fp, fp, C.c_float, C.POINTER(C.c_float),
                                           C.POINTER(C.c_double)]
    L.lsgpu_point_to_plane_cov_solve.argtypes = [C.POINTER(C.c_double), C.c_float, C.POINTER(C.c_double)]
    L.lsgpu_loaded_chain_covariance.argtypes = [C.POINTER(LoadedChain), C.POINTER(C.c_float)]
    L.lsgpu_icp_set_chain_cuts.argtypes = [vp, C.POINTER(ChainCuts)]
    L.lsgpu_icp_filter_section.argtypes = [vp, C.POINTER(ChainCuts), C.c_int, C.c_float, fp, i64, i64, fp, C.POINTER(i64)]
    L.lsgpu_chain_load_cuts.argtypes = [C.POINTER(YamlModule), C.c_int, C.POINTER(ChainCuts), C.c_char_p, C.c_int]
    L.lsgpu_max_density_config_default.argtypes = [C.POINTER(MaxDensityCfg)]
    L.lsgpu_max_density_config_default.restype = None
    L.lsgpu_max_density_config_check.argtypes = [C.POINTER(MaxDensityCfg), C.c_int]
    L.lsgpu_max_density_config_why.argtypes = [C.POINTER(MaxDensityCfg), C.c_int]
    L.lsgpu_max_density_config_why.restype = C.c_char_p
    L.lsgpu_icp_set_max_density.argtypes = [vp, C.POINTER(MaxDensityCfg)]
    L.lsgpu_icp_filter_reference_normals_densities.argtypes = [vp, fp, i64, C.c_int, fp, fp, fp, fp]
    L.lsgpu_icp_filter_reference_max_density.argtypes = [vp, fp, i64, C.c_int, C.c_float, i64, fp, fp, fp, C.POINTER(i64),
                                                         C.POINTER(i64)]
    L.lsgpu_filter_surface_normal_densities.argtypes = [fp, i64, C.c_int, fp, fp, fp, fp]
    L.lsgpu_filter_max_density.argtypes = [fp, i64, C.c_int, C.c_float, i64, fp, fp, fp, C.POINTER(i64), C.POINTER(i64)]
    L.lsgpu_loaded_chain_max_density.argtypes = [C.POINTER(LoadedChain), C.POINTER(C.c_float)]
    L.lsgpu_shadow_config_default.argtypes = [C.POINTER(ShadowCfg)]
    L.lsgpu_shadow_config_default.restype = None
    L.lsgpu_shadow_config_check.argtypes = [C.POINTER(ShadowCfg)]
    L.lsgpu_shadow_config_why.argtypes = [C.POINTER(ShadowCfg)]
    L.lsgpu_shadow_config_why.restype = C.c_char_p
    L.lsgpu_icp_set_shadow.argtypes = [vp, C.POINTER(ShadowCfg)]
    L.lsgpu_icp_filter_shadow.argtypes = [vp, fp, fp, i64, C.c_float, fp, fp, C.POINTER(i64)]
    L.lsgpu_filter_shadow.argtypes = [fp, fp, i64, C.c_float, fp, fp, C.POINTER(i64)]
    L.lsgpu_chain_load_shadow.argtypes = [C.POINTER(YamlModule), C.c_int, C.POINTER(ShadowCfg), C.c_char_p, C.c_int]
    L.lsgpu_icp_filter_cov_sampling.argtypes = [vp, fp, fp, i64, C.c_int, C.c_int, fp, fp, vp, C.POINTER(i64), vp]
    L.lsgpu_icp_cov_sampling_phase_ms.argtypes = [vp, C.POINTER(C.c_double)]
    L.lsgpu_filter_cov_sampling.argtypes = [fp, fp, i64, C.c_int, C.c_int, vp, fp, fp, vp, C.POINTER(i64), vp]
    L.lsgpu_cov_sampling_eigen.argtypes = [vp, vp, vp]
    L.lsgpu_cov_sampling_config_default.argtypes = [C.POINTER(CovSamplingCfg)]
    L.lsgpu_cov_sampling_config_default.restype = None
    L.lsgpu_cov_sampling_config_check.argtypes = [C.POINTER(CovSamplingCfg)]
    L.lsgpu_cov_sampling_config_why.argtypes = [C.POINTER(CovSamplingCfg)]
    L.lsgpu_cov_sampling_config_why.restype = C.c_char_p
    L.lsgpu_icp_set_cov_sampling.argtypes = [vp, C.POINTER(CovSamplingCfg)]
    L.lsgpu_chain_load_cov_sampling.argtypes = [C.POINTER(YamlModule), C.c_int, C.POINTER(CovSamplingCfg), C.c_char_p, C.c_int]
    L.lsgpu_motion_config_default.argtypes = [C.POINTER(MotionCfg)]
    L.lsgpu_motion_config_default.restype = None
    L.lsgpu_motion_config_check.argtypes = [C.POINTER(MotionCfg)]
    L.lsgpu_motion_config_why.argtypes = [C.POINTER(MotionCfg)]
    L.lsgpu_motion_config_why.restype = C.c_char_p
    L.lsgpu_icp_set_motion.argtypes = [vp, C.POINTER(MotionCfg)]
    L.lsgpu_point_to_plane_solve_dof.argtypes = [C.POINTER(C.c_double), C.c_int, fp]
    L.lsgpu_bound_first_violation.argtypes = [fp, C.c_int, C.c_float, C.c_float]
    L.lsgpu_chain_load_motion.argtypes = [C.POINTER(YamlModule), C.c_int, C.POINTER(MotionCfg), C.c_char_p, C.c_int]
    L.lsgpu_cloud_upload_normals.argtypes = [vp, C.c_int, fp, fp, i64]
    L.lsgpu_cloud_has_normals.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.lsgpu_cloud_ingest.argtypes = [vp, C.c_int, C.POINTER(PointFilter), C.c_int, fp, i64, i64, C.c_int, C.c_int,
                                     C.POINTER(C.c_float), fp, fp, C.POINTER(i64)]
    L.lsgpu_cloud_download.argtypes = [vp, C.c_int, fp, fp, i64]
    L.lsgpu_icp_compute_normals.argtypes = [vp, fp, fp, i64, fp, fp, i64, C.POINTER(C.c_float), C.POINTER(ChainCfg),
                                            C.POINTER(C.c_float), C.POINTER(IcpStats)]
    L.lsgpu_icp_compute_clouds_upload_normals.argtypes = [vp, C.c_int, fp, fp, i64, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int,
                                                          C.POINTER(C.c_float), C.POINTER(ChainCfg), C.POINTER(C.c_float),
                                                          C.POINTER(IcpStats)]
    L.lsgpu_chain_load_carried.argtypes = [C.POINTER(YamlModule), C.c_int, C.c_uint, C.POINTER(LoadedChain), C.c_char_p, C.c_int]
    L.lsgpu_chain_load_parts_carried.argtypes = [C.POINTER(YamlModule), C.c_int, C.c_uint, C.POINTER(ChainCuts), C.POINTER(ShadowCfg),
                                                 C.POINTER(MotionCfg), C.POINTER(CovSamplingCfg), C.c_char_p, C.c_int]
    L.lsgpu_chain_load_modules.argtypes = [C.POINTER(YamlModule), C.c_int, C.c_uint, C.POINTER(ChainModules), C.c_char_p, C.c_int]
    L.lsgpu_icp_set_modules.argtypes = [vp, C.POINTER(ChainModules)]
    L.lsgpu_surface_normal_params_check.argtypes = [C.POINTER(YamlParam), C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    _lib = L
    return L


def strerror(code: int) -> str:
    return lib().lsgpu_strerror(code).decode()
