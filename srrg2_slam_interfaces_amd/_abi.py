"""ctypes mirror of the PODs and enums in include/srrg2_slam_amd.h.

Shared by the product binding (``_capi.py``) and by the test-side oracle binding
(``oracle/pyoracle.py``); it contains declarations only, no behaviour.
"""
import ctypes as C

ABI_VERSION = 4
MAX_SLICES = 8

# enum srrg2_variable_kind  (S/registration/aligners/multi_aligner.h:152-158)
SE2_RIGHT, SE3_EULER_RIGHT, SE3_QUAT_RIGHT = 0, 1, 2
# enum srrg2_status  (S/registration/aligners/aligner.h:23-28)
SUCCESS, NOT_ENOUGH_CORRESPONDENCES, NOT_ENOUGH_INLIERS, FAIL = 0, 1, 2, 3
# enum srrg2_slice_kind
SLICE_P2P, SLICE_P2PLANE, SLICE_REPROJECTION, SLICE_PRIOR = 0, 1, 2, 3
# enum srrg2_finder_kind
FINDER_NONE, FINDER_NN_GATED, FINDER_PROJECTIVE, FINDER_CORRESPONDENCES = 0, 1, 2, 3
# enum srrg2_robustifier_kind
ROBUST_NONE, ROBUST_CLAMP, ROBUST_SATURATED, ROBUST_CAUCHY = 0, 1, 2, 3
# enum srrg2_factor_status
FACTOR_INLIER, FACTOR_KERNELIZED, FACTOR_SUPPRESSED = 0, 1, 2
# enum srrg2_mem
MEM_HOST, MEM_DEVICE, MEM_DEVICE_KEPT = 0, 1, 2


class Correspondence(C.Structure):
    _fields_ = [("fixed_idx", C.c_int32), ("moving_idx", C.c_int32), ("response", C.c_float)]


class IterationStats(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32),
        ("num_inliers", C.c_int32),
        ("num_outliers", C.c_int32),
        ("num_suppressed", C.c_int32),
        ("num_correspondences", C.c_int32),
        ("solver_status", C.c_int32),
        ("chi_inliers", C.c_float),
        ("chi_outliers", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class AlignerParams(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("min_num_inliers", C.c_int32),
        ("enable_inlier_only_runs", C.c_int32),
        ("keep_only_inlier_correspondences", C.c_int32),
    ]


class TerminationParams(C.Structure):
    _fields_ = [
        ("window_size", C.c_int32),
        ("num_correspondences_range", C.c_int32),
        ("num_inliers_range", C.c_int32),
        ("num_outliers_range", C.c_int32),
        ("chi_epsilon", C.c_float),
    ]


class SliceConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("finder", C.c_int32),
        ("robustifier", C.c_int32),
        ("robustifier_chi_threshold", C.c_float),
        ("min_num_correspondences", C.c_int32),
        ("finder_max_distance", C.c_float),
        ("finder_normal_cos", C.c_float),
        ("finder_cell_size", C.c_float),
        ("sensor_in_robot", C.c_float * 12),
        ("camera_matrix", C.c_float * 9),
        ("image_rows", C.c_int32),
        ("image_cols", C.c_int32),
        ("depth_min", C.c_float),
        ("depth_max", C.c_float),
        ("prior_information_diag", C.c_float * 6),
        ("prior_sets_initial_guess", C.c_int32),
    ]


class BatchResult(C.Structure):
    _fields_ = [
        ("moving_in_fixed", C.c_float * 12),
        ("status", C.c_int32),
        ("num_iterations", C.c_int32),
        ("last", IterationStats),
        ("num_correspondences", C.c_int32),
        ("reserved_", C.c_int32),
        ("information", C.c_float * 36),
    ]


class BatchSliceClouds(C.Structure):
    """srrg2_batch_slice_clouds: one slice's K moving clouds in a srrg2_align_batch_slices call (all null: no entry)"""
    _fields_ = [
        ("coords", C.POINTER(C.c_float)),
        ("coord_stride_bytes", C.c_int32),
        ("normals", C.POINTER(C.c_float)),
        ("normal_stride_bytes", C.c_int32),
        ("offsets", C.POINTER(C.c_int32)),
    ]


# srrg2_aligner_tuning.strategy_mask: the only bits srrg2_aligner_set_tuning accepts (each forces a path the library also
# takes by itself on other configurations)
TUNE_PROJ_SEPARATE_LAUNCHES = 1 << 17  # projective slices in launches of their own
TUNE_INIT_LAUNCH = 1 << 23  # the k_icp_init launch in front of every compute()


class AlignerTuning(C.Structure):
    """srrg2_aligner_tuning: strategy knobs, every setting gives the same results (include/srrg2_slam_amd.h)"""
    _fields_ = [
        ("strategy_mask", C.c_int32),
        ("queue_probe_iteration", C.c_int32),
        ("small_max_points", C.c_int32),
        ("fast_from_iteration", C.c_int32),
        ("fast_points_per_thread", C.c_int32),
        ("fast_min_points", C.c_int32),
        ("fast_gather", C.c_int32),
        ("fast_batch_queue", C.c_int32),
        ("queue_min_points", C.c_int32),
        ("msort_segments", C.c_int32),
        ("msort_key_bits", C.c_int32),
        ("lds_tile", C.c_int32),
        ("cell_target", C.c_float),
        ("rmax_cap", C.c_float),
        ("search_lists", C.c_int32),
        ("search_team", C.c_int32),
        ("batch_pipeline", C.c_int32),
        ("fused_control", C.c_int32),
        ("reserved_", C.c_int32 * 6),
    ]


# enum srrg2_adaptor_status (RawDataPreprocessor_::Status, raw_data_preprocessor.h:22), enum srrg2_image_type
ADAPTOR_READY, ADAPTOR_INITIALIZING, ADAPTOR_ERROR = 0, 1, 2
IMAGE_NONE, IMAGE_U8, IMAGE_U16, IMAGE_F32 = 0, 1, 2, 3


class DepthAdaptorParams(C.Structure):
    """srrg2_depth_adaptor_params"""
    _fields_ = [
        ("camera_matrix", C.c_float * 9),
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("depth_scale", C.c_float),
        ("depth_min", C.c_float),
        ("depth_max", C.c_float),
        ("normal_col_gap", C.c_int32),
        ("normal_row_gap", C.c_int32),
        ("normal_max_distance_squared", C.c_float),
        ("drop_points_without_normal", C.c_int32),
        ("compact", C.c_int32),
    ]


class ScanAdaptorParams(C.Structure):
    """srrg2_scan_adaptor_params"""
    _fields_ = [
        ("angle_min", C.c_double),
        ("angle_increment", C.c_double),
        ("range_min", C.c_float),
        ("range_max", C.c_float),
        ("normal_half_window", C.c_int32),
        ("normal_max_distance_squared", C.c_float),
        ("drop_points_without_normal", C.c_int32),
        ("compact", C.c_int32),
    ]


class SphericalModel(C.Structure):
    """srrg2_spherical_model: the range image of a spinning 3-D lidar (rows = rings, cols = azimuth steps)"""
    _fields_ = [("azimuth_min", C.c_double), ("azimuth_increment", C.c_double), ("elevation_min", C.c_double),
                ("elevation_increment", C.c_double), ("rows", C.c_int32), ("cols", C.c_int32), ("range_min", C.c_float),
                ("range_max", C.c_float)]


class LidarAdaptorParams(C.Structure):
    """srrg2_lidar_adaptor_params"""
    _fields_ = [("model", SphericalModel), ("normal_col_gap", C.c_int32), ("normal_row_gap", C.c_int32),
                ("normal_max_distance_squared", C.c_float), ("drop_points_without_normal", C.c_int32), ("compact", C.c_int32),
                ("reserved", C.c_int32)]


class LidarSweepExtras(C.Structure):
    """srrg2_lidar_sweep_extras: ring elevation table (host doubles) and motion de-skew of srrg2_adapt_lidar_sweep_ex"""
    _fields_ = [("ring_elevations", C.POINTER(C.c_double)), ("times", C.c_void_p), ("time_stride_bytes", C.c_int32),
                ("deskew", C.c_int32), ("time_begin", C.c_double), ("time_end", C.c_double), ("reference", C.c_double),
                ("motion", C.c_float * 12), ("reserved", C.c_int32 * 2)]


class SphericalClipParams(C.Structure):
    """srrg2_spherical_clip_params"""
    _fields_ = [("model", SphericalModel), ("sensor_in_robot", C.c_float * 12), ("occlusion_margin", C.c_float),
                ("reserved", C.c_int32)]


class AdaptResult(C.Structure):
    """srrg2_adapt_result"""
    _fields_ = [("status", C.c_int32), ("num_raw", C.c_int32), ("num_in_range", C.c_int32), ("num_valid", C.c_int32),
                ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FeatureParams(C.Structure):
    """srrg2_feature_params"""
    _fields_ = [("fast_threshold", C.c_int32), ("max_features", C.c_int32), ("oriented", C.c_int32), ("reserved", C.c_int32)]


class Keypoint(C.Structure):
    """srrg2_keypoint"""
    _fields_ = [("pixel", C.c_int32), ("score", C.c_int32), ("angle_bin", C.c_int32), ("reserved", C.c_int32)]


class FeatureResult(C.Structure):
    """srrg2_feature_result"""
    _fields_ = [("status", C.c_int32), ("num_pixels", C.c_int32), ("num_candidates", C.c_int32), ("num_maxima", C.c_int32),
                ("num_selected", C.c_int32), ("num_with_depth", C.c_int32), ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PyramidParams(C.Structure):
    """srrg2_pyramid_params"""
    _fields_ = [("num_levels", C.c_int32), ("scale_num", C.c_int32), ("scale_den", C.c_int32), ("reserved", C.c_int32)]


class PyramidKeypoint(C.Structure):
    """srrg2_pyramid_keypoint"""
    _fields_ = [("pixel", C.c_int32), ("score", C.c_int32), ("angle_bin", C.c_int32), ("level", C.c_int32),
                ("level_pixel", C.c_int32), ("u_q8", C.c_int32), ("v_q8", C.c_int32), ("reserved", C.c_int32)]


PYRAMID_MAX_LEVELS = 8


class PyramidResult(C.Structure):
    """srrg2_pyramid_result"""
    _fields_ = [("status", C.c_int32), ("num_levels_built", C.c_int32), ("scene_size", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_int32 * PYRAMID_MAX_LEVELS) for n in ("rows", "cols", "num_candidates", "num_maxima", "num_selected",
                                                              "num_with_depth", "quota")]

    def as_dict(self):
        """the scalars as they are, the per-level arrays as lists of num_levels_built entries"""
        out = {n: getattr(self, n) for n, _ in self._fields_[:4]}
        out.update({n: list(getattr(self, n))[:self.num_levels_built] for n, _ in self._fields_[4:]})
        return out


class StereoParams(C.Structure):
    """srrg2_stereo_params"""
    _fields_ = [("baseline", C.c_float), ("min_disparity", C.c_int32), ("max_disparity", C.c_int32), ("row_tolerance", C.c_int32),
                ("max_distance", C.c_int32), ("cross_check", C.c_int32), ("subpixel", C.c_int32), ("reserved", C.c_int32)]


class DenseStereoParams(C.Structure):
    """srrg2_dense_stereo_params"""
    _fields_ = [("baseline", C.c_float), ("min_disparity", C.c_int32), ("max_disparity", C.c_int32), ("paths", C.c_int32),
                ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness_ratio", C.c_int32), ("lr_check", C.c_int32),
                ("lr_tolerance", C.c_int32), ("subpixel", C.c_int32), ("reserved", C.c_int32)]


class DenseStereoResult(C.Structure):
    """srrg2_dense_stereo_result"""
    _fields_ = [("status", C.c_int32), ("num_pixels", C.c_int32), ("num_evaluated", C.c_int32), ("num_unique", C.c_int32),
                ("num_consistent", C.c_int32), ("num_in_range", C.c_int32), ("num_valid", C.c_int32), ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RectifierParams(C.Structure):
    """srrg2_rectifier_params"""
    _fields_ = [("camera_matrix", C.c_double * 9), ("distortion", C.c_double * 8), ("rotation", C.c_double * 9),
                ("new_camera_matrix", C.c_double * 9), ("src_rows", C.c_int32), ("src_cols", C.c_int32), ("dst_rows", C.c_int32),
                ("dst_cols", C.c_int32)]


class RectifierInfo(C.Structure):
    """srrg2_rectifier_info"""
    _fields_ = [("num_pixels", C.c_int32), ("num_valid", C.c_int32), ("first_row", C.c_int32), ("last_row", C.c_int32),
                ("first_col", C.c_int32), ("last_col", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GridMapParams(C.Structure):
    """srrg2_gridmap_params"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("resolution", C.c_float), ("origin", C.c_float * 2)]


class GridMapScanParams(C.Structure):
    """srrg2_gridmap_scan_params"""
    _fields_ = [("angle_min", C.c_double), ("angle_increment", C.c_double), ("num_beams", C.c_int32), ("range_min", C.c_float),
                ("range_max", C.c_float), ("sensor_in_robot", C.c_float * 9), ("clear_beyond_max", C.c_int32)]


class GridMapResult(C.Structure):
    """srrg2_gridmap_result"""
    _fields_ = [("num_beams_total", C.c_int64), ("num_returns", C.c_int64), ("num_cleared_only", C.c_int64),
                ("num_skipped", C.c_int64), ("num_hits_in_grid", C.c_int64), ("num_miss_updates", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GridMapMatchParams(C.Structure):
    """srrg2_gridmap_match_params"""
    _fields_ = [("half_window_x", C.c_int32), ("half_window_y", C.c_int32), ("half_steps_theta", C.c_int32), ("reserved", C.c_int32),
                ("theta_step", C.c_double)]


class GridMapMatchResult(C.Structure):
    """srrg2_gridmap_match_result"""
    _fields_ = [("robot_in_world", C.c_float * 9), ("dx", C.c_int32), ("dy", C.c_int32), ("jtheta", C.c_int32), ("score", C.c_int32),
                ("score_at_guess", C.c_int32), ("num_scored_beams", C.c_int32)]


class GridMapPruneParams(C.Structure):
    """srrg2_gridmap_prune_params"""
    _fields_ = [("num_levels", C.c_int32), ("max_list_entries", C.c_int32)]


class GridMapPruneStats(C.Structure):
    """srrg2_gridmap_prune_stats"""
    _fields_ = [("num_candidates", C.c_int32), ("num_evaluated", C.c_int32 * 7), ("num_survivors", C.c_int32 * 7),
                ("floor_score", C.c_int32), ("seed_block", C.c_int32), ("fell_back", C.c_int32)]

    def as_dict(self):
        return {"num_candidates": self.num_candidates, "num_evaluated": list(self.num_evaluated), "num_survivors": list(self.num_survivors),
                "floor_score": self.floor_score, "seed_block": self.seed_block, "fell_back": self.fell_back}


class TsdfParams(C.Structure):
    """srrg2_tsdf_params"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("voxel_size", C.c_float), ("origin", C.c_float * 3),
                ("with_intensity", C.c_int32)]


class TsdfFrameParams(C.Structure):
    """srrg2_tsdf_frame_params"""
    _fields_ = [("mu", C.c_float), ("reserved", C.c_int32)]


class TsdfRaycastParams(C.Structure):
    """srrg2_tsdf_raycast_params"""
    _fields_ = [("step", C.c_float), ("min_weight", C.c_int32), ("skip_empty", C.c_int32), ("reserved", C.c_int32)]


class TsdfResult(C.Structure):
    """srrg2_tsdf_result"""
    _fields_ = [("num_frames", C.c_int64), ("num_pixels", C.c_int64), ("num_valid_depth", C.c_int64), ("num_voxel_updates", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TsdfRaycastResult(C.Structure):
    """srrg2_tsdf_raycast_result"""
    _fields_ = [("num_pixels", C.c_int32), ("num_surface", C.c_int32), ("adapt", AdaptResult)]

    def as_dict(self):
        return {"num_pixels": self.num_pixels, "num_surface": self.num_surface, "adapt": self.adapt.as_dict()}


class TsdfExportResult(C.Structure):
    """srrg2_tsdf_export_result"""
    _fields_ = [("num_points", C.c_int32), ("reserved", C.c_int32)]


class StereoMatch(C.Structure):
    """srrg2_stereo_match"""
    _fields_ = [("left_pixel", C.c_int32), ("right_pixel", C.c_int32), ("distance", C.c_int32), ("disparity", C.c_float)]


class StereoResult(C.Structure):
    """srrg2_stereo_result"""
    _fields_ = [("status", C.c_int32), ("num_pixels", C.c_int32), ("num_left", C.c_int32), ("num_right", C.c_int32),
                ("num_matched", C.c_int32), ("num_mutual", C.c_int32), ("num_in_range", C.c_int32), ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TrackParams(C.Structure):
    """srrg2_track_params"""
    _fields_ = [("camera_matrix", C.c_float * 9), ("image_rows", C.c_int32), ("image_cols", C.c_int32), ("depth_min", C.c_float),
                ("depth_max", C.c_float), ("search_radius", C.c_int32), ("max_distance", C.c_int32), ("min_margin", C.c_int32),
                ("cross_check", C.c_int32), ("reserved", C.c_int32)]


class TrackResult(C.Structure):
    """srrg2_track_result"""
    _fields_ = [("num_moving", C.c_int32), ("num_fixed", C.c_int32), ("num_in_view", C.c_int32), ("num_with_candidate", C.c_int32),
                ("num_accepted", C.c_int32), ("num_mutual", C.c_int32), ("num_correspondences", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# enum srrg2_consensus_status
CONSENSUS_FOUND, CONSENSUS_NO_HYPOTHESIS, CONSENSUS_TOO_FEW_INLIERS = 0, 1, 2


class ConsensusParams(C.Structure):
    """srrg2_consensus_params (32 bytes)"""
    _fields_ = [("num_hypotheses", C.c_int32), ("inlier_distance", C.c_float), ("min_sample_distance", C.c_float),
                ("min_inliers", C.c_int32), ("seed", C.c_uint32), ("length_check", C.c_int32), ("reserved", C.c_int32 * 2)]


class ConsensusResult(C.Structure):
    """srrg2_consensus_result (96 bytes)"""
    _fields_ = [("moving_in_fixed", C.c_float * 12), ("status", C.c_int32), ("best_hypothesis", C.c_int32), ("num_inliers", C.c_int32),
                ("num_pairs", C.c_int32), ("num_valid_pairs", C.c_int32), ("num_degenerate", C.c_int32), ("num_rejected", C.c_int32),
                ("num_scored", C.c_int32), ("cost_exponent", C.c_int32), ("reserved", C.c_int32), ("cost", C.c_int64)]


assert C.sizeof(ConsensusParams) == 32 and C.sizeof(ConsensusResult) == 96


class NormalsParams(C.Structure):
    """srrg2_normals_params"""
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_int32), ("max_curvature", C.c_float), ("viewpoint", C.c_float * 3),
                ("drop_points_without_normal", C.c_int32), ("reserved", C.c_int32)]


class NormalsResult(C.Structure):
    """srrg2_normals_result"""
    _fields_ = [("num_points", C.c_int32), ("num_finite", C.c_int32), ("num_with_normal", C.c_int32), ("num_too_few", C.c_int32),
                ("num_degenerate", C.c_int32), ("num_too_curved", C.c_int32), ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


VOXEL_CENTROID, VOXEL_FIRST = 0, 1


class VoxelParams(C.Structure):
    """srrg2_voxel_params"""
    _fields_ = [("leaf_size", C.c_float), ("origin", C.c_float * 3), ("mode", C.c_int32), ("min_points_per_voxel", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class VoxelResult(C.Structure):
    """srrg2_voxel_result"""
    _fields_ = [("num_points", C.c_int32), ("num_finite", C.c_int32), ("num_occupied", C.c_int32), ("num_voxels", C.c_int32),
                ("num_with_normal", C.c_int32), ("max_points_per_voxel", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def transform_size(variable_kind):
    return 9 if variable_kind == SE2_RIGHT else 12


def point_dim(variable_kind):
    return 2 if variable_kind == SE2_RIGHT else 3


def default_aligner_params():
    # aligner.h:30; multi_aligner.h:45-57
    return AlignerParams(10, 10, 0, 0)


def default_termination_params():
    # aligner_termination_criteria.h:40-56
    return TerminationParams(5, 20, 20, 20, 0.2)


def default_slice_config(variable_kind):
    c = SliceConfig()
    c.kind = SLICE_P2P
    c.finder = FINDER_NN_GATED
    c.robustifier = ROBUST_NONE
    c.robustifier_chi_threshold = 1.0
    c.min_num_correspondences = 0  # aligner_slice_processor.h:62-66
    c.finder_max_distance = 1.0
    c.finder_normal_cos = -2.0
    c.finder_cell_size = 0.0
    ident = [1, 0, 0, 0, 1, 0, 0, 0, 1] if variable_kind == SE2_RIGHT else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    for i, v in enumerate(ident):
        c.sensor_in_robot[i] = v
    for i in range(6):
        # aligner_slice_odometry_prior.h:17-21 (2D: 1e2) and :41-45 (3D: 1)
        c.prior_information_diag[i] = 100.0 if variable_kind == SE2_RIGHT else 1.0
    c.prior_sets_initial_guess = 1
    return c

# srrg2_aligner_last_compute_path (strategy introspection: what the path tests assert)
PATH_FUSED_CONTROL, PATH_ALL_PASSES_FUSED, PATH_FINAL_WAVE, PATH_PROLOGUE_IN_PASS, PATH_ONE_WORKGROUP, PATH_PRIORS_FUSED = 1, 2, 4, 8, 16, 32
