"""ctypes loader of the product library (lib/libsrrg2_slam_amd.so = HIP kernels + C ABI).

There is NO fallback: if the shared library is missing or cannot be loaded this raises, and
creating an aligner without a HIP device fails with SRRG2_E_NO_DEVICE.  The CPU oracle under
oracle/ is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

from .aligner import Backend

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SRRG2_AMD_LIB: an instrumented build of the same sources for profiling -- make OUT=... EXTRA=-DSRRG2_TILE_STATS; never a fallback)
LIB_PATH = os.environ.get("SRRG2_AMD_LIB") or os.path.join(_HERE, "lib", "libsrrg2_slam_amd.so")
_LIB = None


class LibraryMissing(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C srrg2_slam_interfaces_amd/csrc` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        _LIB = C.CDLL(LIB_PATH)
        _LIB.srrg2_amd_last_error.restype = C.c_char_p
        _LIB.srrg2_aligner_profile_get.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]
        # srrg2_descriptor_db_* (descriptors.DescriptorDatabase): float / int64 arguments need their types
        u8p = C.POINTER(C.c_uint8)
        _LIB.srrg2_descriptor_db_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _LIB.srrg2_descriptor_db_destroy.argtypes = [C.c_void_p]
        _LIB.srrg2_descriptor_db_add.argtypes = [C.c_void_p, u8p, u8p, C.c_int, C.POINTER(C.c_int)]
        _LIB.srrg2_descriptor_db_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
        _LIB.srrg2_descriptor_db_match.argtypes = [C.c_void_p, u8p, u8p, C.c_int, C.c_int64, C.c_float, C.c_uint32,
                                                   C.c_int64, C.POINTER(C.c_int)]
        _LIB.srrg2_descriptor_db_get_candidates.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                                            C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        _LIB.srrg2_descriptor_db_get_correspondences.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        _LIB.srrg2_descriptor_db_get_map_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        _LIB.srrg2_descriptor_db_last_match_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _LIB.srrg2_descriptor_db_add_scene.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        _LIB.srrg2_descriptor_db_match_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_uint32, C.c_int64,
                                                         C.POINTER(C.c_int)]
        # srrg2_adapt_* (adaptors.MeasurementAdaptorDepthImage / MeasurementAdaptorLaserScan)
        from . import _abi as abi

        _LIB.srrg2_adapt_default_depth_params.argtypes = [C.POINTER(abi.DepthAdaptorParams)]
        _LIB.srrg2_adapt_default_depth_params.restype = None
        _LIB.srrg2_adapt_default_scan_params.argtypes = [C.POINTER(abi.ScanAdaptorParams)]
        _LIB.srrg2_adapt_default_scan_params.restype = None
        _LIB.srrg2_adapt_depth_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.AdaptResult)]
        _LIB.srrg2_adapt_laser_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(abi.ScanAdaptorParams),
                                                C.POINTER(abi.AdaptResult)]
        # srrg2_adapt_lidar_sweep (adaptors.MeasurementAdaptorLidarSweep), srrg2_spherical_model_full_turn
        _LIB.srrg2_adapt_default_lidar_params.argtypes = [C.POINTER(abi.LidarAdaptorParams)]
        _LIB.srrg2_adapt_default_lidar_params.restype = None
        _LIB.srrg2_spherical_model_full_turn.argtypes = [C.POINTER(abi.SphericalModel), C.c_int, C.c_int, C.c_double, C.c_double]
        _LIB.srrg2_adapt_lidar_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.POINTER(abi.LidarAdaptorParams), C.POINTER(abi.AdaptResult)]
        _LIB.srrg2_adapt_default_lidar_sweep_extras.argtypes = [C.POINTER(abi.LidarSweepExtras)]
        _LIB.srrg2_adapt_default_lidar_sweep_extras.restype = None
        _LIB.srrg2_adapt_lidar_sweep_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(abi.LidarAdaptorParams), C.POINTER(abi.LidarSweepExtras),
                                                    C.POINTER(abi.AdaptResult)]
        # srrg2_adapt_image_features (adaptors.MeasurementAdaptorImageFeatures), srrg2_feature_pattern
        _LIB.srrg2_adapt_default_feature_params.argtypes = [C.POINTER(abi.FeatureParams)]
        _LIB.srrg2_adapt_default_feature_params.restype = None
        _LIB.srrg2_adapt_image_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.FeatureParams),
                                                    C.POINTER(abi.Keypoint), C.c_int, C.POINTER(abi.FeatureResult)]
        _LIB.srrg2_feature_pattern.argtypes = [C.c_int, C.POINTER(C.c_int8)]
        # srrg2_adapt_image_features_pyramid (adaptors.MeasurementAdaptorImageFeaturesPyramid)
        _LIB.srrg2_adapt_default_pyramid_params.argtypes = [C.POINTER(abi.PyramidParams)]
        _LIB.srrg2_adapt_default_pyramid_params.restype = None
        _LIB.srrg2_adapt_image_features_pyramid.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                            C.c_int, C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.FeatureParams),
                                                            C.POINTER(abi.PyramidParams), C.POINTER(abi.PyramidKeypoint), C.c_int,
                                                            C.POINTER(abi.PyramidResult)]
        # srrg2_adapt_stereo_features (adaptors.MeasurementAdaptorStereoFeatures)
        _LIB.srrg2_adapt_default_stereo_params.argtypes = [C.POINTER(abi.StereoParams)]
        _LIB.srrg2_adapt_default_stereo_params.restype = None
        _LIB.srrg2_adapt_stereo_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                     C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.FeatureParams),
                                                     C.POINTER(abi.StereoParams), C.POINTER(abi.Keypoint), C.c_int,
                                                     C.POINTER(abi.StereoMatch), C.c_int, C.POINTER(abi.StereoResult)]
        # srrg2_adapt_stereo_dense (adaptors.MeasurementAdaptorStereoDense)
        _LIB.srrg2_adapt_default_dense_stereo_params.argtypes = [C.POINTER(abi.DenseStereoParams)]
        _LIB.srrg2_adapt_default_dense_stereo_params.restype = None
        _LIB.srrg2_adapt_stereo_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                  C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.DenseStereoParams), C.c_void_p,
                                                  C.c_int, C.POINTER(abi.DenseStereoResult)]
        # srrg2_rectifier_*, srrg2_rectify_*, srrg2_stereo_rectify (rectify.ImageRectifier / StereoRectifier)
        dp = C.POINTER(C.c_double)
        _LIB.srrg2_rectifier_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _LIB.srrg2_rectifier_destroy.argtypes = [C.c_void_p]
        _LIB.srrg2_rectifier_default_params.argtypes = [C.POINTER(abi.RectifierParams)]
        _LIB.srrg2_rectifier_default_params.restype = None
        _LIB.srrg2_rectifier_set.argtypes = [C.c_void_p, C.POINTER(abi.RectifierParams), C.POINTER(abi.RectifierInfo)]
        _LIB.srrg2_rectifier_get_map.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int64]
        _LIB.srrg2_rectifier_camera.argtypes = [C.c_void_p, C.POINTER(abi.DepthAdaptorParams)]
        _LIB.srrg2_rectify_image.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_int, C.c_int]
        _LIB.srrg2_rectify_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        _LIB.srrg2_stereo_rectify.argtypes = [dp, dp, dp, dp, dp, dp, dp, dp]
        # srrg2_gridmap_* (gridmap.OccupancyGrid)
        i32p = C.POINTER(C.c_int32)
        _LIB.srrg2_gridmap_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _LIB.srrg2_gridmap_destroy.argtypes = [C.c_void_p]
        _LIB.srrg2_gridmap_default_params.argtypes = [C.POINTER(abi.GridMapParams)]
        _LIB.srrg2_gridmap_default_params.restype = None
        _LIB.srrg2_gridmap_default_scan_params.argtypes = [C.POINTER(abi.GridMapScanParams)]
        _LIB.srrg2_gridmap_default_scan_params.restype = None
        _LIB.srrg2_gridmap_reset.argtypes = [C.c_void_p, C.POINTER(abi.GridMapParams)]
        _LIB.srrg2_gridmap_integrate_scans.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                       C.POINTER(abi.GridMapScanParams), C.c_int, C.POINTER(abi.GridMapResult)]
        _LIB.srrg2_gridmap_get_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _LIB.srrg2_gridmap_device_arrays.argtypes = [C.c_void_p, C.POINTER(i32p), C.POINTER(i32p)]
        _LIB.srrg2_gridmap_render.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        _LIB.srrg2_gridmap_to_scene.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _LIB.srrg2_gridmap_default_likelihood_lut.argtypes = [C.c_int, C.c_void_p]
        _LIB.srrg2_gridmap_build_likelihood.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _LIB.srrg2_gridmap_get_likelihood.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        _LIB.srrg2_gridmap_match_scans.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(abi.GridMapScanParams),
                                                   C.POINTER(abi.GridMapMatchParams), C.POINTER(abi.GridMapMatchResult), C.c_void_p,
                                                   C.c_int]
        _LIB.srrg2_gridmap_default_prune_params.argtypes = [C.POINTER(abi.GridMapPruneParams)]
        _LIB.srrg2_gridmap_default_prune_params.restype = None
        _LIB.srrg2_gridmap_build_bounds.argtypes = [C.c_void_p, C.c_int]
        _LIB.srrg2_gridmap_get_bounds.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
        _LIB.srrg2_gridmap_match_scans_pruned.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                          C.POINTER(abi.GridMapScanParams), C.POINTER(abi.GridMapMatchParams),
                                                          C.POINTER(abi.GridMapPruneParams), C.POINTER(abi.GridMapMatchResult),
                                                          C.POINTER(abi.GridMapPruneStats)]
        # srrg2_tsdf_* (tsdf.TsdfVolume)
        _LIB.srrg2_tsdf_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        _LIB.srrg2_tsdf_destroy.argtypes = [C.c_void_p]
        _LIB.srrg2_tsdf_default_params.argtypes = [C.POINTER(abi.TsdfParams)]
        _LIB.srrg2_tsdf_default_params.restype = None
        _LIB.srrg2_tsdf_default_frame_params.argtypes = [C.POINTER(abi.TsdfFrameParams)]
        _LIB.srrg2_tsdf_default_frame_params.restype = None
        _LIB.srrg2_tsdf_default_raycast_params.argtypes = [C.POINTER(abi.TsdfRaycastParams)]
        _LIB.srrg2_tsdf_default_raycast_params.restype = None
        _LIB.srrg2_tsdf_reset.argtypes = [C.c_void_p, C.POINTER(abi.TsdfParams)]
        _LIB.srrg2_tsdf_integrate_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_int, C.POINTER(abi.DepthAdaptorParams),
                                                     C.POINTER(abi.TsdfFrameParams), C.c_int, C.POINTER(abi.TsdfResult)]
        _LIB.srrg2_tsdf_raycast.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.DepthAdaptorParams), C.POINTER(abi.TsdfRaycastParams),
                                            C.c_void_p, C.c_void_p, C.c_int, C.POINTER(abi.TsdfRaycastResult)]
        _LIB.srrg2_tsdf_to_scene.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(abi.TsdfExportResult)]
        _LIB.srrg2_tsdf_get_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _LIB.srrg2_tsdf_device_arrays.argtypes = [C.c_void_p, C.POINTER(i32p), C.POINTER(i32p), C.POINTER(i32p)]
        # srrg2_scene_track_features (mapping.FeatureTracker)
        _LIB.srrg2_track_default_params.argtypes = [C.POINTER(abi.TrackParams)]
        _LIB.srrg2_track_default_params.restype = None
        _LIB.srrg2_scene_track_features.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(abi.TrackParams),
                                                    C.c_void_p, C.c_int, C.POINTER(abi.TrackResult)]
        # srrg2_consensus_* (consensus.ConsensusVerifier)
        _LIB.srrg2_consensus_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        _LIB.srrg2_consensus_destroy.argtypes = [C.c_void_p]
        _LIB.srrg2_consensus_default_params.argtypes = [C.POINTER(abi.ConsensusParams)]
        _LIB.srrg2_consensus_default_params.restype = None
        _LIB.srrg2_consensus_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                 C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                                 C.POINTER(abi.ConsensusParams), C.c_void_p, C.c_void_p, C.c_int64,
                                                 C.POINTER(C.c_int64)]
        # srrg2_scene_clip_projective (mapping.SceneClipperProjective)
        from . import mapping

        _LIB.srrg2_clip_default_projective_params.argtypes = [C.POINTER(mapping.ProjectiveClipParams)]
        _LIB.srrg2_clip_default_projective_params.restype = None
        _LIB.srrg2_scene_clip_projective.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(mapping.ProjectiveClipParams),
                                                     C.c_void_p, C.POINTER(mapping.ClipResult)]
        # srrg2_scene_clip_scan (mapping.SceneClipperScan)
        _LIB.srrg2_clip_default_scan_params.argtypes = [C.POINTER(mapping.ScanClipParams)]
        _LIB.srrg2_clip_default_scan_params.restype = None
        _LIB.srrg2_scene_clip_scan.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(mapping.ScanClipParams), C.c_void_p,
                                               C.POINTER(mapping.ClipResult)]
        # srrg2_scene_clip_spherical (mapping.SceneClipperSpherical)
        _LIB.srrg2_clip_default_spherical_params.argtypes = [C.POINTER(abi.SphericalClipParams)]
        _LIB.srrg2_clip_default_spherical_params.restype = None
        _LIB.srrg2_scene_clip_spherical.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(abi.SphericalClipParams),
                                                    C.c_void_p, C.POINTER(mapping.ClipResult)]
        _LIB.srrg2_scene_clip_spherical_rings.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(abi.SphericalClipParams),
                                                          C.POINTER(C.c_double), C.c_void_p, C.POINTER(mapping.ClipResult)]
        # srrg2_scene_estimate_normals (mapping.Scene.estimate_normals)
        _LIB.srrg2_normals_default_params.argtypes = [C.POINTER(abi.NormalsParams), C.c_int]
        _LIB.srrg2_normals_default_params.restype = None
        _LIB.srrg2_normals_exponents.argtypes = [C.c_float, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _LIB.srrg2_normals_exponents.restype = None
        _LIB.srrg2_scene_estimate_normals.argtypes = [C.c_void_p, C.POINTER(abi.NormalsParams), C.POINTER(C.c_float),
                                                      C.POINTER(abi.NormalsResult)]
        # srrg2_scene_voxelize (mapping.Scene.voxelize)
        _LIB.srrg2_voxel_default_params.argtypes = [C.POINTER(abi.VoxelParams)]
        _LIB.srrg2_voxel_default_params.restype = None
        _LIB.srrg2_scene_voxelize.argtypes = [C.c_void_p, C.POINTER(abi.VoxelParams), C.c_void_p, C.POINTER(C.c_int32),
                                              C.POINTER(abi.VoxelResult)]
    return _LIB


def backend():
    l = lib()
    return Backend(l, "srrg2_aligner_", l.srrg2_amd_last_error, needs_device=True)


def device_count():
    return lib().srrg2_amd_device_count()
