"""MI355X-native multi-cue aligner hot path of srrg2_slam_interfaces."""
from . import _abi as abi  # noqa: F401


def MultiAligner(variable_kind=abi.SE3_QUAT_RIGHT, device=0):
    """Product aligner on the HIP library (raises if the library or a HIP device is missing)."""
    from . import _capi
    from .aligner import MultiAligner as _MA

    return _MA(_capi.backend(), variable_kind, device)


def PoseGraph(variable_kind=abi.SE3_QUAT_RIGHT, device=0):
    """Product pose-graph solver on the HIP library (raises if the library or a HIP device is missing)."""
    from . import _capi
    from .posegraph import PoseGraph as _PG

    l = _capi.lib()
    return _PG(l, "srrg2_posegraph_", l.srrg2_amd_last_error, variable_kind, device=device)


def scene_binding(device=0):
    """Binding of the scene/clipper/merger classes of ``mapping`` to the HIP library."""
    from . import _capi
    from .mapping import _Binding

    l = _capi.lib()
    return _Binding(l, "srrg2_scene_", l.srrg2_amd_last_error, device)


def FeatureTracker(params=None, device=0):
    """Per-frame data association of a visual tracker on the HIP library: keypoints of the measurement against the landmarks of
    the clipped local map, by projective window and descriptor distance; see ``mapping.FeatureTracker``."""
    from .mapping import FeatureTracker as _FT

    return _FT(scene_binding(device), params)


def DescriptorDatabase(device=0):
    """Device-resident database of 256-bit binary descriptors with exact matching (the matching half of the HBST loop
    detector; raises if the library or a HIP device is missing)."""
    from .descriptors import DescriptorDatabase as _DD

    return _DD(device=device)


def ConsensusVerifier(dim=3, device=0):
    """Geometric verification of descriptor matches on the HIP library: a consensus pose and its inlier matches per candidate
    (batched RANSAC with a fixed hypothesis count); see ``consensus.ConsensusVerifier``."""
    from .consensus import ConsensusVerifier as _CV

    return _CV(dim, device)


def MeasurementAdaptorDepthImage(params=None):
    """Depth image -> measurement scene on the device (the adapt step of a tracker's frame); see ``adaptors``."""
    from .adaptors import MeasurementAdaptorDepthImage as _A

    return _A(params)


def MeasurementAdaptorLaserScan(params=None):
    """Laser scan -> measurement scene on the device; see ``adaptors``."""
    from .adaptors import MeasurementAdaptorLaserScan as _A

    return _A(params)


def MeasurementAdaptorLidarSweep(params=None):
    """3-D lidar sweep (point list) -> measurement scene with normals on the device; see ``adaptors``."""
    from .adaptors import MeasurementAdaptorLidarSweep as _A

    return _A(params)


def MeasurementAdaptorImageFeatures(params=None, camera=None):
    """8-bit intensity image (+ optional depth image) -> scene of keypoints with descriptors on the device; see ``adaptors``."""
    from .adaptors import MeasurementAdaptorImageFeatures as _A

    return _A(params, camera)


def MeasurementAdaptorImageFeaturesPyramid(params=None, camera=None, pyramid=None):
    """MeasurementAdaptorImageFeatures on every level of a scale pyramid, into one scene; see ``adaptors``."""
    from .adaptors import MeasurementAdaptorImageFeaturesPyramid as _A

    return _A(params, camera, pyramid)


def MeasurementAdaptorStereoFeatures(params=None, stereo=None, camera=None):
    """Rectified pair of 8-bit images -> scene of matched, triangulated keypoints with descriptors on the device; see
    ``adaptors``."""
    from .adaptors import MeasurementAdaptorStereoFeatures as _A

    return _A(params, stereo, camera)


def MeasurementAdaptorStereoDense(stereo=None, camera=None):
    """Rectified pair of 8-bit images -> per-pixel disparity -> the depth adaptor's scene, on the device; see ``adaptors``."""
    from .adaptors import MeasurementAdaptorStereoDense as _A

    return _A(stereo, camera)


def ImageRectifier(device=0):
    """Lens undistortion / rectification of raw images on the device, the stage in front of the image adaptors; see ``rectify``."""
    from .rectify import ImageRectifier as _R

    return _R(device)


def OccupancyGrid(device=0):
    """Occupancy grid map from laser scans and poses on the device: integrate / remove scans, read the counts, render the
    image, export the occupied cells as a 2-D scene, match scans against its likelihood field over a window of poses; see
    ``gridmap``."""
    from .gridmap import OccupancyGrid as _G

    return _G(device)


def TsdfVolume(device=0):
    """Truncated signed-distance volume from depth frames and poses on the device: integrate / remove frames, raycast an
    organised scene with normals from a pose (frame-to-model tracking), export the surface as a 3-D scene; see ``tsdf``."""
    from .tsdf import TsdfVolume as _T

    return _T(device)


def StereoRectifier(device=0):
    """Two ``ImageRectifier``s set from a stereo calibration; both images of a pair rectified in one launch; see ``rectify``."""
    from .rectify import StereoRectifier as _R

    return _R(device)
