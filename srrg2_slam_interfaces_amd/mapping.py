"""Python mirror of the tracker-side scene steps over the C ABI (srrg2_scene_*).

``Scene``                      a point(+normal) cloud kept in device memory (a LocalMap scene slice / a measurement); with
                               ``set_features`` also a 256-bit descriptor and an intensity per point (PointIntensityDescriptor2f / 3f
                               clouds), which clipper and merger move with the points
``SceneClipperBall``           ``SceneClipper_`` (S/mapping/scene_clipper.h:17-122) with the ball policy
``SceneClipperProjective``     the same interface with the projective policy: what a pinhole camera sees (3-D, product library)
``SceneClipperScan``           the same interface with the scan policy: what a planar laser scanner sees (2-D, product library)
``SceneClipperSpherical``      the same interface with the spherical policy: what a spinning 3-D lidar sees (3-D, product library)
``FeatureTracker``             a concrete ``CorrespondenceFinder_``: keypoints of the measurement against the landmarks of the clipped
                               map by projective window and descriptor distance (3-D, product library); ``to_merger`` flips its pairs
``MergerCorrespondenceHomo``   ``MergerCorrespondenceHomo_`` (S/mapping/merger_correspondence_homo_impl.cpp:11-125)

Method names follow the reference setters (snake_case).  Thin marshalling only; parametrised by
(lib, prefix, err_fn) like ``posegraph.PoseGraph`` so that the test-side oracle binding reuses it.
"""
import ctypes as C

import numpy as np

from . import _abi as abi

MERGER_ERROR, MERGER_INITIALIZING, MERGER_SUCCESS = 0, 1, 2
CLIPPER_ERROR, CLIPPER_SUCCESSFUL, CLIPPER_READY = 0, 1, 2


class MergerParams(C.Structure):
    _fields_ = [("maximum_response", C.c_float), ("maximum_distance_geometry_squared", C.c_float),
                ("target_number_of_merges", C.c_int32)]


class MergeResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("num_correspondences", C.c_int32), ("num_merged", C.c_int32),
                ("num_added", C.c_int32), ("scene_size", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ProjectiveClipParams(C.Structure):
    """srrg2_projective_clip_params"""
    _fields_ = [("camera_matrix", C.c_float * 9), ("image_rows", C.c_int32), ("image_cols", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float), ("sensor_in_robot", C.c_float * 12),
                ("occlusion_margin", C.c_float)]


class ScanClipParams(C.Structure):
    """srrg2_scan_clip_params"""
    _fields_ = [("angle_min", C.c_double), ("angle_increment", C.c_double), ("num_beams", C.c_int32), ("range_min", C.c_float),
                ("range_max", C.c_float), ("sensor_in_robot", C.c_float * 9), ("occlusion_margin", C.c_float)]


class ClipResult(C.Structure):
    """srrg2_clip_result"""
    _fields_ = [("status", C.c_int32), ("num_valid", C.c_int32), ("num_in_view", C.c_int32), ("num_kept", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def default_projective_clip_params():
    """identity sensor, depth 0.4 .. 8 m, occlusion_margin < 0 (frustum only); camera matrix / rows / cols are the caller's"""
    from . import _capi

    p = ProjectiveClipParams()
    _capi.lib().srrg2_clip_default_projective_params(C.byref(p))
    return p


def default_scan_clip_params():
    """identity sensor, range 0.05 .. 30 m, occlusion_margin < 0 (sector only); angle_min / angle_increment / num_beams are the
    caller's"""
    from . import _capi

    p = ScanClipParams()
    _capi.lib().srrg2_clip_default_scan_params(C.byref(p))
    return p


SphericalModel, SphericalClipParams = abi.SphericalModel, abi.SphericalClipParams


def default_spherical_clip_params():
    """identity sensor, range 0.5 .. 120 m, occlusion_margin < 0 (field of view only); the model's angles / rows / cols are the
    caller's (``adaptors.spherical_model_full_turn(rows, cols, first, last, model=p.model)`` fills a full turn)"""
    from . import _capi

    p = SphericalClipParams()
    _capi.lib().srrg2_clip_default_spherical_params(C.byref(p))
    return p


VoxelParams, VoxelResult = abi.VoxelParams, abi.VoxelResult
VOXEL_MODES = {"centroid": abi.VOXEL_CENTROID, "first": abi.VOXEL_FIRST}


def default_voxel_params():
    """leaf 0.05 m, origin 0 (the grid is anchored to the frame), centroid mode, min_points_per_voxel 1"""
    from . import _capi

    p = VoxelParams()
    _capi.lib().srrg2_voxel_default_params(C.byref(p))
    return p


def default_merger_params():
    """merger.h:126-131, merger_correspondence_homo.h:22-31"""
    return MergerParams(50.0, 0.25, 200)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class _Binding:
    def __init__(self, lib, prefix, err_fn, device):
        self.lib, self.prefix, self.err, self.device = lib, prefix, err_fn, device

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def check(self, rc):
        if rc != 0:
            msg = self.err()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))


def as_scene_features(descriptors, intensity, n):
    """argument checking of Scene.set_features: (descriptors as (n, 32) uint8 or None, intensity as (n,) float32 or None)"""
    d = i = None
    if descriptors is not None:
        from .descriptors import as_descriptors

        d = as_descriptors(descriptors)
        if d.shape[0] != n:
            raise ValueError("descriptors: %d rows for a scene of %d points" % (d.shape[0], n))
    if intensity is not None:
        i = np.asarray(intensity)
        if i.dtype.kind not in "fiub":
            raise ValueError("intensity: numbers expected, got %s" % i.dtype)
        if i.shape not in ((n,), (n, 1)):
            raise ValueError("intensity: expected %d values, got shape %s" % (n, i.shape))
        i = np.ascontiguousarray(i, dtype=np.float32).reshape(n)
    return d, i


class Scene:
    def __init__(self, binding, dim=3):
        self._b = binding
        self.dim = dim
        self._h = C.c_void_p()
        if binding.device is None:
            rc = binding.fn("create")(C.c_int(dim), C.byref(self._h))
        else:
            rc = binding.fn("create")(C.c_int(dim), C.c_int(binding.device), C.byref(self._h))
        binding.check(rc)

    def close(self):
        if self._h:
            self._b.fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, coords, normals=None):
        c = _f32(coords).reshape(-1, self.dim)
        n = None if normals is None else _f32(normals).reshape(-1, self.dim)
        args = [self._h, _fp(c), C.c_int(4 * self.dim), _fp(n) if n is not None else None, C.c_int(4 * self.dim),
                C.c_int(c.shape[0])]
        if self._b.device is not None:
            args.append(C.c_int(abi.MEM_HOST))
        self._b.check(self._b.fn("set")(*args))

    def size(self):
        n = C.c_int(0)
        self._b.check(self._b.fn("size")(self._h, C.byref(n)))
        return n.value

    def get(self):
        """(coords, normals) as (n, dim) float32 arrays."""
        n = self.size()
        c = np.zeros((max(n, 1), self.dim), np.float32)
        m = np.zeros((max(n, 1), self.dim), np.float32)
        k = C.c_int(0)
        self._b.check(self._b.fn("get")(self._h, _fp(c), _fp(m), C.c_int(n), C.byref(k)))
        return c[:n], m[:n]

    def _feature_fn(self, name):
        """the feature entry points exist in the HIP library only"""
        f = getattr(self._b.lib, self._b.prefix + name, None)
        if f is None:
            raise NotImplementedError("%s%s: this binding has no per-point features (product library only)"
                                      % (self._b.prefix, name))
        return f

    def set_features(self, descriptors=None, intensity=None):
        """one 256-bit descriptor ((n, 32) uint8 rows) and / or one intensity per point; None = that field is absent
        (both None drops the features).  They follow the points through clip and merge."""
        d, i = as_scene_features(descriptors, intensity, self.size())
        f = self._feature_fn("set_features")
        n = self.size()
        self._b.check(f(self._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(32),
                        None if i is None else _fp(i), C.c_int(4), C.c_int(n), C.c_int(abi.MEM_HOST)))

    def has_features(self):
        """(has descriptors, has intensity)"""
        d, i = C.c_int(0), C.c_int(0)
        self._b.check(self._feature_fn("has_features")(self._h, C.byref(d), C.byref(i)))
        return bool(d.value), bool(i.value)

    def features(self):
        """(descriptors as (n, 32) uint8 or None, intensity as (n,) float32 or None)"""
        hd, hi = self.has_features()
        n = self.size()
        d = np.zeros((max(n, 1), 32), np.uint8) if hd else None
        i = np.zeros(max(n, 1), np.float32) if hi else None
        k = C.c_int(0)
        self._b.check(self._feature_fn("get_features")(
            self._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint8)), None if i is None else _fp(i),
            C.c_int(n), C.byref(k)))
        return (None if d is None else d[:n]), (None if i is None else i[:n])

    def device_features(self):
        """(descriptors_ptr or None, intensity_ptr or None, n): device arrays, rows of 32 bytes / floats; valid until the
        scene is next modified"""
        d, i, n = C.POINTER(C.c_uint8)(), C.POINTER(C.c_float)(), C.c_int(0)
        self._b.check(self._feature_fn("device_features")(self._h, C.byref(d), C.byref(i), C.byref(n)))
        return (d if d else None), (i if i else None), n.value

    def global_indices(self):
        n = C.c_int(0)
        self._b.check(self._b.fn("global_indices")(self._h, None, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.int32)
        k = C.c_int(n.value)
        self._b.check(self._b.fn("global_indices")(self._h, buf.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)))
        return buf[:n.value]

    def estimate_normals(self, radius, min_neighbours=None, max_curvature=1.0, viewpoint=(0.0, 0.0, 0.0), drop=True,
                         return_curvature=False, want_result=True):
        """normals from the PCA of every point's radius neighbourhood, on the device (srrg2_scene_estimate_normals; product
        library only).  ``viewpoint`` None: no viewpoint (the largest component of a normal is made positive).  ``drop``:
        points that get no normal leave the scene.  Returns the counts as a dict -- with ``return_curvature`` the pair
        (counts, curvature per point as indexed BEFORE the call).  ``want_result=False`` with ``drop=False`` and no curvature
        queues the work and returns None without waiting."""
        f = self._feature_fn("estimate_normals")
        p = abi.NormalsParams()
        self._b.lib.srrg2_normals_default_params(C.byref(p), C.c_int(self.dim))
        p.radius = float(radius)
        if min_neighbours is not None:
            p.min_neighbours = int(min_neighbours)
        p.max_curvature = float(max_curvature)
        vp = (np.nan,) * 3 if viewpoint is None else tuple(float(v) for v in viewpoint) + (0.0,) * (3 - len(viewpoint))
        for k in range(3):
            p.viewpoint[k] = vp[k]
        p.drop_points_without_normal = int(drop)
        out = abi.NormalsResult()
        curv = np.zeros(max(self.size(), 1), np.float32) if return_curvature else None
        n = self.size()
        self._b.check(f(self._h, C.byref(p), _fp(curv) if return_curvature else None, C.byref(out) if want_result else None))
        res = out.as_dict() if want_result else None
        return (res, curv[:n]) if return_curvature else res

    def voxelize(self, dst, leaf_size, origin=(0.0, 0.0, 0.0), mode="centroid", min_points=1, return_counts=False,
                 want_result=True):
        """voxel-grid decimation into the scene ``dst`` (srrg2_scene_voxelize; product library only): one point per occupied
        cell of ``leaf_size``, in the order of each cell's first point; this scene is left untouched and
        ``dst.global_indices()`` names every emitted point's representative here.  ``mode``: "centroid" (the cell's mean point
        and mean normal, the representative's descriptor and intensity) or "first" (the representative verbatim).  Returns the
        counts as a dict (None without ``want_result``) -- with ``return_counts`` the pair (counts, points per emitted cell)."""
        f = self._feature_fn("voxelize")
        p = VoxelParams()
        self._b.lib.srrg2_voxel_default_params(C.byref(p))
        p.leaf_size = float(leaf_size)
        o = tuple(float(v) for v in origin) + (0.0,) * (3 - len(origin))
        for k in range(3):
            p.origin[k] = o[k]
        if mode not in VOXEL_MODES:
            raise ValueError("voxelize: mode is 'centroid' or 'first', got %r" % (mode,))
        p.mode = VOXEL_MODES[mode]
        p.min_points_per_voxel = int(min_points)
        out = VoxelResult()
        counts = np.zeros(max(self.size(), 1), np.int32) if return_counts else None
        self._b.check(f(self._h, C.byref(p), dst._h, counts.ctypes.data_as(C.POINTER(C.c_int32)) if return_counts else None,
                        C.byref(out) if want_result else None))
        res = out.as_dict() if want_result else None
        return (res, counts[:dst.size()]) if return_counts else res

    def device_arrays(self):
        """(coords_ptr, normals_ptr or None, n): device float4 arrays (product backend only)."""
        c, m, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int(0)
        self._b.check(self._b.fn("device_arrays")(self._h, C.byref(c), C.byref(m), C.byref(n)))
        return c, (m if m else None), n.value


class _ClipperBase:
    """what the four clippers share: the full scene, the clipped scene, the pose, status() and global_indices()."""

    def __init__(self, binding):
        self._b = binding
        self._full = self._clipped = None
        self._robot_in_local_map = None
        self._status = CLIPPER_ERROR

    def set_full_scene(self, scene):
        self._full = scene

    def set_clipped_scene_in_robot(self, scene):
        self._clipped = scene

    def set_robot_in_local_map(self, T):
        self._robot_in_local_map = _f32(T)

    def _ready(self):
        if self._full is None or self._clipped is None or self._robot_in_local_map is None:
            raise RuntimeError("%s::compute|scene, output or pose not set" % type(self).__name__)

    def status(self):
        return self._status

    def global_indices(self):
        return self._clipped.global_indices()


class SceneClipperBall(_ClipperBase):
    """setFullScene / setClippedSceneInRobot / setRobotInLocalMap / compute / status / globalIndices."""

    def __init__(self, binding, range_max=10.0):
        super().__init__(binding)
        self.range_max = float(range_max)

    def compute(self):
        self._ready()
        st = C.c_int(0)
        self._b.check(self._b.fn("clip_ball")(self._full._h, _fp(self._robot_in_local_map), C.c_float(self.range_max),
                                              self._clipped._h, C.byref(st)))
        self._status = st.value


class _ViewClipperBase(_ClipperBase):
    """the clippers with a sensor: ``params`` (its sensor_in_robot has ``_SENSOR_FLOATS`` floats), ``last`` and the frame of
    compute(); a subclass makes the call in ``_clip(out)``, ``out`` being the result struct by reference or None."""

    def __init__(self, binding, params):
        super().__init__(binding)
        self.params = params
        self.last = None

    def set_sensor_in_robot(self, T):
        for i, v in enumerate(_f32(T).reshape(self._SENSOR_FLOATS)):
            self.params.sensor_in_robot[i] = float(v)

    def compute(self, want_result=True):
        self._ready()
        out = ClipResult()
        self._status = CLIPPER_ERROR
        self._b.check(self._clip(C.byref(out) if want_result else None))
        if want_result:
            self._status, self.last = out.status, out.as_dict()
        else:
            self._status, self.last = (CLIPPER_SUCCESSFUL if self._full.size() else CLIPPER_READY), None
        return self.last


class SceneClipperProjective(_ViewClipperBase):
    """setFullScene / setClippedSceneInRobot / setRobotInLocalMap / setSensorInRobot / setCameraMatrix / compute / status /
    globalIndices.  ``params``: ProjectiveClipParams (image size, depth range, occlusion_margin); ``last``: the counts of the
    last compute() (``want_result=False`` passes no result struct: ``last`` is then None)."""
    _SENSOR_FLOATS = 12

    def __init__(self, binding, params=None):
        super().__init__(binding, params or default_projective_clip_params())

    def set_camera_matrix(self, K):
        for i, v in enumerate(_f32(K).reshape(9)):
            self.params.camera_matrix[i] = float(v)

    def _clip(self, out):
        return self._b.fn("clip_projective")(self._full._h, _fp(self._robot_in_local_map), C.byref(self.params), self._clipped._h, out)


class SceneClipperScan(_ViewClipperBase):
    """setFullScene / setClippedSceneInRobot / setRobotInLocalMap / setSensorInRobot / compute / status / globalIndices for 2-D
    scenes.  ``params``: ScanClipParams (angle_min, angle_increment, num_beams, range interval, occlusion_margin); ``last``: the
    counts of the last compute() (``want_result=False`` passes no result struct: ``last`` is then None)."""
    _SENSOR_FLOATS = 9

    def __init__(self, binding, params=None):
        super().__init__(binding, params or default_scan_clip_params())

    def _clip(self, out):
        return self._b.fn("clip_scan")(self._full._h, _fp(self._robot_in_local_map), C.byref(self.params), self._clipped._h, out)


class SceneClipperSpherical(_ViewClipperBase):
    """setFullScene / setClippedSceneInRobot / setRobotInLocalMap / setSensorInRobot / compute / status / globalIndices for 3-D
    scenes seen by a spinning lidar.  ``params``: SphericalClipParams (model, occlusion_margin); ``last``: the counts of the last
    compute() (``want_result=False`` passes no result struct: ``last`` is then None)."""
    _SENSOR_FLOATS = 12

    def __init__(self, binding, params=None):
        super().__init__(binding, params or default_spherical_clip_params())
        self._rings = None

    def set_model(self, model):
        C.memmove(C.byref(self.params.model), C.byref(model), C.sizeof(SphericalModel))

    def set_ring_elevations(self, elevations):
        """one elevation (radians) per row of the model, strictly ascending or descending, for sensors whose rings are not
        uniformly spaced (the model's elevation_min / elevation_increment are then ignored); None: the model's uniform rows.
        A copy is kept; its length must be ``params.model.rows`` at compute()."""
        self._rings = None if elevations is None else np.array(elevations, dtype=np.float64).reshape(-1)

    def _clip(self, out):
        if self._rings is None:
            return self._b.fn("clip_spherical")(self._full._h, _fp(self._robot_in_local_map), C.byref(self.params), self._clipped._h,
                                                out)
        if self._rings.shape[0] != self.params.model.rows:
            raise ValueError("ring elevations: %d entries for %d rows" % (self._rings.shape[0], self.params.model.rows))
        return self._b.fn("clip_spherical_rings")(self._full._h, _fp(self._robot_in_local_map), C.byref(self.params),
                                                  self._rings.ctypes.data_as(C.POINTER(C.c_double)), self._clipped._h, out)


TrackParams, TrackResult = abi.TrackParams, abi.TrackResult
CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])


def default_track_params():
    """depth 0.4 .. 8 m, search_radius 16, max_distance 48, min_margin 0 (off), cross_check 1; camera matrix / rows / cols are
    the caller's"""
    from . import _capi

    p = TrackParams()
    _capi.lib().srrg2_track_default_params(C.byref(p))
    return p


def to_merger(corr, moving_global_indices):
    """a FeatureTracker result (fixed_idx = measurement point, moving_idx = point of the clipped map) flipped and globalised on
    the host, as TrackerSliceProcessor_::merge() does (tracker_slice_processor_impl.cpp:160-186): fixed_idx = map point
    (``moving_global_indices`` = the clipped scene's global_indices()), moving_idx = measurement point, response kept.  What
    ``MergerCorrespondenceHomo.set_correspondences`` takes."""
    g = np.asarray(moving_global_indices, np.int32).reshape(-1)
    out = np.zeros(len(corr), CORR_DTYPE)
    out["fixed_idx"] = g[np.asarray(corr["moving_idx"], np.int64)]
    out["moving_idx"] = corr["fixed_idx"]
    out["response"] = corr["response"]
    return out


class FeatureTracker:
    """setFixed / setMoving / setLocalMapInSensor / compute of the reference's CorrespondenceFinder_
    (S/registration/correspondence_finder.h:56-114), made concrete for clouds with descriptors (srrg2_scene_track_features;
    product library only).  ``fixed``: the measurement, a scene of keypoints whose global indices are pixel indices (an image,
    stereo or pyramid adaptor's output); ``moving``: the clipped local map, landmarks with descriptors; ``moving_in_sensor``: the pose
    guess (3 x 4).  ``params``: TrackParams (camera matrix, image size, depth range, search_radius, max_distance, min_margin,
    cross_check).  compute() returns the pairs as a CORR_DTYPE array in ascending moving_idx -- what
    ``MultiAligner.set_correspondences`` takes for a FINDER_CORRESPONDENCES slice; ``result``: the counters of the last call."""

    def __init__(self, binding, params=None):
        self._b = binding
        self.params = params or default_track_params()
        self._fixed = self._moving = None
        self._T = _f32(np.eye(3, 4))
        self.result = None

    def set_camera_matrix(self, K):
        for i, v in enumerate(_f32(K).reshape(9)):
            self.params.camera_matrix[i] = float(v)

    def set_fixed(self, scene):
        self._fixed = scene

    def set_moving(self, scene):
        self._moving = scene

    def set_moving_in_sensor(self, T):
        self._T = _f32(T).reshape(12)

    def compute(self, capacity=None, want_result=True):
        """``capacity``: at most that many pairs are returned (``result["num_correspondences"]`` still counts all); None:
        room for every landmark.  ``want_result=False`` passes no result struct: ``result`` is then None and the array has
        ``capacity`` rows, of which the caller cannot tell how many are pairs."""
        if self._fixed is None or self._moving is None:
            raise RuntimeError("FeatureTracker::compute|fixed or moving not set")
        f = getattr(self._b.lib, self._b.prefix + "track_features", None)
        if f is None:
            raise NotImplementedError("%strack_features: this binding has no feature tracker (product library only)" % self._b.prefix)
        cap = self._moving.size() if capacity is None else int(capacity)
        buf = np.zeros(max(cap, 1), CORR_DTYPE)
        out = TrackResult()
        self.result = None
        self._b.check(f(self._moving._h, self._fixed._h, _fp(self._T), C.byref(self.params), C.c_void_p(buf.ctypes.data) if cap > 0 else None,
                        C.c_int(cap), C.byref(out) if want_result else None))
        if not want_result:
            return buf[:max(cap, 0)]
        self.result = out.as_dict()
        return buf[:min(max(cap, 0), out.num_correspondences)]


class MergerCorrespondenceHomo:
    """setScene / setMeasurement / setMeasurementInScene / setCorrespondences / compute / status."""

    def __init__(self, binding, params=None):
        self._b = binding
        self.params = params or default_merger_params()
        self._scene = self._meas = None
        self._T = None
        self._corr = None  # None = "no correspondences set" (merger_correspondence_homo_impl.cpp:30)
        self._status = MERGER_ERROR
        self.last = None

    def set_scene(self, scene):
        self._scene = scene

    def set_measurement(self, scene):
        self._meas = scene

    def set_measurement_in_scene(self, T):
        self._T = _f32(T)

    def set_correspondences(self, corr):
        """structured array with fixed_idx (scene), moving_idx (measurement), response -- or None."""
        self._corr = corr

    def _ready(self):
        if self._scene is None or self._meas is None or self._T is None:
            raise RuntimeError("MergerCorrespondenceHomo::compute|scene, measurement or transform not set")

    def compute(self):
        self._ready()
        out = MergeResult()
        if self._corr is None:
            cptr, n = None, -1
        else:
            arr = (abi.Correspondence * max(len(self._corr), 1))()
            for k, c in enumerate(self._corr):
                arr[k].fixed_idx, arr[k].moving_idx, arr[k].response = int(c["fixed_idx"]), int(c["moving_idx"]), float(c["response"])
            cptr, n = arr, len(self._corr)
        self._b.check(self._b.fn("merge")(self._scene._h, self._meas._h, _fp(self._T), cptr, C.c_int(n),
                                          C.byref(self.params), C.byref(out)))
        self._status, self.last = out.status, out.as_dict()
        return self.last

    def compute_from_aligner(self, aligner, slice_idx, clipped):
        """correspondences taken on the device from an aligner whose moving cloud was ``clipped`` and whose fixed
        cloud was the measurement (TrackerSliceProcessor_::merge(), tracker_slice_processor_impl.cpp:160-186)."""
        self._ready()
        out = MergeResult()
        self._b.check(self._b.fn("merge_from_aligner")(self._scene._h, self._meas._h, _fp(self._T), aligner._h,
                                                       C.c_int(slice_idx), clipped._h, C.byref(self.params), C.byref(out)))
        self._status, self.last = out.status, out.as_dict()
        return self.last

    def status(self):
        return self._status
