"""Python mirror of the measurement adaptors over the C ABI (srrg2_adapt_*): raw sensor data -> measurement scene, on the device.

``MeasurementAdaptorDepthImage``   depth image (uint16 counts or float32 metres, + optional intensity image) -> organised
                                   or compact 3-D scene with normals
``MeasurementAdaptorLaserScan``    ranges -> 2-D scene with normals
``MeasurementAdaptorLidarSweep``   3-D lidar sweep (a list of points, + optional intensity) -> organised or compact 3-D scene
                                   with normals, through the range image of a spherical sensor model
``MeasurementAdaptorImageFeatures`` 8-bit intensity image (+ optional depth image) -> compact 3-D scene of keypoints, each with
                                   a 256-bit descriptor and an intensity (FAST corners, rotated-pair descriptors)
``MeasurementAdaptorImageFeaturesPyramid`` the same on every level of a scale pyramid of the image -> ONE compact scene,
                                   level-major, points at the keypoints' level-0 positions
``MeasurementAdaptorStereoFeatures`` rectified pair of 8-bit images -> compact 3-D scene of the left image's keypoints that were
                                   matched in the right image, triangulated (z = fx * baseline / disparity)
``MeasurementAdaptorStereoDense``  rectified pair of 8-bit images -> a disparity per pixel (census cost, four-path semi-global
                                   aggregation) -> depth -> the scene of MeasurementAdaptorDepthImage, organised or compact

Method names follow ``RawDataPreprocessor_`` (S/raw_data_preprocessors/raw_data_preprocessor.h:13-88), snake_case:
``set_raw_data``, ``set_meas``, ``compute``, ``status``, ``reset``; ``status()`` is ERROR after ``set_raw_data`` until
``compute()`` (:67-72).  Thin marshalling only; product library only (the oracle has no adaptor: the parity target is
tests/adaptor_restatement.py, tests/lidar_restatement.py, tests/features_restatement.py, tests/pyramid_restatement.py, tests/stereo_restatement.py and tests/stereo_dense_restatement.py).
"""
import ctypes as C

import numpy as np

from . import _abi as abi

_IMAGE_TYPES = {np.dtype(np.uint8): abi.IMAGE_U8, np.dtype(np.uint16): abi.IMAGE_U16, np.dtype(np.float32): abi.IMAGE_F32}


def default_depth_params():
    from . import _capi

    p = abi.DepthAdaptorParams()
    _capi.lib().srrg2_adapt_default_depth_params(C.byref(p))
    return p


def default_scan_params():
    from . import _capi

    p = abi.ScanAdaptorParams()
    _capi.lib().srrg2_adapt_default_scan_params(C.byref(p))
    return p


def default_lidar_params():
    """model zeroed except range 0.5 .. 120 m (fill it with ``spherical_model_full_turn`` or field by field); gaps 1 / 1,
    normal_max_distance_squared 1.0, drop 1, organised"""
    from . import _capi

    p = abi.LidarAdaptorParams()
    _capi.lib().srrg2_adapt_default_lidar_params(C.byref(p))
    return p


def spherical_model_full_turn(rows, cols, elevation_first, elevation_last, model=None):
    """srrg2_spherical_model_full_turn: columns tiling [-pi, pi), rows from elevation_first to elevation_last, range
    0.5 .. 120 m; fills ``model`` (e.g. ``params.model``) in place when given.  Raises on rows < 2, cols < 1, bad elevations."""
    from . import _capi

    m = abi.SphericalModel() if model is None else model
    lib = _capi.lib()
    if lib.srrg2_spherical_model_full_turn(C.byref(m), int(rows), int(cols), float(elevation_first), float(elevation_last)) != 0:
        msg = lib.srrg2_amd_last_error()
        raise ValueError(msg.decode() if msg else "spherical_model_full_turn")
    return m


def _image(img, image_type, what):
    """numpy 2-D array -> (array kept alive, pointer, type, row stride, MEM_HOST, shape); (device_pointer, stride) -> the
    same with MEM_DEVICE and no shape (``image_type`` says what the pointer holds)"""
    if isinstance(img, tuple):
        ptr, stride = img
        if image_type is None:
            raise ValueError("%s: a (device_pointer, stride) pair needs its image type" % what)
        return None, C.c_void_p(int(ptr)), int(image_type), int(stride), abi.MEM_DEVICE, None
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype not in _IMAGE_TYPES:
        raise ValueError("%s: a 2-D uint8 / uint16 / float32 array expected, got %s %s" % (what, a.dtype, a.shape))
    if a.size and a.strides[1] != a.itemsize:
        a = np.ascontiguousarray(a)
    stride = a.strides[0] if a.shape[0] > 1 and a.size else a.shape[1] * a.itemsize
    return a, C.c_void_p(a.ctypes.data), _IMAGE_TYPES[a.dtype], int(stride), abi.MEM_HOST, a.shape


class _AdaptorBase:
    def __init__(self):
        from . import _capi

        self._lib = _capi.lib()
        self._meas = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None

    def _check(self, rc):
        if rc != 0:
            self._status = abi.ADAPTOR_ERROR
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    def set_meas(self, scene):
        """the scene that compute() fills (its content is replaced)"""
        self._meas = scene

    def status(self):
        return self._status

    def _ready(self):
        if self._meas is None or self._raw is None:
            raise RuntimeError("%s::compute|raw data or measurement not set" % type(self).__name__)

    def _finish(self, out, want_result):
        """status READY unless nothing came in; the counts only when they were asked for (asking waits for the device)"""
        if want_result:
            self._status, self.last = out.status, out.as_dict()
        else:
            self._status, self.last = abi.ADAPTOR_READY, None
        return self.last


class MeasurementAdaptorDepthImage(_AdaptorBase):
    """params: abi.DepthAdaptorParams (camera_matrix, gates, gaps, compact, ...); rows / cols are taken from a numpy image."""

    def __init__(self, params=None):
        super().__init__()
        self.params = params or default_depth_params()
        self._raw = self._inten = None

    def set_camera_matrix(self, K):
        for i, v in enumerate(np.asarray(K, np.float32).reshape(9)):
            self.params.camera_matrix[i] = float(v)

    def set_raw_data(self, depth, intensity=None, depth_type=None, intensity_type=None):
        """depth (and intensity): 2-D numpy arrays, or (device_pointer, row_stride_bytes) pairs with their abi.IMAGE_* type
        (then params.rows / cols say the size).  The arrays are read at compute()."""
        raw = _image(depth, depth_type, "depth")
        inten = None if intensity is None else _image(intensity, intensity_type, "intensity")
        if inten is not None and (inten[4] != raw[4] or (raw[5] is not None and inten[5] != raw[5])):
            raise ValueError("intensity: same memory space and shape as the depth image expected")
        self._raw, self._inten = raw, inten
        if raw[5] is not None:
            self.params.rows, self.params.cols = raw[5]
        self._status = abi.ADAPTOR_ERROR  # raw_data_preprocessor.h:67-72: not computed yet

    def reset(self):
        self._raw = self._inten = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None

    def compute(self, want_result=True):
        """fills the measurement scene; returns the counts (dict), or None with ``want_result=False`` -- an organised adapt
        then only queues its work"""
        self._ready()
        out = abi.AdaptResult()
        _, dptr, dtype, dstride, mem, _ = self._raw
        if self._inten is None:
            iptr, itype, istride = None, abi.IMAGE_NONE, 0
        else:
            _, iptr, itype, istride, _, _ = self._inten
        self._check(self._lib.srrg2_adapt_depth_image(self._meas._h, dptr, dtype, dstride, iptr, itype, istride, mem,
                                                      C.byref(self.params), C.byref(out) if want_result else None))
        return self._finish(out, want_result)


class MeasurementAdaptorLaserScan(_AdaptorBase):
    """params: abi.ScanAdaptorParams (angle_min, angle_increment, gates, half window, compact, ...)."""

    def __init__(self, params=None):
        super().__init__()
        self.params = params or default_scan_params()
        self._raw = None

    def set_raw_data(self, ranges):
        """ranges: 1-D array of float32 metres, or a (device_pointer, num_beams) pair"""
        if isinstance(ranges, tuple):
            self._raw = (None, C.c_void_p(int(ranges[0])), int(ranges[1]), abi.MEM_DEVICE)
        else:
            a = np.ascontiguousarray(ranges, dtype=np.float32).reshape(-1)
            self._raw = (a, C.c_void_p(a.ctypes.data), a.shape[0], abi.MEM_HOST)
        self._status = abi.ADAPTOR_ERROR

    def reset(self):
        self._raw = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None

    def compute(self, want_result=True):
        self._ready()
        out = abi.AdaptResult()
        _, ptr, n, mem = self._raw
        self._check(self._lib.srrg2_adapt_laser_scan(self._meas._h, ptr, n, mem, C.byref(self.params),
                                                     C.byref(out) if want_result else None))
        return self._finish(out, want_result)


def default_lidar_sweep_extras():
    """srrg2_lidar_sweep_extras with everything off: no ring table, no times, deskew 0, reference 1, identity motion"""
    from . import _capi

    x = abi.LidarSweepExtras()
    _capi.lib().srrg2_adapt_default_lidar_sweep_extras(C.byref(x))
    return x


class MeasurementAdaptorLidarSweep(_AdaptorBase):
    """params: abi.LidarAdaptorParams (model, gaps, gate, drop, compact).  In compact mode the scene's global indices are the
    pixel indices row*cols + col of the range image.  ``set_ring_elevations`` and ``set_motion`` switch on the per-ring table
    and the de-skew of srrg2_adapt_lidar_sweep_ex; without them compute() is srrg2_adapt_lidar_sweep."""

    def __init__(self, params=None):
        super().__init__()
        self.params = params or default_lidar_params()
        self._raw = None
        self._rings = None
        self._motion = None  # (motion (12,) float32, reference, time_begin, time_end)

    def set_model(self, model):
        """copy an abi.SphericalModel (e.g. from ``spherical_model_full_turn``) into the params"""
        C.memmove(C.byref(self.params.model), C.byref(model), C.sizeof(abi.SphericalModel))

    def set_ring_elevations(self, elevations):
        """one elevation (radians) per row of the model, strictly ascending or descending (the model's elevation_min /
        elevation_increment are then ignored); None: the model's uniform rows.  A copy is kept."""
        self._rings = None if elevations is None else np.array(elevations, dtype=np.float64).reshape(-1)

    def set_motion(self, motion, reference=1.0, time_begin=None, time_end=None):
        """de-skew the sweep: ``motion`` is the 3x4 [R|t] of the sensor at the sweep's end in its frame at the sweep's start
        (prev^-1 * curr of a constant-velocity model), ``reference`` the normalised time of the frame the scene is expressed in
        (1: the end).  ``time_begin`` / ``time_end`` say which per-point times (``set_raw_data(times=...)``) mean the start and
        the end; without per-point times the time comes from the raw azimuth.  ``motion=None`` switches the de-skew off."""
        if motion is None:
            self._motion = None
            return
        m = np.ascontiguousarray(np.asarray(motion, np.float32).reshape(-1)[:12])
        if m.shape[0] != 12:
            raise ValueError("motion: a 3x4 (or 4x4) matrix expected")
        self._motion = (m, float(reference), time_begin, time_end)

    def set_raw_data(self, points, intensity=None, times=None):
        """points: (n, 3) float32 array of x, y, z in the sensor frame, or (n, 4) of x, y, z, intensity (then ``intensity``
        must be None), or (n, 5) of x, y, z, intensity, time (then ``times`` must be None as well), or a
        (device_pointer, stride_bytes, n) triple; intensity: (n,) floats, or a (device_pointer, stride_bytes) pair next to device
        points; times: likewise, one float32 per point (read only when a motion is set).  The arrays are read at compute()."""
        if isinstance(points, tuple):
            ptr, stride, n = points
            iptr, istride = (None, 0) if intensity is None else (C.c_void_p(int(intensity[0])), int(intensity[1]))
            tptr, tstride = (None, 0) if times is None else (C.c_void_p(int(times[0])), int(times[1]))
            self._raw = (None, C.c_void_p(int(ptr)), int(stride), iptr, istride, int(n), abi.MEM_DEVICE, tptr, tstride)
        else:
            a = np.asarray(points)
            if a.ndim != 2 or a.shape[1] not in (3, 4, 5):
                raise ValueError("points: an (n, 3), (n, 4) or (n, 5) array expected, got %s" % (a.shape,))
            a = np.ascontiguousarray(a, dtype=np.float32)
            n, w = a.shape
            keep, iptr, istride, tptr, tstride = [a], None, 0, None, 0
            if w >= 4:
                if intensity is not None:
                    raise ValueError("intensity: given twice (the points already have a fourth column)")
                iptr, istride = C.c_void_p(a.ctypes.data + 12), 4 * w
            elif intensity is not None:
                it = np.ascontiguousarray(intensity, dtype=np.float32).reshape(-1)
                if it.shape[0] != n:
                    raise ValueError("intensity: one value per point expected")
                keep.append(it)
                iptr, istride = C.c_void_p(it.ctypes.data), 4
            if w == 5:
                if times is not None:
                    raise ValueError("times: given twice (the points already have a fifth column)")
                tptr, tstride = C.c_void_p(a.ctypes.data + 16), 20
            elif times is not None:
                tm = np.ascontiguousarray(times, dtype=np.float32).reshape(-1)
                if tm.shape[0] != n:
                    raise ValueError("times: one value per point expected")
                keep.append(tm)
                tptr, tstride = C.c_void_p(tm.ctypes.data), 4
            self._raw = (tuple(keep), C.c_void_p(a.ctypes.data), 4 * w, iptr, istride, n, abi.MEM_HOST, tptr, tstride)
        self._status = abi.ADAPTOR_ERROR

    def reset(self):
        self._raw = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None

    def _extras(self, tptr, tstride):
        """the srrg2_lidar_sweep_extras of this compute(), or None for the plain call"""
        if self._rings is None and self._motion is None:
            return None
        x = default_lidar_sweep_extras()
        if self._rings is not None:
            if self._rings.shape[0] != self.params.model.rows:
                raise ValueError("ring elevations: %d entries for %d rows" % (self._rings.shape[0], self.params.model.rows))
            x.ring_elevations = self._rings.ctypes.data_as(C.POINTER(C.c_double))
        if self._motion is not None:
            m, reference, t0, t1 = self._motion
            x.deskew, x.reference = 1, reference
            for i in range(12):
                x.motion[i] = float(m[i])
            if tptr is not None:
                if t0 is None or t1 is None:
                    raise ValueError("set_motion: time_begin and time_end are needed with per-point times")
                x.times, x.time_stride_bytes, x.time_begin, x.time_end = tptr.value, tstride, float(t0), float(t1)
        return x

    def compute(self, want_result=True):
        self._ready()
        out = abi.AdaptResult()
        _, ptr, stride, iptr, istride, n, mem, tptr, tstride = self._raw
        x = self._extras(tptr, tstride)
        res = C.byref(out) if want_result else None
        if x is None:
            rc = self._lib.srrg2_adapt_lidar_sweep(self._meas._h, ptr, stride, iptr, istride, n, mem, C.byref(self.params), res)
        else:
            rc = self._lib.srrg2_adapt_lidar_sweep_ex(self._meas._h, ptr, stride, iptr, istride, n, mem, C.byref(self.params),
                                                      C.byref(x), res)
        self._check(rc)
        return self._finish(out, want_result)


def default_feature_params():
    """srrg2_feature_params: fast_threshold 20, max_features 1000, oriented 1"""
    from . import _capi

    p = abi.FeatureParams()
    _capi.lib().srrg2_adapt_default_feature_params(C.byref(p))
    return p


def feature_pattern(angle_bin):
    """srrg2_feature_pattern: the (256, 4) int8 point pairs (ax, ay, bx, by) of an orientation bin; needs no device"""
    from . import _capi

    out = np.zeros((256, 4), np.int8)
    lib = _capi.lib()
    if lib.srrg2_feature_pattern(int(angle_bin), out.ctypes.data_as(C.POINTER(C.c_int8))) != 0:
        msg = lib.srrg2_amd_last_error()
        raise ValueError(msg.decode() if msg else "feature_pattern")
    return out


class MeasurementAdaptorImageFeatures(_AdaptorBase):
    """params: abi.FeatureParams (fast_threshold, max_features, oriented); camera: abi.DepthAdaptorParams, of which the
    camera matrix and the depth scale / gates are read (rows / cols are taken from a numpy image).  compute() leaves a compact
    scene of keypoints: point, 256-bit descriptor, intensity; global indices = pixel indices."""

    def __init__(self, params=None, camera=None):
        super().__init__()
        self.params = params or default_feature_params()
        self.camera = camera or default_depth_params()
        self._raw = self._depth = None
        self._keypoints = np.zeros((0, 4), np.int32)

    def set_camera_matrix(self, K):
        for i, v in enumerate(np.asarray(K, np.float32).reshape(9)):
            self.camera.camera_matrix[i] = float(v)

    def set_raw_data(self, intensity, depth=None, intensity_type=None, depth_type=None):
        """intensity (uint8) and optionally depth (uint16 counts / float32 metres): 2-D numpy arrays, or
        (device_pointer, row_stride_bytes) pairs with their abi.IMAGE_* type (then camera.rows / cols say the size)"""
        raw = _image(intensity, intensity_type, "intensity")
        dep = None if depth is None else _image(depth, depth_type, "depth")
        if dep is not None and (dep[4] != raw[4] or (raw[5] is not None and dep[5] != raw[5])):
            raise ValueError("depth: same memory space and shape as the intensity image expected")
        self._raw, self._depth = raw, dep
        if raw[5] is not None:
            self.camera.rows, self.camera.cols = raw[5]
        self._status = abi.ADAPTOR_ERROR

    def reset(self):
        self._raw = self._depth = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None
        self._keypoints = np.zeros((0, 4), np.int32)

    def compute(self, want_keypoints=True):
        """fills the measurement scene; returns the counters of srrg2_feature_result (dict)"""
        self._ready()
        out = abi.FeatureResult()
        _, iptr, itype, istride, mem, _ = self._raw
        if self._depth is None:
            dptr, dtype, dstride = None, abi.IMAGE_NONE, 0
        else:
            _, dptr, dtype, dstride, _, _ = self._depth
        cap = 0
        if want_keypoints:  # every selected keypoint fits: the cap, or every admissible pixel
            inner = max(self.camera.rows - 32, 0) * max(self.camera.cols - 32, 0)
            cap = min(inner, self.params.max_features) if self.params.max_features > 0 else inner
        buf = np.zeros((max(cap, 1), 4), np.int32)
        self._check(self._lib.srrg2_adapt_image_features(self._meas._h, iptr, itype, istride, dptr, dtype, dstride, mem,
                                                         C.byref(self.camera), C.byref(self.params),
                                                         buf.ctypes.data_as(C.POINTER(abi.Keypoint)) if cap > 0 else None, cap,
                                                         C.byref(out)))
        self._keypoints = buf[:min(out.scene_size, cap)]
        return self._finish(out, True)

    def keypoints(self):
        """(n, 4) int32 rows of pixel, score, angle_bin, 0 of the last compute(), aligned with the scene's points"""
        return self._keypoints


def default_pyramid_params():
    """srrg2_pyramid_params: 4 levels at 6/5"""
    from . import _capi

    p = abi.PyramidParams()
    _capi.lib().srrg2_adapt_default_pyramid_params(C.byref(p))
    return p


PYRAMID_KEYPOINT_DTYPE = np.dtype([(n, np.int32) for n, _ in abi.PyramidKeypoint._fields_])


class MeasurementAdaptorImageFeaturesPyramid(MeasurementAdaptorImageFeatures):
    """MeasurementAdaptorImageFeatures over a scale pyramid (pyramid: abi.PyramidParams -- num_levels, scale_num / scale_den):
    compute() leaves ONE compact scene of the keypoints of every level, level-major; the points lie at the keypoints' level-0
    positions, global indices = nearest level-0 pixel (the same pixel may appear once per level)."""

    def __init__(self, params=None, camera=None, pyramid=None):
        super().__init__(params, camera)
        self.pyramid = pyramid or default_pyramid_params()
        self._keypoints = np.zeros(0, PYRAMID_KEYPOINT_DTYPE)

    def reset(self):
        super().reset()
        self._keypoints = np.zeros(0, PYRAMID_KEYPOINT_DTYPE)

    def compute(self, want_keypoints=True):
        """fills the measurement scene; returns the counters of srrg2_pyramid_result (dict, per-level lists)"""
        self._ready()
        out = abi.PyramidResult()
        _, iptr, itype, istride, mem, _ = self._raw
        if self._depth is None:
            dptr, dtype, dstride = None, abi.IMAGE_NONE, 0
        else:
            _, dptr, dtype, dstride, _, _ = self._depth
        cap = 0
        if want_keypoints:  # every selected keypoint fits: the cap, or every admissible pixel of every level
            if self.params.max_features > 0:
                cap = self.params.max_features
            else:
                rows, cols = self.camera.rows, self.camera.cols
                for _ in range(max(self.pyramid.num_levels, 0)):
                    cap += max(rows - 32, 0) * max(cols - 32, 0)
                    rows = rows * self.pyramid.scale_den // max(self.pyramid.scale_num, 1)
                    cols = cols * self.pyramid.scale_den // max(self.pyramid.scale_num, 1)
        buf = np.zeros(max(cap, 1), PYRAMID_KEYPOINT_DTYPE)
        self._check(self._lib.srrg2_adapt_image_features_pyramid(
            self._meas._h, iptr, itype, istride, dptr, dtype, dstride, mem, C.byref(self.camera), C.byref(self.params),
            C.byref(self.pyramid), buf.ctypes.data_as(C.POINTER(abi.PyramidKeypoint)) if cap > 0 else None, cap, C.byref(out)))
        self._keypoints = buf[:min(out.scene_size, cap)]
        return self._finish(out, True)

    def keypoints(self):
        """(n,) structured array (pixel, score, angle_bin, level, level_pixel, u_q8, v_q8, reserved) of the last compute(),
        aligned with the scene's points"""
        return self._keypoints


def default_stereo_params():
    """srrg2_stereo_params: baseline 0 (set it), disparity 1 .. 128, row_tolerance 1, max_distance 48, cross_check 1, subpixel 1"""
    from . import _capi

    p = abi.StereoParams()
    _capi.lib().srrg2_adapt_default_stereo_params(C.byref(p))
    return p


MATCH_DTYPE = np.dtype([("left_pixel", np.int32), ("right_pixel", np.int32), ("distance", np.int32), ("disparity", np.float32)])


class MeasurementAdaptorStereoFeatures(_AdaptorBase):
    """params: abi.FeatureParams (per image); stereo: abi.StereoParams (baseline, disparity range, row tolerance, gates);
    camera: abi.DepthAdaptorParams, of which the camera matrix and depth_min / depth_max are read (rows / cols are taken from
    numpy images).  compute() leaves a compact scene of the left image's matched keypoints: triangulated point, left
    descriptor, left intensity; global indices = left pixel indices."""

    def __init__(self, params=None, stereo=None, camera=None):
        super().__init__()
        self.params = params or default_feature_params()
        self.stereo = stereo or default_stereo_params()
        self.camera = camera or default_depth_params()
        self._raw = self._right = None
        self._keypoints = np.zeros((0, 4), np.int32)
        self._matches = np.zeros(0, MATCH_DTYPE)

    def set_camera_matrix(self, K):
        for i, v in enumerate(np.asarray(K, np.float32).reshape(9)):
            self.camera.camera_matrix[i] = float(v)

    def set_raw_data(self, left, right):
        """the rectified pair (uint8): 2-D numpy arrays of one shape, or (device_pointer, row_stride_bytes) pairs (then
        camera.rows / cols say the size)"""
        raw = _image(left, abi.IMAGE_U8, "left")
        other = _image(right, abi.IMAGE_U8, "right")
        if raw[2] != abi.IMAGE_U8 or other[2] != abi.IMAGE_U8:
            raise ValueError("left / right: uint8 images expected")
        if other[4] != raw[4] or other[5] != raw[5]:
            raise ValueError("right: same memory space and shape as the left image expected")
        self._raw, self._right = raw, other
        if raw[5] is not None:
            self.camera.rows, self.camera.cols = raw[5]
        self._status = abi.ADAPTOR_ERROR

    def reset(self):
        self._raw = self._right = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None
        self._keypoints = np.zeros((0, 4), np.int32)
        self._matches = np.zeros(0, MATCH_DTYPE)

    def compute(self, want_records=True):
        """fills the measurement scene; returns the counters of srrg2_stereo_result (dict)"""
        self._ready()
        out = abi.StereoResult()
        _, lptr, _, lstride, mem, _ = self._raw
        _, rptr, _, rstride, _, _ = self._right
        cap = 0
        if want_records:  # every left keypoint fits: the cap, or every admissible pixel
            inner = max(self.camera.rows - 32, 0) * max(self.camera.cols - 32, 0)
            cap = min(inner, self.params.max_features) if self.params.max_features > 0 else inner
        kps = np.zeros((max(cap, 1), 4), np.int32)
        ms = np.zeros(max(cap, 1), MATCH_DTYPE)
        self._check(self._lib.srrg2_adapt_stereo_features(self._meas._h, lptr, lstride, rptr, rstride, mem, C.byref(self.camera),
                                                          C.byref(self.params), C.byref(self.stereo),
                                                          kps.ctypes.data_as(C.POINTER(abi.Keypoint)) if cap > 0 else None, cap,
                                                          ms.ctypes.data_as(C.POINTER(abi.StereoMatch)) if cap > 0 else None, cap,
                                                          C.byref(out)))
        got = min(out.scene_size, cap)
        self._keypoints, self._matches = kps[:got], ms[:got]
        return self._finish(out, True)

    def keypoints(self):
        """(n, 4) int32 rows of left pixel, score, angle_bin, 0 of the last compute(), aligned with the scene's points"""
        return self._keypoints

    def matches(self):
        """(n,) structured array (left_pixel, right_pixel, distance, disparity) of the last compute(), in the scene's order"""
        return self._matches


def default_dense_stereo_params():
    """srrg2_dense_stereo_params: baseline 0 (set it), disparity 1 .. 64, paths 4, p1 8, p2 48, uniqueness_ratio 10, lr_check 1,
    lr_tolerance 1, subpixel 1"""
    from . import _capi

    p = abi.DenseStereoParams()
    _capi.lib().srrg2_adapt_default_dense_stereo_params(C.byref(p))
    return p


class MeasurementAdaptorStereoDense(_AdaptorBase):
    """stereo: abi.DenseStereoParams (baseline, disparity range, paths, penalties, uniqueness, left-right check, sub-pixel);
    camera: abi.DepthAdaptorParams, all of it (rows / cols are taken from numpy images): compute() leaves the scene that
    MeasurementAdaptorDepthImage leaves for the depth fx * baseline / disparity with the left image as its intensity --
    organised or compact, with normals by the gaps.  Without a measurement scene (``set_meas`` never called, or with None) only
    the disparity image is computed."""

    def __init__(self, stereo=None, camera=None):
        super().__init__()
        self.stereo = stereo or default_dense_stereo_params()
        self.camera = camera or default_depth_params()
        self._raw = self._right = None
        self._disparity = None

    def set_camera_matrix(self, K):
        for i, v in enumerate(np.asarray(K, np.float32).reshape(9)):
            self.camera.camera_matrix[i] = float(v)

    def set_raw_data(self, left, right):
        """the rectified pair (uint8): 2-D numpy arrays of one shape, or (device_pointer, row_stride_bytes) pairs (then
        camera.rows / cols say the size)"""
        raw = _image(left, abi.IMAGE_U8, "left")
        other = _image(right, abi.IMAGE_U8, "right")
        if raw[2] != abi.IMAGE_U8 or other[2] != abi.IMAGE_U8:
            raise ValueError("left / right: uint8 images expected")
        if other[4] != raw[4] or other[5] != raw[5]:
            raise ValueError("right: same memory space and shape as the left image expected")
        self._raw, self._right = raw, other
        if raw[5] is not None:
            self.camera.rows, self.camera.cols = raw[5]
        self._status = abi.ADAPTOR_ERROR

    def reset(self):
        self._raw = self._right = None
        self._status = abi.ADAPTOR_INITIALIZING
        self.last = None
        self._disparity = None

    def compute(self, want_result=True, want_disparity=False):
        """fills the measurement scene; returns the counters of srrg2_dense_stereo_result (dict), or None with
        ``want_result=False`` -- an organised adapt whose disparity stays on the device then only queues its work.
        want_disparity: True with numpy images (``disparity()`` then gives the (rows, cols) float32 image), or the float32 array
        that shall receive it (its bytes between rows are left alone); with device images a (device_pointer, row_stride_bytes)
        pair that receives it."""
        if self._raw is None:
            raise RuntimeError("%s::compute|raw data not set" % type(self).__name__)
        out = abi.DenseStereoResult()
        _, lptr, _, lstride, mem, _ = self._raw
        _, rptr, _, rstride, _, _ = self._right
        self._disparity = None
        dptr, dstride = None, 0
        if isinstance(want_disparity, tuple):
            if mem != abi.MEM_DEVICE:
                raise ValueError("want_disparity: a (device_pointer, stride) pair goes with device images")
            dptr, dstride = C.c_void_p(int(want_disparity[0])), int(want_disparity[1])
            self._disparity = want_disparity
        elif isinstance(want_disparity, np.ndarray):  # the caller's own image, rows at its stride
            a = want_disparity
            if mem != abi.MEM_HOST or a.dtype != np.float32 or a.shape != (self.camera.rows, self.camera.cols) or \
                    (a.size and a.strides[1] != 4):
                raise ValueError("want_disparity: a (rows, cols) float32 array with unit column stride goes with numpy images")
            self._disparity = a
            dptr, dstride = C.c_void_p(a.ctypes.data), int(a.strides[0]) if a.shape[0] > 1 else 4 * self.camera.cols
        elif want_disparity:
            if mem != abi.MEM_HOST:
                raise ValueError("want_disparity: device images need a (device_pointer, stride) pair")
            self._disparity = np.zeros((self.camera.rows, self.camera.cols), np.float32)
            dptr, dstride = C.c_void_p(self._disparity.ctypes.data), 4 * self.camera.cols
        self._check(self._lib.srrg2_adapt_stereo_dense(None if self._meas is None else self._meas._h, lptr, lstride, rptr, rstride,
                                                       mem, C.byref(self.camera), C.byref(self.stereo), dptr, dstride,
                                                       C.byref(out) if want_result else None))
        return self._finish(out, want_result)

    def disparity(self):
        """the disparity image of the last compute() that asked for it: a (rows, cols) float32 array, 0 where a pixel has none
        (or the device pair that was handed in); None otherwise"""
        return self._disparity
