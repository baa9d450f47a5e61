"""Python mirror of the measurement adaptors over the C ABI (srrg2_adapt_*): raw sensor data -> measurement scene, on the device.

``MeasurementAdaptorDepthImage``   depth image (uint16 counts or float32 metres, + optional intensity image) -> organised
                                   or compact 3-D scene with normals
``MeasurementAdaptorLaserScan``    ranges -> 2-D scene with normals

Method names follow ``RawDataPreprocessor_`` (S/raw_data_preprocessors/raw_data_preprocessor.h:13-88), snake_case:
``set_raw_data``, ``set_meas``, ``compute``, ``status``, ``reset``; ``status()`` is ERROR after ``set_raw_data`` until
``compute()`` (:67-72).  Thin marshalling only; product library only (the oracle has no adaptor: the parity target is
tests/adaptor_restatement.py).
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
