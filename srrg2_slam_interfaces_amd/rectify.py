"""Python mirror of the rectification stage over the C ABI (srrg2_rectifier_*, srrg2_rectify_image / _pair,
srrg2_stereo_rectify): lens undistortion and stereo rectification of raw images on the device, in front of the image adaptors.

``ImageRectifier``   one camera and one target: a map built on the device, images remapped through it (uint8 bilinear;
                     uint16 / float32 depth images nearest, identity rotation only)
``StereoRectifier``  two ``ImageRectifier``s set from a stereo calibration (``stereo_rectify``); ``rectify(left, right)`` remaps
                     both images in one launch and returns the device pairs the adaptors' ``set_raw_data`` takes

``rectify(..., order_on=scene)`` with a device destination only queues its work on that scene's stream: the adaptor that then
fills the scene from the rectified device image is ordered behind it, with no host wait between.  Thin marshalling only; the
contract is DESIGN.md section 4 "Rectification", its restatement tests/rectify_restatement.py.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .adaptors import _IMAGE_TYPES, _image

_ELEMENT = {abi.IMAGE_U8: 1, abi.IMAGE_U16: 2, abi.IMAGE_F32: 4}
_DTYPE = {abi.IMAGE_U8: np.uint8, abi.IMAGE_U16: np.uint16, abi.IMAGE_F32: np.float32}


def _doubles(v, n, what):
    a = np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
    if a.size != n:
        raise ValueError("%s: %d values expected, got %d" % (what, n, a.size))
    return a


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def default_rectifier_params():
    """srrg2_rectifier_params: zeros, identity rotation"""
    from . import _capi

    p = abi.RectifierParams()
    _capi.lib().srrg2_rectifier_default_params(C.byref(p))
    return p


def stereo_rectify(KL, KR, R, t):
    """srrg2_stereo_rectify (host only): both camera matrices and R, t with X_right = R X_left + t -> (R1, R2, Knew, baseline);
    the right camera then sits at +baseline along the rectified x axis.  Raises ValueError on a degenerate calibration."""
    from . import _capi

    lib = _capi.lib()
    R1, R2, Kn = (np.zeros(9, np.float64) for _ in range(3))
    b = C.c_double(0.0)
    rc = lib.srrg2_stereo_rectify(_dp(_doubles(KL, 9, "KL")), _dp(_doubles(KR, 9, "KR")), _dp(_doubles(R, 9, "R")),
                                  _dp(_doubles(t, 3, "t")), _dp(R1), _dp(R2), _dp(Kn), C.byref(b))
    if rc != 0:
        msg = lib.srrg2_amd_last_error()
        raise ValueError("%s (code %d)" % (msg.decode() if msg else "stereo_rectify", rc))
    return R1.reshape(3, 3), R2.reshape(3, 3), Kn.reshape(3, 3), b.value


class DeviceImage:
    """a rectified image in device memory: ``pair`` = (pointer, row stride in bytes), the form the adaptors' ``set_raw_data``
    takes; ``tensor`` keeps the memory alive; ``numpy()`` waits for the device and copies it to the host"""

    def __init__(self, tensor, shape, image_type):
        self.tensor, self.shape, self.image_type = tensor, shape, image_type
        self.pair = (tensor.data_ptr(), tensor.shape[1] if tensor.ndim == 2 else 0)

    def numpy(self):
        import torch

        torch.cuda.synchronize()
        rows, cols = self.shape
        raw = self.tensor.cpu().numpy()
        return np.ascontiguousarray(raw[:, :cols * _ELEMENT[self.image_type]]).view(_DTYPE[self.image_type]).reshape(rows, cols)


def _device_image(shape, image_type, device):
    """rows at a pitch of a multiple of 4 bytes (what the image adaptors read fastest)"""
    import torch

    rows, cols = shape
    pitch = (cols * _ELEMENT[image_type] + 3) // 4 * 4
    # (empty, not zeros: a fill on torch's stream would race the remap, which runs on the scene's or the rectifier's stream)
    return DeviceImage(torch.empty((rows, max(pitch, 4)), dtype=torch.uint8, device="cuda:%d" % device), shape, image_type)


class ImageRectifier:
    def __init__(self, device=0):
        from . import _capi

        self._lib = _capi.lib()
        self._h = C.c_void_p()
        self.device = int(device)
        self.params = default_rectifier_params()
        self.info = None
        self._check(self._lib.srrg2_rectifier_create(self.device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.srrg2_rectifier_destroy(self._h)  # (waits for work queued with this map)
            self._h = C.c_void_p()

    close = __del__

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    def set_camera(self, K, distortion=None, rotation=None, new_K=None, src_shape=None, dst_shape=None):
        """K: source camera matrix (3 x 3); distortion: up to 8 of k1, k2, p1, p2, k3, k4, k5, k6; rotation: X_rect = R X_src
        (default identity); new_K: the target's camera matrix (default K); dst_shape: default src_shape.  Builds the map on the
        device; returns the counts of srrg2_rectifier_info (dict)."""
        if src_shape is None:
            raise ValueError("set_camera: src_shape=(rows, cols) is required")
        p = self.params
        d = np.zeros(8, np.float64)
        if distortion is not None:
            given = np.asarray(distortion, np.float64).reshape(-1)
            if given.size > 8:
                raise ValueError("distortion: at most 8 coefficients")
            d[:given.size] = given
        for dst, src in ((p.camera_matrix, _doubles(K, 9, "K")), (p.distortion, d),
                         (p.rotation, _doubles(np.eye(3) if rotation is None else rotation, 9, "rotation")),
                         (p.new_camera_matrix, _doubles(K if new_K is None else new_K, 9, "new_K"))):
            for i, v in enumerate(src):
                dst[i] = float(v)
        p.src_rows, p.src_cols = (int(v) for v in src_shape)
        p.dst_rows, p.dst_cols = (int(v) for v in (src_shape if dst_shape is None else dst_shape))
        info = abi.RectifierInfo()
        self._check(self._lib.srrg2_rectifier_set(self._h, C.byref(p), C.byref(info)))
        self.info = info.as_dict()
        return self.info

    @property
    def dst_shape(self):
        return self.params.dst_rows, self.params.dst_cols

    def map(self):
        """(dst_rows, dst_cols, 2) int32: per target pixel (U, V) in 1/256 source pixel, INT32_MIN twice = invalid"""
        rows, cols = self.dst_shape
        uv = np.zeros((rows, cols, 2), np.int32)
        self._check(self._lib.srrg2_rectifier_get_map(self._h, uv.ctypes.data_as(C.POINTER(C.c_int32)), uv.size))
        return uv

    def camera(self, params=None):
        """the target's camera matrix, rows and cols written into an adaptor's abi.DepthAdaptorParams (a default one when none
        is given): ``adaptor.camera`` / ``adaptor.params`` of the adaptor that reads the rectified image"""
        from .adaptors import default_depth_params

        cam = default_depth_params() if params is None else params
        self._check(self._lib.srrg2_rectifier_camera(self._h, C.byref(cam)))
        return cam

    def rectify(self, img, out=None, order_on=None, border=0, image_type=None):
        """img: a 2-D uint8 / uint16 / float32 numpy array of the source's shape, or a (device_pointer, row_stride_bytes) pair
        with its abi.IMAGE_* ``image_type``.  out: None -- a numpy array for a numpy image, a ``DeviceImage`` for a device pair
        or whenever ``order_on`` is given; 'device' / 'host' to choose; a numpy array of the target's shape (filled in place,
        its bytes between rows left alone); or a (device_pointer, row_stride_bytes) pair.  order_on: the scene whose stream the
        work is queued on when the destination is in device memory (the call then returns without waiting)."""
        keep, sptr, stype, sstride, smem, shape = _image(img, image_type, "img")
        if shape is not None and tuple(shape) != (self.params.src_rows, self.params.src_cols):
            raise ValueError("img: shape %s expected, got %s" % ((self.params.src_rows, self.params.src_cols), tuple(shape)))
        rows, cols = self.dst_shape
        if out is None:
            out = "device" if (smem == abi.MEM_DEVICE or order_on is not None) else "host"
        result = None
        if isinstance(out, str):
            if out == "device":
                result = _device_image((rows, cols), stype, self.device)
                dptr, dstride, dmem = C.c_void_p(result.pair[0]), result.pair[1], abi.MEM_DEVICE
            elif out == "host":
                result = np.zeros((rows, cols), _DTYPE[stype])
                dptr, dstride, dmem = C.c_void_p(result.ctypes.data), cols * _ELEMENT[stype], abi.MEM_HOST
            else:
                raise ValueError("out: 'host' or 'device'")
        elif isinstance(out, tuple):
            dptr, dstride, dmem = C.c_void_p(int(out[0])), int(out[1]), abi.MEM_DEVICE
            result = out
        elif isinstance(out, DeviceImage):
            dptr, dstride, dmem = C.c_void_p(out.pair[0]), out.pair[1], abi.MEM_DEVICE
            result = out
        else:
            a = out
            if not isinstance(a, np.ndarray) or _IMAGE_TYPES.get(a.dtype) != stype or a.shape != (rows, cols) or \
                    (a.size and a.strides[1] != a.itemsize):
                raise ValueError("out: a (dst_rows, dst_cols) array of the image's type with unit column stride expected")
            dptr, dmem = C.c_void_p(a.ctypes.data), abi.MEM_HOST
            dstride = int(a.strides[0]) if rows > 1 else cols * a.itemsize
            result = a
        self._check(self._lib.srrg2_rectify_image(self._h, None if order_on is None else order_on._h, sptr, stype, sstride, smem,
                                                  dptr, dstride, dmem, int(border)))
        return result


class StereoRectifier:
    """left / right: the two ``ImageRectifier``s; after ``set_calibration``: R1, R2, new_K, baseline"""

    def __init__(self, device=0):
        self.device = int(device)
        self.left, self.right = ImageRectifier(device), ImageRectifier(device)
        self.R1 = self.R2 = self.new_K = self.baseline = None

    def set_calibration(self, KL, dist_left, KR, dist_right, R, t, src_shape, dst_shape=None, new_K=None):
        """R, t: X_right = R X_left + t.  Both maps are built for one target (``new_K`` default: the shared camera of
        ``stereo_rectify``; dst_shape default: src_shape).  Returns the two infos."""
        self.R1, self.R2, Kn, self.baseline = stereo_rectify(KL, KR, R, t)
        self.new_K = Kn if new_K is None else np.asarray(new_K, np.float64).reshape(3, 3)
        return (self.left.set_camera(KL, dist_left, self.R1, self.new_K, src_shape, dst_shape),
                self.right.set_camera(KR, dist_right, self.R2, self.new_K, src_shape, dst_shape))

    def camera(self, params=None):
        """the shared target camera into an adaptor's params (``StereoDense.camera``); the baseline goes into its stereo params"""
        return self.left.camera(params)

    def rectify(self, left, right, order_on=None, border=0, out=None):
        """left, right: uint8 numpy arrays, or (device_pointer, row_stride_bytes) pairs.  Returns two ``DeviceImage``s whose
        ``pair`` the adaptors' ``set_raw_data`` takes (``out``: two of them to reuse); with ``order_on`` the call only queues."""
        lk, lptr, _, lstride, lmem, lshape = _image(left, abi.IMAGE_U8, "left")
        rk, rptr, _, rstride, rmem, rshape = _image(right, abi.IMAGE_U8, "right")
        if lmem != rmem or (lk is not None and (lk.dtype != np.uint8 or rk.dtype != np.uint8)):
            raise ValueError("left / right: uint8 images in one memory space expected")
        for shape, r, what in ((lshape, self.left, "left"), (rshape, self.right, "right")):
            if shape is not None and tuple(shape) != (r.params.src_rows, r.params.src_cols):
                raise ValueError("%s: shape %s expected" % (what, (r.params.src_rows, r.params.src_cols)))
        if out is None:
            out = (_device_image(self.left.dst_shape, abi.IMAGE_U8, self.device),
                   _device_image(self.right.dst_shape, abi.IMAGE_U8, self.device))
        dl, dr = out
        lib = self.left._lib
        self.left._check(lib.srrg2_rectify_pair(self.left._h, self.right._h, None if order_on is None else order_on._h, lptr, lstride,
                                                rptr, rstride, lmem, C.c_void_p(dl.pair[0]), dl.pair[1], C.c_void_p(dr.pair[0]),
                                                dr.pair[1], abi.MEM_DEVICE, int(border)))
        return dl, dr
