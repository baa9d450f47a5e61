"""Python mirror of the TSDF volume over the C ABI (srrg2_tsdf_*): depth frames and the poses they were taken from -> one
truncated signed-distance volume on the device, the dense model of the 3-D pipeline.

``TsdfVolume``  ``reset(nx, ny, nz, voxel_size, origin, with_intensity)`` allocates the int32 planes (sum, weight, isum);
                ``integrate(depth, poses, intensity)`` fuses a batch of frames (one frame = the per-frame update), ``remove`` takes
                the same frames out again (weight -1: after a pose-graph optimisation only the frames whose pose moved are
                re-integrated); ``planes()`` reads the volume; ``raycast(pose, scene)`` renders it as a camera at that pose would
                measure it and runs the depth adaptor on the result -- the scene is what the projective finder takes as
                ``set_fixed`` (frame-to-model tracking); ``to_scene(scene)`` exports the surface as a 3-D cloud with normals.

Thin marshalling only; the contract is DESIGN.md section 4 "TSDF volume", its restatement tests/tsdf_restatement.py.
"""
import ctypes as C

import numpy as np

from . import _abi as abi

_TYPES = {np.dtype(np.uint8): abi.IMAGE_U8, np.dtype(np.uint16): abi.IMAGE_U16, np.dtype(np.float32): abi.IMAGE_F32}


def _images(a, what):
    """(keep-alive, pointer, type, row stride in bytes, mem) of K images: a (K, rows, cols) numpy array with unit column stride
    and frames one behind the other (rows may be padded), a contiguous torch tensor, or a (device_pointer, image_type,
    row_stride_bytes) triple"""
    if a is None:
        return None, None, abi.IMAGE_NONE, 0, None
    if isinstance(a, tuple):
        return a, C.c_void_p(int(a[0])), int(a[1]), int(a[2]), abi.MEM_DEVICE
    if hasattr(a, "data_ptr"):  # a torch tensor
        if not a.is_contiguous() or a.dim() != 3:
            raise ValueError("%s: a contiguous (K, rows, cols) tensor expected" % what)
        dt = np.dtype(str(a.dtype).replace("torch.", ""))
        return a, C.c_void_p(a.data_ptr()), _TYPES[dt], int(a.shape[2]) * dt.itemsize, abi.MEM_DEVICE if a.is_cuda else abi.MEM_HOST
    a = np.asarray(a)
    if a.ndim != 3 or a.dtype not in _TYPES:
        raise ValueError("%s: a (K, rows, cols) uint8 / uint16 / float32 array expected" % what)
    if a.size and (a.strides[2] != a.itemsize or (a.shape[0] > 1 and a.strides[0] != a.shape[1] * a.strides[1])):
        a = np.ascontiguousarray(a)
    stride = int(a.strides[1]) if a.size and a.shape[1] > 1 else int(a.shape[2]) * a.itemsize
    return a, C.c_void_p(a.ctypes.data), _TYPES[a.dtype], stride, abi.MEM_HOST


class TsdfVolume:
    def __init__(self, device=0):
        from . import _capi

        self._lib = _capi.lib()
        self._h = C.c_void_p()
        self.device = int(device)
        self.params = abi.TsdfParams()
        self._lib.srrg2_tsdf_default_params(C.byref(self.params))
        self.frame = abi.TsdfFrameParams()
        self._lib.srrg2_tsdf_default_frame_params(C.byref(self.frame))
        self.ray = abi.TsdfRaycastParams()
        self._lib.srrg2_tsdf_default_raycast_params(C.byref(self.ray))
        self.camera = abi.DepthAdaptorParams()
        self._lib.srrg2_adapt_default_depth_params(C.byref(self.camera))
        self._check(self._lib.srrg2_tsdf_create(self.device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.srrg2_tsdf_destroy(self._h)  # (waits for queued work)
            self._h = C.c_void_p()

    close = __del__

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    @property
    def shape(self):
        """(nz, ny, nx): the shape of a plane as a numpy array"""
        return self.params.nz, self.params.ny, self.params.nx

    def reset(self, nx, ny, nz, voxel_size=0.02, origin=(0.0, 0.0, 0.0), with_intensity=False):
        """a new, empty volume of nx x ny x nz voxels; origin: world position of the corner of voxel (0, 0, 0)"""
        p = abi.TsdfParams()
        p.nx, p.ny, p.nz, p.voxel_size, p.with_intensity = int(nx), int(ny), int(nz), float(voxel_size), int(with_intensity)
        for i in range(3):
            p.origin[i] = float(origin[i])
        self._check(self._lib.srrg2_tsdf_reset(self._h, C.byref(p)))
        self.params = p

    def set_camera(self, K, rows, cols, depth_scale=0.001, depth_min=0.4, depth_max=8.0, **adaptor):
        """the camera of the frames and of the raycast; ``adaptor``: further fields of srrg2_depth_adaptor_params (normal gaps,
        normal_max_distance_squared, drop_points_without_normal, compact) that the raycast hands to the depth adaptor"""
        c = self.camera
        for i, v in enumerate(np.asarray(K, np.float32).reshape(9)):
            c.camera_matrix[i] = float(v)
        c.rows, c.cols, c.depth_scale, c.depth_min, c.depth_max = int(rows), int(cols), float(depth_scale), float(depth_min), float(depth_max)
        for k, v in adaptor.items():
            setattr(c, k, v)
        return c

    def integrate(self, depth, poses, intensity=None, weight=+1, want_result=True):
        """depth: (K, rows, cols) uint16 or float32, intensity: None or (K, rows, cols) uint8 / float32, both numpy arrays or both
        torch tensors on the device; poses: (K, 3, 4) camera_in_world, on the host.  One upload and a number of launches that does
        not depend on K.  want_result: wait and return the counters of srrg2_tsdf_result (dict); False: only queue the work on the
        volume's stream and return None."""
        poses = np.ascontiguousarray(poses, np.float32)
        K = poses.size // 12
        if poses.size != 12 * K:
            raise ValueError("poses: (K, 3, 4) expected, got %s" % (poses.shape,))
        dk, dptr, dtype, dstride, dmem = _images(depth, "depth")
        ik, iptr, itype, istride, imem = _images(intensity, "intensity")
        if imem is not None and imem != dmem:
            raise ValueError("depth and intensity must live in one memory space")
        out = abi.TsdfResult() if want_result else None
        self._check(self._lib.srrg2_tsdf_integrate_frames(self._h, dptr, dtype, dstride, iptr, itype, istride, K,
                                                          C.c_void_p(poses.ctypes.data), abi.MEM_HOST if dmem is None else dmem,
                                                          C.byref(self.camera), C.byref(self.frame), int(weight),
                                                          C.byref(out) if want_result else None))
        self._queued = (dk, ik)  # (device inputs of a queued call stay alive until the next call)
        return out.as_dict() if want_result else None

    def remove(self, depth, poses, intensity=None, want_result=True):
        """takes frames out that were integrated with the same images, poses, camera and mu: the planes are restored bit for bit"""
        return self.integrate(depth, poses, intensity, -1, want_result)

    def planes(self):
        """(sum, weight, isum or None): (nz, ny, nx) int32 arrays"""
        got = [np.zeros(self.shape, np.int32) for _ in range(3 if self.params.with_intensity else 2)]
        ptrs = [C.c_void_p(a.ctypes.data) for a in got] + [None] * (3 - len(got))
        self._check(self._lib.srrg2_tsdf_get_planes(self._h, ptrs[0], ptrs[1], ptrs[2], abi.MEM_HOST))
        return got[0], got[1], (got[2] if len(got) == 3 else None)

    def device_arrays(self):
        """(sum, weight, isum) pointers of the planes in device memory (isum 0 without the plane), valid until the next reset"""
        p = [C.POINTER(C.c_int32)() for _ in range(3)]
        self._check(self._lib.srrg2_tsdf_device_arrays(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2])))
        return tuple(C.cast(q, C.c_void_p).value or 0 for q in p)

    def raycast(self, pose, scene=None, want_depth=True):
        """renders the volume from camera_in_world ``pose`` ((3, 4)) with the camera of ``set_camera`` and ``self.ray``; the depth
        image goes through the depth adaptor into ``scene`` (a 3-D ``mapping.Scene``; None: no scene).  Returns (depth image
        (rows, cols) float32 or None, srrg2_tsdf_raycast_result as a dict).  want_depth may be a device pointer: the image is
        written there and None returned in its place."""
        pose = np.ascontiguousarray(pose, np.float32)
        if pose.size != 12:
            raise ValueError("pose: (3, 4) expected")
        depth, dptr, dmem = None, None, abi.MEM_HOST
        if want_depth is True:
            depth = np.zeros((max(self.camera.rows, 0), max(self.camera.cols, 0)), np.float32)
            dptr = C.c_void_p(depth.ctypes.data)
        elif want_depth:
            dptr, dmem = C.c_void_p(int(want_depth)), abi.MEM_DEVICE
        out = abi.TsdfRaycastResult()
        self._check(self._lib.srrg2_tsdf_raycast(self._h, C.c_void_p(pose.ctypes.data), C.byref(self.camera), C.byref(self.ray),
                                                 scene._h if scene is not None else None, dptr, dmem, C.byref(out)))
        return depth, out.as_dict()

    def to_scene(self, scene, min_weight=1):
        """every zero crossing of the volume between a voxel and its +x, +y or +z neighbour -> a point with the voxel's gradient
        as its normal in ``scene`` (a 3-D ``mapping.Scene``), in (voxel, axis) order; ``scene.global_indices()`` are
        3 * plane index + axis.  Returns the number of points."""
        out = abi.TsdfExportResult()
        self._check(self._lib.srrg2_tsdf_to_scene(self._h, int(min_weight), scene._h, C.byref(out)))
        return out.num_points
