"""Python mirror of the occupancy grid over the C ABI (srrg2_gridmap_*): laser scans and the poses they were taken from ->
which cells of a 2-D grid are free, occupied or never seen, on the device.

``OccupancyGrid``  ``reset(rows, cols, resolution, origin)`` allocates the two int32 planes (hits, misses);
                   ``integrate(ranges, poses)`` traces a batch of scans (one scan = the per-frame update), ``remove`` takes the
                   same scans out again (weight -1: after a pose-graph optimisation only the scans whose pose moved are re-drawn);
                   ``counts()`` / ``render()`` read the map, ``to_scene(scene)`` exports the occupied cells as a 2-D scene the
                   aligner takes as it is (scan-to-map tracking).

Thin marshalling only; the contract is DESIGN.md section 4 "Occupancy grid", its restatement tests/gridmap_restatement.py.
"""
import ctypes as C

import numpy as np

from . import _abi as abi


def default_scan_params():
    """srrg2_gridmap_scan_params: identity sensor, 0.05 .. 30 m, clear_beyond_max = 1; bearings and num_beams are the caller's"""
    from . import _capi

    p = abi.GridMapScanParams()
    _capi.lib().srrg2_gridmap_default_scan_params(C.byref(p))
    return p


def _floats(a, what):
    """(keep-alive, pointer, mem, shape) of a float32 numpy array (host) or a contiguous float32 torch tensor on the device"""
    if hasattr(a, "data_ptr"):  # a torch tensor
        import torch

        if a.dtype != torch.float32 or not a.is_contiguous():
            raise ValueError("%s: a contiguous float32 tensor expected" % what)
        mem = abi.MEM_DEVICE if a.is_cuda else abi.MEM_HOST
        return a, C.c_void_p(a.data_ptr()), mem, tuple(a.shape)
    a = np.ascontiguousarray(a, np.float32)
    return a, C.c_void_p(a.ctypes.data), abi.MEM_HOST, a.shape


class OccupancyGrid:
    def __init__(self, device=0):
        from . import _capi

        self._lib = _capi.lib()
        self._h = C.c_void_p()
        self.device = int(device)
        self.params = abi.GridMapParams()
        self._lib.srrg2_gridmap_default_params(C.byref(self.params))
        self.scan = default_scan_params()
        self._check(self._lib.srrg2_gridmap_create(self.device, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.srrg2_gridmap_destroy(self._h)  # (waits for queued work)
            self._h = C.c_void_p()

    close = __del__

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    @property
    def shape(self):
        return self.params.rows, self.params.cols

    def reset(self, rows, cols, resolution=0.05, origin=(0.0, 0.0)):
        """a new, empty map of rows x cols cells; origin: world position of the corner of cell (0, 0)"""
        p = abi.GridMapParams()
        p.rows, p.cols, p.resolution = int(rows), int(cols), float(resolution)
        p.origin[0], p.origin[1] = float(origin[0]), float(origin[1])
        self._check(self._lib.srrg2_gridmap_reset(self._h, C.byref(p)))
        self.params = p

    def set_scan_model(self, angle_min, angle_increment, num_beams, range_min=0.05, range_max=30.0, sensor_in_robot=None,
                       clear_beyond_max=True):
        s = self.scan
        s.angle_min, s.angle_increment, s.num_beams = float(angle_min), float(angle_increment), int(num_beams)
        s.range_min, s.range_max, s.clear_beyond_max = float(range_min), float(range_max), 1 if clear_beyond_max else 0
        T = np.eye(3, dtype=np.float32) if sensor_in_robot is None else np.asarray(sensor_in_robot, np.float32).reshape(3, 3)
        for i, v in enumerate(T.reshape(9)):
            s.sensor_in_robot[i] = float(v)
        return s

    def integrate(self, ranges, poses, weight=+1, want_result=True):
        """ranges: (K, num_beams) float32, poses: (K, 3, 3) robot_in_world -- numpy arrays, or torch tensors on the device (both
        of them).  One upload and one kernel whatever K is.  want_result: wait and return the counters of srrg2_gridmap_result
        (dict); False: only queue the work on the grid's stream and return None."""
        nb = self.scan.num_beams
        rk, rptr, rmem, rshape = _floats(ranges, "ranges")
        pk, pptr, pmem, pshape = _floats(poses, "poses")
        if rmem != pmem:
            raise ValueError("ranges and poses must live in one memory space")
        n_ranges, n_poses = int(np.prod(rshape)), int(np.prod(pshape))
        K = n_poses // 9
        if n_poses != 9 * K or n_ranges != K * nb:
            raise ValueError("ranges: (K, %d) and poses: (K, 3, 3) expected, got %s and %s" % (nb, rshape, pshape))
        out = abi.GridMapResult() if want_result else None
        self._check(self._lib.srrg2_gridmap_integrate_scans(self._h, rptr, K, pptr, rmem, C.byref(self.scan), int(weight),
                                                            C.byref(out) if want_result else None))
        self._queued = (rk, pk)  # (device inputs of a queued call stay alive until the next call)
        return out.as_dict() if want_result else None

    def remove(self, ranges, poses, want_result=True):
        """takes scans out that were integrated with the same ranges, poses and scan model: the planes are restored bit for bit"""
        return self.integrate(ranges, poses, -1, want_result)

    def counts(self):
        """(hits, misses): two (rows, cols) int32 arrays"""
        rows, cols = self.shape
        hits, misses = np.zeros((rows, cols), np.int32), np.zeros((rows, cols), np.int32)
        self._check(self._lib.srrg2_gridmap_get_counts(self._h, C.c_void_p(hits.ctypes.data), C.c_void_p(misses.ctypes.data),
                                                       abi.MEM_HOST))
        return hits, misses

    def device_arrays(self):
        """(hits pointer, misses pointer) of the planes in device memory, valid until the next reset"""
        h, m = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        self._check(self._lib.srrg2_gridmap_device_arrays(self._h, C.byref(h), C.byref(m)))
        return C.cast(h, C.c_void_p).value or 0, C.cast(m, C.c_void_p).value or 0

    def render(self, min_observations=1, out=None):
        """(rows, cols) uint8: 0 .. 100 = percent of the observations that were hits, 255 = unknown (fewer than
        max(min_observations, 1) observations).  out: a uint8 array of that shape with unit column stride, filled in place
        (bytes between its rows are left alone), or a (device_pointer, row_stride_bytes) pair."""
        rows, cols = self.shape
        if isinstance(out, tuple):
            self._check(self._lib.srrg2_gridmap_render(self._h, int(min_observations), C.c_void_p(int(out[0])), int(out[1]),
                                                       abi.MEM_DEVICE))
            return out
        if out is None:
            out = np.zeros((rows, cols), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (rows, cols) or (out.size and out.strides[1] != 1):
            raise ValueError("out: a (rows, cols) uint8 array with unit column stride expected")
        stride = int(out.strides[0]) if rows > 1 else cols
        self._check(self._lib.srrg2_gridmap_render(self._h, int(min_observations), C.c_void_p(out.ctypes.data), stride, abi.MEM_HOST))
        return out

    def to_scene(self, scene, min_observations=1, occupied_percent=50):
        """every cell that renders into [occupied_percent, 100] -> a point at its centre in ``scene`` (a 2-D ``mapping.Scene``), in
        plane-index order; ``scene.global_indices()`` are the plane indices iy*cols + ix.  Returns the number of points."""
        self._check(self._lib.srrg2_gridmap_to_scene(self._h, int(min_observations), int(occupied_percent), scene._h))
        return scene.size()
