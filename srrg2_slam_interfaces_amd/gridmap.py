"""Python mirror of the occupancy grid over the C ABI (srrg2_gridmap_*): laser scans and the poses they were taken from ->
which cells of a 2-D grid are free, occupied or never seen, on the device.

``OccupancyGrid``  ``reset(rows, cols, resolution, origin)`` allocates the two int32 planes (hits, misses);
                   ``integrate(ranges, poses)`` traces a batch of scans (one scan = the per-frame update), ``remove`` takes the
                   same scans out again (weight -1: after a pose-graph optimisation only the scans whose pose moved are re-drawn);
                   ``counts()`` / ``render()`` read the map, ``to_scene(scene)`` exports the occupied cells as a 2-D scene the
                   aligner takes as it is (scan-to-map tracking).
                   ``build_likelihood()`` smooths the occupied cells into a likelihood field, ``match_scans(ranges, guesses, ...)``
                   scores every pose of a window around each guess against it and returns the best (a pose for a scan whose
                   guess is too far off for ICP); ``likelihood()`` reads the field.
                   ``build_bounds()`` builds the pyramid of upper bounds over the field, ``match_scans_pruned`` searches the
                   same window through it (the same answer without scoring most of it) and ``localize(ranges, theta_step)``
                   places scans that have no guess at all against the whole map; ``bounds(level)`` reads a plane.

Thin marshalling only; the contract is DESIGN.md section 4 "Occupancy grid", "Correlative scan matching" and "Pruned scan matching",
its restatements tests/gridmap_restatement.py, tests/scan_match_restatement.py and tests/scan_match_pruned_restatement.py.
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
        self._bounds_levels = 0  # (the levels of bound planes built from the field as it is: every call that makes it stale clears them)

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
        self._bounds_levels = 0
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

    # ---- correlative scan matching (DESIGN.md section 4 "Correlative scan matching", tests/scan_match_restatement.py) ----------

    def build_likelihood(self, min_observations=1, occupied_percent=50, radius_cells=4, lut=None):
        """the likelihood field of the map as it is now: per cell the maximum of lut[dx^2 + dy^2] over the occupied cells within
        radius_cells.  lut: radius_cells^2 + 1 bytes (None: ``default_likelihood_lut``).  Every integrate / remove / reset makes
        the field stale: build it again before the next match."""
        lut = default_likelihood_lut(radius_cells) if lut is None else np.ascontiguousarray(lut, np.uint8)
        if 0 <= int(radius_cells) <= 16 and lut.size != int(radius_cells) ** 2 + 1:
            raise ValueError("lut: radius_cells^2 + 1 bytes expected")
        self._bounds_levels = 0
        self._check(self._lib.srrg2_gridmap_build_likelihood(self._h, int(min_observations), int(occupied_percent), int(radius_cells),
                                                             C.c_void_p(lut.ctypes.data)))

    def likelihood(self, out=None):
        """(rows, cols) uint8, the field; out: as in ``render``"""
        rows, cols = self.shape
        if isinstance(out, tuple):
            self._check(self._lib.srrg2_gridmap_get_likelihood(self._h, C.c_void_p(int(out[0])), int(out[1]), abi.MEM_DEVICE))
            return out
        if out is None:
            out = np.zeros((rows, cols), np.uint8)
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (rows, cols) or (out.size and out.strides[1] != 1):
            raise ValueError("out: a (rows, cols) uint8 array with unit column stride expected")
        stride = int(out.strides[0]) if rows > 1 else cols
        self._check(self._lib.srrg2_gridmap_get_likelihood(self._h, C.c_void_p(out.ctypes.data), stride, abi.MEM_HOST))
        return out

    def _match_inputs(self, ranges, guesses, half_window, half_steps_theta, theta_step):
        """what both matchers hand to the library: (keep-alives, ranges pointer, K, guesses pointer, mem, match params)"""
        nb = self.scan.num_beams
        rk, rptr, rmem, rshape = _floats(ranges, "ranges")
        pk, pptr, pmem, pshape = _floats(guesses, "guesses")
        if rmem != pmem:
            raise ValueError("ranges and guesses must live in one memory space")
        n_ranges, n_poses = int(np.prod(rshape)), int(np.prod(pshape))
        K = n_poses // 9
        if n_poses != 9 * K or n_ranges != K * nb:
            raise ValueError("ranges: (K, %d) and guesses: (K, 3, 3) expected, got %s and %s" % (nb, rshape, pshape))
        mp = abi.GridMapMatchParams()
        mp.half_window_x, mp.half_window_y, mp.half_steps_theta = int(half_window[0]), int(half_window[1]), int(half_steps_theta)
        mp.theta_step = float(theta_step)
        return (rk, pk), rptr, K, pptr, rmem, mp

    @staticmethod
    def _match_results(res, K):
        raw = np.frombuffer(res, np.uint8).reshape(max(K, 1), C.sizeof(abi.GridMapMatchResult))[:K]
        out = {"robot_in_world": raw[:, :36].copy().view(np.float32).reshape(K, 3, 3)}
        for i, name in enumerate(("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")):
            out[name] = raw[:, 36 + 4 * i:40 + 4 * i].copy().view(np.int32).reshape(K)
        return out

    def match_scans(self, ranges, guesses, half_window=(0, 0), half_steps_theta=0, theta_step=0.0, want_scores=False):
        """every pose of the window around each scan's guess scored against the likelihood field, the best one per scan.
        ranges: (K, num_beams) float32, guesses: (K, 3, 3) robot_in_world -- numpy arrays, or torch tensors on the device (both).
        half_window: (wx, wy) cells; the rotations are j * theta_step, |j| <= half_steps_theta.  Returns a dict of arrays over
        the K scans: robot_in_world (K, 3, 3), dx, dy, jtheta, score, score_at_guess, num_scored_beams; with want_scores also
        scores, the whole volume (K, Ntheta, Ny, Nx) int32 -- want_scores may be a contiguous int32 torch tensor of that many
        elements on the device, which is then filled and returned as it is."""
        keep, rptr, K, pptr, rmem, mp = self._match_inputs(ranges, guesses, half_window, half_steps_theta, theta_step)
        shape = (K, 2 * mp.half_steps_theta + 1, 2 * mp.half_window_y + 1, 2 * mp.half_window_x + 1)
        res = (abi.GridMapMatchResult * max(K, 1))()
        scores, sptr, smem = None, None, abi.MEM_HOST
        if hasattr(want_scores, "data_ptr"):
            import torch

            if want_scores.dtype != torch.int32 or not want_scores.is_contiguous() or not want_scores.is_cuda or \
                    want_scores.numel() != int(np.prod(shape)):
                raise ValueError("want_scores: a contiguous int32 device tensor of %d elements expected" % int(np.prod(shape)))
            scores, sptr, smem = want_scores, C.c_void_p(want_scores.data_ptr()), abi.MEM_DEVICE
        elif want_scores:
            refused = min(shape[1:]) < 1 or shape[0] * shape[1] * shape[2] * shape[3] > 2 ** 31 - 1
            scores = np.zeros((1, 1, 1, 1) if refused else shape, np.int32)  # (refused: the call says why and writes nothing)
            sptr = C.c_void_p(scores.ctypes.data)
        self._check(self._lib.srrg2_gridmap_match_scans(self._h, rptr, K, pptr, rmem, C.byref(self.scan), C.byref(mp), res, sptr, smem))
        out = self._match_results(res, K)
        if scores is not None:
            out["scores"] = scores
        return out

    # ---- pruned scan matching (DESIGN.md section 4 "Pruned scan matching", tests/scan_match_pruned_restatement.py) -------------

    def build_bounds(self, levels=4):
        """the bound planes P_1 .. P_levels of the field as it is now (levels 1 .. 6): what ``match_scans_pruned`` and ``localize``
        search through.  Whatever makes the field stale -- ``build_likelihood`` too -- makes them stale."""
        self._check(self._lib.srrg2_gridmap_build_bounds(self._h, int(levels)))
        self._bounds_levels = int(levels)

    def bounds(self, level):
        """(rows + s - 1, cols + s - 1) uint8, s = 2^level: [y + s - 1, x + s - 1] is the maximum of the field over the cells
        [x, x + s) x [y, y + s) inside the grid"""
        rows, cols = self.shape
        s = 1 << max(0, min(int(level), 6))
        out = np.zeros((rows + s - 1, cols + s - 1), np.uint8)
        self._check(self._lib.srrg2_gridmap_get_bounds(self._h, int(level), C.c_void_p(out.ctypes.data), cols + s - 1, abi.MEM_HOST))
        return out

    def match_scans_pruned(self, ranges, guesses, half_window=(0, 0), half_steps_theta=0, theta_step=0.0, levels=None, max_list_entries=0,
                           want_stats=False):
        """``match_scans`` through the bound planes: the same inputs, bit for bit the same dict (there is no volume), without
        scoring most of the window.  levels: how many of the built levels to use (None: all of them); max_list_entries: the
        blocks one scan may have listed at one level before it falls back to the exhaustive search (0: 2^20).  With want_stats
        the dict has "stats": one dict per scan (srrg2_gridmap_prune_stats)."""
        keep, rptr, K, pptr, rmem, mp = self._match_inputs(ranges, guesses, half_window, half_steps_theta, theta_step)
        pp = abi.GridMapPruneParams()
        if levels is None and getattr(self, "_bounds_levels", 0) == 0:
            raise RuntimeError("match_scans_pruned: the bound planes are stale or were never built (build_bounds)")
        pp.num_levels = int(self._bounds_levels if levels is None else levels)
        pp.max_list_entries = int(max_list_entries)
        res = (abi.GridMapMatchResult * max(K, 1))()
        stats = (abi.GridMapPruneStats * max(K, 1))() if want_stats else None
        self._check(self._lib.srrg2_gridmap_match_scans_pruned(self._h, rptr, K, pptr, rmem, C.byref(self.scan), C.byref(mp), C.byref(pp),
                                                               res, stats))
        out = self._match_results(res, K)
        if want_stats:
            out["stats"] = [stats[k].as_dict() for k in range(K)]
        return out

    def centre_pose(self):
        """(3, 3) float32: the centre of cell (cols // 2, rows // 2) at heading 0 (float64 arithmetic, rounded once)"""
        rows, cols = self.shape
        guess = np.eye(3, dtype=np.float32)
        guess[0, 2] = float(self.params.origin[0]) + (cols // 2 + 0.5) * float(self.params.resolution)
        guess[1, 2] = float(self.params.origin[1]) + (rows // 2 + 0.5) * float(self.params.resolution)
        return guess

    def localize(self, ranges, theta_step, levels=None, want_stats=False):
        """scans without any guess against the whole map: ``match_scans_pruned`` from the centre of cell (cols // 2, rows // 2) at
        heading 0 with the half window (cols // 2, rows // 2) and ceil(pi / theta_step) steps either way, so that every cell and
        the full turn are covered.  Builds the bound planes if they are stale (levels, or 4); the field must be fresh."""
        rows, cols = self.shape
        if getattr(self, "_bounds_levels", 0) < (levels or 1):
            self.build_bounds(levels or 4)
        nb = self.scan.num_beams
        K = int(np.prod(_floats(ranges, "ranges")[3])) // nb if nb > 0 else 0
        guesses = np.tile(self.centre_pose(), (K, 1, 1))
        if hasattr(ranges, "data_ptr") and ranges.is_cuda:
            import torch

            guesses = torch.from_numpy(guesses).to(ranges.device)
        half_steps = int(np.ceil(np.pi / float(theta_step)))
        return self.match_scans_pruned(ranges, guesses, (cols // 2, rows // 2), half_steps, theta_step, levels, 0, want_stats)


def default_likelihood_lut(radius_cells):
    """lut[d2] = (255 (R^2 + 1 - d2)) / (R^2 + 1), integer division: 255 on an occupied cell, falling linearly in the squared distance"""
    from . import _capi

    lib = _capi.lib()
    lut = np.zeros(max(int(radius_cells), 0) ** 2 + 1, np.uint8)
    if lib.srrg2_gridmap_default_likelihood_lut(int(radius_cells), C.c_void_p(lut.ctypes.data)) != 0:
        raise RuntimeError((lib.srrg2_amd_last_error() or b"").decode())
    return lut
