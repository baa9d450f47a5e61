"""Consensus pose from descriptor matches over the C ABI (srrg2_consensus_*): the geometric verification that follows a descriptor
match -- K candidates x H minimal-sample hypotheses x N matches of transform-and-compare on the device, in one call.

The reference has no such step (its HBST detector hands raw matches to the locked solve, multi_loop_detector_hbst_impl.cpp:257-377).
Contract: include/srrg2_slam_amd.h and DESIGN.md section 4 "Consensus pose"; tests/consensus_restatement.py restates it and the
library gives the same bits.  There is no CPU fallback: without the library or a HIP device, construction raises.
"""
import ctypes as C

import numpy as np

from . import _abi as abi

CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
_RESULT_DTYPE = np.dtype(abi.ConsensusResult)
_COUNTERS = ("status", "best_hypothesis", "num_inliers", "num_pairs", "num_valid_pairs", "num_degenerate", "num_rejected",
             "num_scored", "cost_exponent", "cost")


def default_params():
    """srrg2_consensus_default_params: num_hypotheses 256, inlier_distance 0.05, min_sample_distance 0.1 (all three untuned),
    min_inliers 0, seed 0, length_check 1"""
    from . import _capi

    p = abi.ConsensusParams()
    _capi.lib().srrg2_consensus_default_params(C.byref(p))
    return p


def as_records(corr):
    """CORR_DTYPE records, C-contiguous, from a structured array with those fields or a sequence of mappings"""
    if isinstance(corr, np.ndarray) and corr.dtype == CORR_DTYPE:
        return np.ascontiguousarray(corr)
    if isinstance(corr, np.ndarray) and corr.dtype.names:
        a = np.empty(len(corr), CORR_DTYPE)
        for f in CORR_DTYPE.names:
            a[f] = corr[f]
        return a
    return np.array([(int(c["fixed_idx"]), int(c["moving_idx"]), float(c["response"])) for c in corr], CORR_DTYPE)


class ConsensusVerifier:
    """``compute(fixed, movings, correspondences, **params)``: ``fixed`` is the query cloud, ``movings`` the K candidates' clouds
    (numpy (n, dim) / (n, 4) float32 arrays, or ``mapping.Scene``s -- all of them then, bound from their device arrays),
    ``correspondences`` K record arrays (fixed_idx = query point, moving_idx = point of the candidate's own cloud).  Returns one
    dict per candidate: ``moving_in_fixed`` (3 x 4, or 3 x 3 for dim 2), the counters of srrg2_consensus_result and ``inliers``
    (the best pose's inlier records in input order; empty unless status is CONSENSUS_FOUND)."""

    def __init__(self, dim=3, device=0, lib=None):
        if lib is None:
            from . import _capi

            lib = _capi.lib()
        self._lib = lib
        self.dim, self.device = int(dim), device
        self._h = C.c_void_p()
        self._check(lib.srrg2_consensus_create(C.c_int(self.dim), C.c_int(device), C.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    def close(self):
        if self._h:
            self._lib.srrg2_consensus_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self, **kw):
        p = default_params()
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[0], p.reserved[1] = int(v[0]), int(v[1])
            elif not hasattr(p, k):
                raise TypeError("ConsensusVerifier: unknown parameter %r" % k)
            else:
                setattr(p, k, v)
        return p

    def compute_raw(self, fixed_ptr, fixed_stride, num_fixed, moving_ptr, moving_stride, moving_offsets, mem, records, corr_offsets,
                    params, capacity=None, want_inliers=True):
        """the C call on pointers (integers or None); returns (results as a _RESULT_DTYPE array, inlier records received,
        inlier offsets)"""
        K = len(corr_offsets) - 1
        results = np.zeros(max(K, 1), _RESULT_DTYPE)
        cap = len(records) if capacity is None else int(capacity)
        inl = np.zeros(max(cap, 1), CORR_DTYPE)
        offs = np.zeros(K + 1, np.int64)
        moff = np.ascontiguousarray(moving_offsets, np.int32)
        coff = np.ascontiguousarray(corr_offsets, np.int32)
        self._check(self._lib.srrg2_consensus_compute(
            self._h, fixed_ptr, C.c_int(fixed_stride), C.c_int(num_fixed), C.c_int(K), moving_ptr, C.c_int(moving_stride),
            moff.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(mem), records.ctypes.data if len(records) else None,
            coff.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(params), results.ctypes.data, inl.ctypes.data if want_inliers else None,
            C.c_int64(cap), offs.ctypes.data_as(C.POINTER(C.c_int64))))
        got = min(int(offs[K]), cap) if want_inliers else 0
        return results[:K], inl[:got], offs

    def _unpack(self, results, inl, offs):
        out = []
        for k, r in enumerate(results):
            T = np.array(r["moving_in_fixed"], np.float32)
            d = {n: int(r[n]) for n in _COUNTERS}
            d["moving_in_fixed"] = T.reshape(3, 4) if self.dim == 3 else T[:9].reshape(3, 3)
            d["inliers"] = inl[int(offs[k]):int(offs[k + 1])].copy()
            out.append(d)
        return out

    @staticmethod
    def _is_scene(x):
        from .mapping import Scene

        return isinstance(x, Scene)

    def compute(self, fixed, movings, correspondences, **params):
        p = self.params(**params)
        movings = list(movings)
        recs = [as_records(c) for c in correspondences]
        if len(recs) != len(movings):
            raise ValueError("ConsensusVerifier.compute: one correspondence array per moving cloud")
        K = len(movings)
        coff = np.zeros(K + 1, np.int32)
        coff[1:] = np.cumsum([len(r) for r in recs])
        records = np.concatenate(recs) if recs else np.zeros(0, CORR_DTYPE)
        if self._is_scene(fixed) or any(self._is_scene(m) for m in movings):
            if not (self._is_scene(fixed) and all(self._is_scene(m) for m in movings)):
                raise ValueError("ConsensusVerifier.compute: scenes and host arrays cannot be mixed")
            return self._compute_scenes(fixed, movings, records, coff, p)
        f = self._cloud(fixed)
        ms = [self._cloud(m, f.shape[1]) for m in movings]
        moff = np.zeros(K + 1, np.int32)
        moff[1:] = np.cumsum([len(m) for m in ms])
        m = np.ascontiguousarray(np.concatenate(ms)) if ms else np.zeros((0, f.shape[1]), np.float32)
        return self._unpack(*self.compute_raw(f.ctypes.data if len(f) else None, f.strides[0], len(f), m.ctypes.data if len(m) else None,
                                              m.strides[0], moff, abi.MEM_HOST, records, coff, p))

    def _cloud(self, a, cols=None):
        a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] < self.dim:
            raise ValueError("ConsensusVerifier: clouds are (n, >= dim) float32 arrays")
        if cols is not None and a.shape[1] != cols:
            raise ValueError("ConsensusVerifier: the moving clouds need the fixed cloud's row width")
        return a

    def _compute_scenes(self, fixed, movings, records, coff, p):
        """device-resident clouds: the query scene's float4 array is the fixed cloud, the candidates' are concatenated device to
        device into one buffer for the call"""
        lib = self._lib
        lib.srrg2_amd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        lib.srrg2_amd_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.srrg2_amd_device_free.argtypes = [C.c_void_p]
        addr = lambda q: C.cast(q, C.c_void_p).value  # noqa: E731
        fp, _, nf = fixed.device_arrays()
        arrays = [m.device_arrays() for m in movings]
        moff = np.zeros(len(movings) + 1, np.int32)
        moff[1:] = np.cumsum([a[2] for a in arrays])
        buf = C.c_void_p()
        if lib.srrg2_amd_device_malloc(C.c_size_t(16 * max(int(moff[-1]), 1)), C.byref(buf)):
            raise RuntimeError("srrg2_amd_device_malloc failed")
        try:
            for k, (cp, _, n) in enumerate(arrays):
                if n and lib.srrg2_amd_memcpy(C.c_void_p(buf.value + 16 * int(moff[k])), C.c_void_p(addr(cp)), C.c_size_t(16 * n), 2, None):
                    raise RuntimeError("srrg2_amd_memcpy (device -> device) failed")
            return self._unpack(*self.compute_raw(addr(fp) if nf else None, 16, nf, buf.value if moff[-1] else None, 16, moff,
                                                  abi.MEM_DEVICE, records, coff, p))
        finally:
            lib.srrg2_amd_device_free(buf)
