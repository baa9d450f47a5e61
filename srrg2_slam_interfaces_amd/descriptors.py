"""Device-resident database of 256-bit binary descriptors with exact matching over the C ABI (srrg2_descriptor_db_*):
the matching half of MultiLoopDetectorHBST_ (S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:41-197).

The reference keeps an srrg_hbst::BinaryTree256<uint64_t> (multi_loop_detector_hbst.h:40-44); this database is that
tree with a single leaf, searched exhaustively on the GPU, so it finds every match within the distance threshold.
Semantics (include/srrg2_slam_amd.h, DESIGN.md section 5 "Descriptor matching"):
  - a descriptor is a row of 32 bytes; ``valid`` marks the points whose status is Valid (None = all).  Indices are
    point indices of the caller's arrays, never compacted.
  - ``add`` appends the valid descriptors of one local map and returns its database index (-1: nothing valid, not added).
  - ``match`` returns the candidate maps (age gate, count gate) with their deduplicated correspondences.
  - ``add_scene`` / ``match_scene`` are ``add`` / ``match`` fed on the device with the descriptors of a ``mapping.Scene``
    that carries them and valid = the points with finite coordinates.
There is no CPU fallback: without the library or a HIP device, construction raises.
"""
import ctypes as C
import math

import numpy as np

CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
DESCRIPTOR_BYTES = 32


def as_descriptors(descriptors):
    """(n, 32) uint8 rows, C-contiguous (any array whose rows are 32 bytes, e.g. (n, 4) uint64, is viewed as such)."""
    a = np.ascontiguousarray(descriptors)
    if a.ndim != 2 or a.shape[1] * a.dtype.itemsize != DESCRIPTOR_BYTES:
        raise ValueError("descriptors: expected an (n, 32) uint8 array (256-bit rows), got %s %s" % (a.shape, a.dtype))
    if a.dtype.kind not in "uib":
        raise ValueError("descriptors: integer rows expected, got %s" % a.dtype)
    return a.view(np.uint8).reshape(a.shape[0], DESCRIPTOR_BYTES)


def as_valid(valid, n):
    """None (all valid) or n bytes, nonzero = POINT_STATUS::Valid"""
    if valid is None:
        return None
    v = np.ascontiguousarray(valid)
    if v.shape != (n,):
        raise ValueError("valid: expected %d entries, got shape %s" % (n, v.shape))
    return (v != 0).astype(np.uint8)


def check_match_args(max_distance, min_age, min_matches, query_index=0):
    if math.isnan(float(max_distance)):
        raise ValueError("maximum_descriptor_distance is NaN")
    if not 0 <= int(min_age) < 2 ** 32:
        raise ValueError("minimum_age_difference_to_candidates must fit an unsigned 32-bit integer")
    if int(min_matches) < 0:
        raise ValueError("min_matches must be >= 0")
    if int(query_index) < 0:
        raise ValueError("query_index must be >= 0")


def _u8p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


class MatchResult:
    """What one match() found.  ``indices``: candidate database indices, ascending; ``num_matches``: their pair counts
    before deduplication; ``correspondences[k]``: candidate k's correspondences (CORR_DTYPE, ascending in moving_idx);
    ``map_counts``: the pair count of every map, -1 for maps the age gate skipped."""

    def __init__(self, indices, num_matches, correspondences, map_counts, device_ms):
        self.indices = indices
        self.num_matches = num_matches
        self.correspondences = correspondences
        self.map_counts = map_counts
        self.device_ms = device_ms

    def __len__(self):
        return len(self.indices)


class DescriptorDatabase:
    def __init__(self, device=0, lib=None):
        if lib is None:
            from . import _capi

            lib = _capi.lib()
        self._lib = lib
        self.device = device
        self._h = C.c_void_p()
        self._check(lib.srrg2_descriptor_db_create(C.c_int(device), C.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.srrg2_amd_last_error()
            raise RuntimeError("%s (code %d)" % (msg.decode() if msg else "", rc))

    def close(self):
        if self._h:
            self._lib.srrg2_descriptor_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        """(number of maps, number of descriptors)"""
        m, d = C.c_int(), C.c_int64()
        self._check(self._lib.srrg2_descriptor_db_size(self._h, C.byref(m), C.byref(d)))
        return m.value, d.value

    def __len__(self):
        return self.size()[0]

    def add(self, descriptors, valid=None):
        """Append one local map (its valid descriptors); returns its database index, or -1 when nothing is valid."""
        d = as_descriptors(descriptors)
        v = as_valid(valid, len(d))
        idx = C.c_int(-1)
        self._check(self._lib.srrg2_descriptor_db_add(self._h, _u8p(d), _u8p(v), C.c_int(len(d)), C.byref(idx)))
        return idx.value

    def _scene_handle(self, scene):
        if getattr(scene, "_b", None) is None or scene._b.lib is not self._lib:
            raise ValueError("add_scene / match_scene need a Scene of the HIP library (mapping.Scene on scene_binding())")
        return scene._h

    def add_scene(self, scene):
        """add() with the descriptors of ``scene`` (Scene.set_features) read on the device; valid = finite coordinates."""
        idx = C.c_int(-1)
        self._check(self._lib.srrg2_descriptor_db_add_scene(self._h, self._scene_handle(scene), C.byref(idx)))
        return idx.value

    def match_scene(self, scene, query_index=None, max_distance=25.0, min_age=0, min_matches=0):
        """match() with the descriptors of ``scene`` read on the device; fixed_idx are the scene's point indices."""
        if query_index is None:
            query_index = self.size()[0]
        check_match_args(max_distance, min_age, min_matches, query_index)
        K = C.c_int(0)
        self._check(self._lib.srrg2_descriptor_db_match_scene(self._h, self._scene_handle(scene), C.c_int64(int(query_index)),
                                                              C.c_float(max_distance), C.c_uint32(int(min_age)),
                                                              C.c_int64(int(min_matches)), C.byref(K)))
        return self._result(K.value)

    def match(self, descriptors, valid=None, query_index=None, max_distance=25.0, min_age=0, min_matches=0):
        """query_index: the query map's database index (None: a new map, index = number of maps)."""
        d = as_descriptors(descriptors)
        v = as_valid(valid, len(d))
        if query_index is None:
            query_index = self.size()[0]
        check_match_args(max_distance, min_age, min_matches, query_index)
        K = C.c_int(0)
        self._check(self._lib.srrg2_descriptor_db_match(self._h, _u8p(d), _u8p(v), C.c_int(len(d)),
                                                        C.c_int64(int(query_index)), C.c_float(max_distance),
                                                        C.c_uint32(int(min_age)), C.c_int64(int(min_matches)),
                                                        C.byref(K)))
        return self._result(K.value)

    def _result(self, K):
        """the getters after a match"""
        ref = np.zeros(K, np.int32)
        cnt = np.zeros(K, np.int64)
        off = np.zeros(K + 1, np.int64)
        n = C.c_int(K)
        self._check(self._lib.srrg2_descriptor_db_get_candidates(
            self._h, ref.ctypes.data_as(C.POINTER(C.c_int32)), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
            off.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
        total = C.c_int64(int(off[-1]))
        corr = np.zeros(int(off[-1]), CORR_DTYPE)
        self._check(self._lib.srrg2_descriptor_db_get_correspondences(self._h, C.c_void_p(corr.ctypes.data),
                                                                      C.byref(total)))
        nm = C.c_int(0)
        self._check(self._lib.srrg2_descriptor_db_get_map_counts(self._h, None, C.byref(nm)))
        counts = np.zeros(nm.value, np.int64)
        self._check(self._lib.srrg2_descriptor_db_get_map_counts(self._h, counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                                                 C.byref(nm)))
        ms = C.c_double(0.0)
        self._check(self._lib.srrg2_descriptor_db_last_match_ms(self._h, C.byref(ms)))
        return MatchResult(ref, cnt, [corr[off[k]:off[k + 1]] for k in range(K)], counts, ms.value)
