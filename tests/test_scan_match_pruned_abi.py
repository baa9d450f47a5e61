"""CPU: the C surface of pruned scan matching -- exports, struct sizes against the ctypes mirrors, the default parameters, and
every refusal that needs no device: srrg2_gridmap_build_bounds, srrg2_gridmap_get_bounds and srrg2_gridmap_match_scans_pruned check
their parameters before their handle, so each of those is reachable here and must leave its destinations untouched (what needs a
handle is in tests/test_gpu_scan_match_pruned.py); no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4
NAMES = ("srrg2_gridmap_default_prune_params", "srrg2_gridmap_build_bounds", "srrg2_gridmap_get_bounds", "srrg2_gridmap_match_scans_pruned")
F = np.float32
NB = 1081


def _scan(**kw):
    p = abi.GridMapScanParams()
    _capi.lib().srrg2_gridmap_default_scan_params(C.byref(p))
    p.angle_min, p.angle_increment, p.num_beams = -2.35619, 4.71238 / 1080, NB
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _window(wx=14, wy=14, ht=12, step=0.0175):
    m = abi.GridMapMatchParams()
    m.half_window_x, m.half_window_y, m.half_steps_theta, m.theta_step = wx, wy, ht, step
    return m


def _prune(levels=4, limit=0):
    p = abi.GridMapPruneParams()
    p.num_levels, p.max_list_entries = levels, limit
    return p


class _Call:
    """one srrg2_gridmap_match_scans_pruned without a handle; results and statistics are filled with a pattern that must survive"""

    def __init__(self):
        self.res = (abi.GridMapMatchResult * 2)()
        self.stats = (abi.GridMapPruneStats * 2)()
        C.memset(self.res, 0x5a, C.sizeof(self.res))
        C.memset(self.stats, 0x5a, C.sizeof(self.stats))
        self.before = bytes(self.res), bytes(self.stats)

    def __call__(self, window, prune, scan=None, K=2, ranges=None, guesses=None, mem=abi.MEM_HOST, results=True, stats=True):
        scan = _scan() if scan is None else scan
        nb = max(scan.num_beams, 0)
        r = np.full(max(K, 0) * nb + 1, 1.0, F) if ranges is None else ranges
        t = np.tile(np.eye(3, dtype=F).reshape(-1), max(K, 0) + 1) if guesses is None else guesses
        rp = r.ctypes.data if isinstance(r, np.ndarray) else r
        tp = t.ctypes.data if isinstance(t, np.ndarray) else t
        rc = _capi.lib().srrg2_gridmap_match_scans_pruned(None, C.c_void_p(rp), K, C.c_void_p(tp), mem, C.byref(scan),
                                                          None if window is None else C.byref(window),
                                                          None if prune is None else C.byref(prune), self.res if results else None,
                                                          self.stats if stats else None)
        assert (bytes(self.res), bytes(self.stats)) == self.before
        return rc, _capi.lib().srrg2_amd_last_error()


def test_exports_struct_sizes_and_the_default_parameters():
    lib = _capi.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.srrg2_amd_abi_version() == 4 == abi.ABI_VERSION  # additions do not bump it
    assert C.sizeof(abi.GridMapPruneParams) == 8 and abi.GridMapPruneParams.max_list_entries.offset == 4
    assert C.sizeof(abi.GridMapPruneStats) == 72 and abi.GridMapPruneStats.num_evaluated.offset == 4
    assert abi.GridMapPruneStats.num_survivors.offset == 32 and abi.GridMapPruneStats.floor_score.offset == 60
    assert abi.GridMapPruneStats.fell_back.offset == 68
    p = _prune(-7, -7)
    lib.srrg2_gridmap_default_prune_params(C.byref(p))
    assert (p.num_levels, p.max_list_entries) == (4, 0)
    lib.srrg2_gridmap_default_prune_params(None)  # (a null pointer is left alone)


def test_build_and_get_bounds_refuse_their_parameters_before_their_handle():
    lib = _capi.lib()
    for levels in (0, -1, 7):
        assert lib.srrg2_gridmap_build_bounds(None, levels) == INVALID
        msg = lib.srrg2_amd_last_error()
        assert b"gridmap_build_bounds" in msg and b"num_levels" in msg and b"null handle" not in msg
    for levels in (1, 6):  # at their limits the parameters pass: only the handle is missing
        assert lib.srrg2_gridmap_build_bounds(None, levels) == INVALID and b"null handle" in lib.srrg2_amd_last_error()
    img = np.full((8, 8), 0xaa, np.uint8)
    for level, mem, word in ((1, 3, b"bad mem"), (0, abi.MEM_HOST, b"level"), (7, abi.MEM_HOST, b"level"), (1, abi.MEM_HOST, b"null handle"),
                             (6, abi.MEM_DEVICE, b"null handle")):
        assert lib.srrg2_gridmap_get_bounds(None, level, C.c_void_p(img.ctypes.data), 8, mem) == INVALID
        assert word in lib.srrg2_amd_last_error() and (img == 0xaa).all(), (level, mem)


def test_pruned_match_refuses_its_parameters_before_its_handle():
    nan, inf = float("nan"), float("inf")
    call = _Call()
    # what is new: the prune parameters
    rc, msg = call(_window(), None)
    assert rc == INVALID and b"null prune params" in msg
    for p, word in ((_prune(0), b"num_levels"), (_prune(7), b"num_levels"), (_prune(-1), b"num_levels"), (_prune(4, -1), b"max_list_entries")):
        rc, msg = call(_window(), p)
        assert rc == INVALID and b"gridmap_match_scans_pruned" in msg and word in msg and b"null handle" not in msg, msg
    # what srrg2_gridmap_match_scans refuses of the window, the scan model and the data
    for w in (_window(wx=-1), _window(wy=-1), _window(ht=-1), _window(step=nan), _window(step=0.0), _window(step=inf),
              _window(step=-0.01), _window(ht=1, step=-inf)):
        rc, msg = call(w, _prune())
        assert rc == INVALID and b"gridmap_match_scans_pruned" in msg and b"null handle" not in msg, msg
    rc, msg = call(None, _prune())
    assert rc == INVALID and b"null match params" in msg
    for kw in (dict(scan=_scan(num_beams=-1)), dict(scan=_scan(angle_increment=0.0)), dict(scan=_scan(angle_increment=nan)),
               dict(scan=_scan(angle_min=6.3)), dict(scan=_scan(num_beams=1442)), dict(scan=_scan(range_min=0.0)),
               dict(scan=_scan(range_max=0.01)), dict(scan=_scan(clear_beyond_max=2)), dict(K=-1), dict(mem=2), dict(mem=-1),
               dict(ranges=0), dict(guesses=0), dict(results=False)):
        rc, msg = call(_window(), _prune(), **kw)
        assert rc == INVALID and b"gridmap_match_scans_pruned" in msg and b"null handle" not in msg, (kw, msg)
    buf = np.zeros(16 + 4 * 2 * NB, np.uint8)
    for kw in (dict(ranges=buf.ctypes.data + 1), dict(guesses=buf.ctypes.data + 2)):
        rc, msg = call(_window(), _prune(), **kw)
        assert rc == INVALID and b"misaligned" in msg, kw
    for kw in (dict(guesses=0), dict(guesses=buf.ctypes.data + 2), dict(guesses=0, mem=abi.MEM_DEVICE)):
        rc, msg = call(_window(), _prune(), scan=_scan(num_beams=0), ranges=0, **kw)
        assert rc == INVALID and b"guesses" in msg and b"null handle" not in msg, (kw, msg)
    for w in (_window(32767, 32767, 0), _window(1000, 1000, 300), _window(2 ** 30, 0, 0), _window(0, 0, 2 ** 30)):
        rc, msg = call(w, _prune())
        assert rc == UNSUPPORTED and b"candidates" in msg, msg
    rc, msg = call(_window(0, 0, 10 ** 6), _prune())  # 2 x 1 081 x 2 000 001 end cells
    assert rc == UNSUPPORTED and b"rotations" in msg
    # at their limits the parameters pass: only the handle is missing
    for w, p, kw in ((_window(), _prune(1), {}), (_window(), _prune(6, 2 ** 31 - 1), {}), (_window(0, 0, 0, nan), _prune(), {}),
                     (_window(500, 500, 500), _prune(), dict(K=3)), (_window(), _prune(), dict(stats=False)),
                     (_window(), _prune(), dict(K=0, ranges=0, guesses=0, results=False, stats=False)),
                     (_window(), _prune(), dict(scan=_scan(num_beams=0), ranges=0)), (_window(), _prune(), dict(mem=abi.MEM_DEVICE))):
        rc, msg = call(w, p, **kw)
        assert rc == INVALID and b"null handle" in msg, (kw, msg)


def test_no_cpu_fallback_without_a_device():
    import srrg2_slam_interfaces_amd as pkg

    lib = _capi.lib()
    h = C.c_void_p()
    rc = lib.srrg2_gridmap_create(0, C.byref(h))
    if _capi.device_count() > 0:
        assert rc == 0 and h
    else:
        assert rc == NO_DEVICE and not h
        with pytest.raises(RuntimeError, match="no HIP device"):
            pkg.OccupancyGrid()
    # without a device there is no handle and nothing computes on the host (null handle); with one, a handle without a grid is refused
    word = b"no grid" if h else b"null handle"
    img = np.full((3, 3), 0xaa, np.uint8)
    assert lib.srrg2_gridmap_build_bounds(h, 2) == INVALID and word in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_get_bounds(h, 1, C.c_void_p(img.ctypes.data), 3, abi.MEM_HOST) == INVALID and word in lib.srrg2_amd_last_error()
    r, t = np.ones(4, F), np.eye(3, dtype=F)
    res, stats = abi.GridMapMatchResult(), abi.GridMapPruneStats()
    C.memset(C.byref(res), 0x5a, C.sizeof(res)), C.memset(C.byref(stats), 0x5a, C.sizeof(stats))
    before = bytes(res), bytes(stats)
    scan = _scan(num_beams=4, angle_increment=0.01)
    assert lib.srrg2_gridmap_match_scans_pruned(h, C.c_void_p(r.ctypes.data), 1, C.c_void_p(t.ctypes.data), abi.MEM_HOST, C.byref(scan),
                                                C.byref(_window(1, 1, 1)), C.byref(_prune(1)), C.byref(res), C.byref(stats)) == INVALID
    assert word in lib.srrg2_amd_last_error() and (bytes(res), bytes(stats)) == before and (img == 0xaa).all()
    assert lib.srrg2_gridmap_destroy(h) == 0
