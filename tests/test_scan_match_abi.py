"""CPU: the C surface of correlative scan matching -- exports, struct sizes against the ctypes mirrors, the default table bit for
bit against its formula, and every refusal that needs no device: srrg2_gridmap_build_likelihood and srrg2_gridmap_match_scans
check their parameters before their handle, so each of those is reachable here and must leave its destinations untouched (what
needs a handle is in tests/test_gpu_scan_match.py); no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4
NAMES = ("srrg2_gridmap_default_likelihood_lut", "srrg2_gridmap_build_likelihood", "srrg2_gridmap_get_likelihood",
         "srrg2_gridmap_match_scans")
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


class _Call:
    """one srrg2_gridmap_match_scans without a handle; results and volume are filled with a pattern that must survive"""

    def __init__(self):
        self.res = (abi.GridMapMatchResult * 2)()
        C.memset(self.res, 0x5a, C.sizeof(self.res))
        self.vol = np.full(64, 0x5a5a5a5a, np.int32)
        self.before = bytes(self.res)

    def __call__(self, window, scan=None, K=2, ranges=None, guesses=None, mem=abi.MEM_HOST, results=True, scores=False,
                 scores_mem=abi.MEM_HOST):
        scan = _scan() if scan is None else scan
        nb = max(scan.num_beams, 0)
        r = np.full(max(K, 0) * nb + 1, 1.0, F) if ranges is None else ranges
        t = np.tile(np.eye(3, dtype=F).reshape(-1), max(K, 0) + 1) if guesses is None else guesses
        rp = r.ctypes.data if isinstance(r, np.ndarray) else r
        tp = t.ctypes.data if isinstance(t, np.ndarray) else t
        sp = None if scores is False else C.c_void_p(self.vol.ctypes.data if scores is True else scores)
        rc = _capi.lib().srrg2_gridmap_match_scans(None, C.c_void_p(rp), K, C.c_void_p(tp), mem, C.byref(scan),
                                                   None if window is None else C.byref(window), self.res if results else None, sp,
                                                   scores_mem)
        assert bytes(self.res) == self.before and (self.vol == 0x5a5a5a5a).all()
        return rc, _capi.lib().srrg2_amd_last_error()


def test_exports_struct_sizes_and_the_default_table():
    lib = _capi.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.srrg2_amd_abi_version() == 4 == abi.ABI_VERSION  # additions do not bump it
    assert C.sizeof(abi.GridMapMatchParams) == 24 and abi.GridMapMatchParams.theta_step.offset == 16
    assert C.sizeof(abi.GridMapMatchResult) == 60 and abi.GridMapMatchResult.dx.offset == 36
    assert abi.GridMapMatchResult.num_scored_beams.offset == 56
    for R in range(17):
        n = R * R + 1
        lut = np.full(n + 2, 0xaa, np.uint8)
        assert lib.srrg2_gridmap_default_likelihood_lut(R, C.c_void_p(lut.ctypes.data)) == 0
        assert list(lut[:n]) == [(255 * (n - d2)) // n for d2 in range(n)] and lut[0] == 255 and list(lut[n:]) == [0xaa, 0xaa]
    lut = np.full(300, 0xaa, np.uint8)
    for R in (-1, 17):
        assert lib.srrg2_gridmap_default_likelihood_lut(R, C.c_void_p(lut.ctypes.data)) == INVALID
    assert lib.srrg2_gridmap_default_likelihood_lut(4, None) == INVALID and (lut == 0xaa).all()
    from srrg2_slam_interfaces_amd import gridmap

    assert list(gridmap.default_likelihood_lut(4)) == [(255 * (17 - d2)) // 17 for d2 in range(17)]


def test_build_and_get_likelihood_refuse_their_parameters_before_their_handle():
    lib = _capi.lib()
    lut = np.zeros(257, np.uint8)
    for args, word in (((1, 50, -1), b"radius"), ((1, 50, 17), b"radius"), ((1, -1, 4), b"occupied_percent"), ((1, 101, 4), b"occupied_percent")):
        assert lib.srrg2_gridmap_build_likelihood(None, *args, C.c_void_p(lut.ctypes.data)) == INVALID, args
        msg = lib.srrg2_amd_last_error()
        assert b"gridmap_build_likelihood" in msg and word in msg and b"null handle" not in msg
    assert lib.srrg2_gridmap_build_likelihood(None, 1, 50, 4, None) == INVALID and b"null lut" in lib.srrg2_amd_last_error()
    for args in ((1, 50, 0), (1, 0, 16), (0, 100, 4)):  # at their limits the parameters pass: only the handle is missing
        assert lib.srrg2_gridmap_build_likelihood(None, *args, C.c_void_p(lut.ctypes.data)) == INVALID
        assert b"null handle" in lib.srrg2_amd_last_error(), args
    img = np.full((3, 4), 0xaa, np.uint8)
    assert lib.srrg2_gridmap_get_likelihood(None, C.c_void_p(img.ctypes.data), 4, 3) == INVALID and b"bad mem" in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_get_likelihood(None, C.c_void_p(img.ctypes.data), 4, abi.MEM_HOST) == INVALID
    assert b"null handle" in lib.srrg2_amd_last_error() and (img == 0xaa).all()


def test_match_refuses_its_parameters_before_its_handle():
    nan, inf = float("nan"), float("inf")
    call = _Call()
    for w in (_window(wx=-1), _window(wy=-1), _window(ht=-1), _window(step=nan), _window(step=0.0), _window(step=inf),
              _window(step=-0.01), _window(ht=1, step=-inf)):
        rc, msg = call(w, scores=True)
        assert rc == INVALID and b"gridmap_match_scans" in msg and b"null handle" not in msg, msg
    rc, msg = call(None)
    assert rc == INVALID and b"null match params" in msg
    # the scan model and the data, as srrg2_gridmap_integrate_scans refuses them
    for kw in (dict(scan=_scan(num_beams=-1)), dict(scan=_scan(angle_increment=0.0)), dict(scan=_scan(angle_increment=nan)),
               dict(scan=_scan(angle_min=6.3)), dict(scan=_scan(num_beams=1442)), dict(scan=_scan(range_min=0.0)),
               dict(scan=_scan(range_max=0.01)), dict(scan=_scan(clear_beyond_max=2)), dict(K=-1), dict(mem=2), dict(mem=-1),
               dict(ranges=0), dict(guesses=0), dict(results=False), dict(scores=True, scores_mem=2), dict(scores=True, scores_mem=-1)):
        rc, msg = call(_window(), **kw)
        assert rc == INVALID and b"gridmap_match_scans" in msg and b"null handle" not in msg, (kw, msg)
    buf = np.zeros(16 + 4 * 2 * NB, np.uint8)
    for kw in (dict(ranges=buf.ctypes.data + 1), dict(guesses=buf.ctypes.data + 2), dict(scores=call.vol.ctypes.data + 2)):
        rc, msg = call(_window(), **kw)
        assert rc == INVALID and b"misaligned" in msg, kw
    # a scan without beams still gets its guess back: the guesses are read, so they are checked whatever num_beams is
    for kw in (dict(guesses=0), dict(guesses=buf.ctypes.data + 2), dict(guesses=0, mem=abi.MEM_DEVICE)):
        rc, msg = call(_window(), scan=_scan(num_beams=0), ranges=0, scores=True, **kw)
        assert rc == INVALID and b"guesses" in msg and b"null handle" not in msg, (kw, msg)
    # the overflows: candidates per scan, the volume, the end cells
    for w in (_window(32767, 32767, 0), _window(1000, 1000, 300), _window(2 ** 30, 0, 0), _window(0, 0, 2 ** 30)):
        rc, msg = call(w, scores=True)
        assert rc == UNSUPPORTED and b"candidates" in msg, msg
    rc, msg = call(_window(500, 500, 500), K=3, scores=True)  # 1 001^3 fits, three of them do not
    assert rc == UNSUPPORTED and b"volume" in msg
    rc, msg = call(_window(0, 0, 10 ** 6))  # 2 x 1 081 x 2 000 001 end cells
    assert rc == UNSUPPORTED and b"rotations" in msg
    rc, msg = call(_window(), K=2 * 10 ** 6, ranges=buf.ctypes.data, guesses=buf.ctypes.data)  # (refused before anything is read)
    assert rc == UNSUPPORTED and b"int32" in msg
    # at their limits the parameters pass: only the handle is missing
    for w, kw in ((_window(), {}), (_window(0, 0, 0, nan), {}), (_window(0, 0, 0, 0.0), {}), (_window(0, 0, 0, -inf), {}),
                  (_window(500, 500, 500), dict(K=2, scores=True)), (_window(500, 500, 500), dict(K=3)), (_window(23169, 23169, 0, 0.0), {}),
                  (_window(), dict(K=0, ranges=0, guesses=0, results=False)), (_window(), dict(scan=_scan(num_beams=0), ranges=0)),
                  (_window(), dict(mem=abi.MEM_DEVICE, scores=True, scores_mem=abi.MEM_DEVICE)), (_window(1, 1, 1, 1e-9), {})):
        rc, msg = call(w, **kw)
        assert rc == INVALID and b"null handle" in msg, (kw, msg)


def test_no_cpu_fallback_without_a_device():
    import srrg2_slam_interfaces_amd as pkg

    lib = _capi.lib()
    h = C.c_void_p()
    rc = lib.srrg2_gridmap_create(0, C.byref(h))
    said = lib.srrg2_amd_last_error()
    if _capi.device_count() > 0:
        assert rc == 0 and h
    else:
        assert rc == NO_DEVICE and not h and b"no HIP device" in said
        with pytest.raises(RuntimeError, match="no HIP device"):
            pkg.OccupancyGrid()
    # the new entry points on what create left: without a device there is no handle and nothing computes on the host (null
    # handle); with one, a handle without a grid is refused
    word = b"no grid" if h else b"null handle"
    lut, img = np.zeros(17, np.uint8), np.full((2, 2), 0xaa, np.uint8)
    assert lib.srrg2_gridmap_build_likelihood(h, 1, 50, 4, C.c_void_p(lut.ctypes.data)) == INVALID and word in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_get_likelihood(h, C.c_void_p(img.ctypes.data), 2, abi.MEM_HOST) == INVALID and word in lib.srrg2_amd_last_error()
    r, t = np.ones(4, F), np.eye(3, dtype=F)
    res = abi.GridMapMatchResult()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    before = bytes(res)
    scan = _scan(num_beams=4, angle_increment=0.01)
    assert lib.srrg2_gridmap_match_scans(h, C.c_void_p(r.ctypes.data), 1, C.c_void_p(t.ctypes.data), abi.MEM_HOST, C.byref(scan),
                                         C.byref(_window(1, 1, 1)), C.byref(res), None, abi.MEM_HOST) == INVALID
    assert word in lib.srrg2_amd_last_error() and bytes(res) == before and (img == 0xaa).all()
    assert lib.srrg2_gridmap_destroy(h) == 0
