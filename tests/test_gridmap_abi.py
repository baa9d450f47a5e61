"""CPU: the C surface of the occupancy grid -- exports, struct sizes against the ctypes mirrors, defaults, and every refusal that
needs no device: srrg2_gridmap_reset and srrg2_gridmap_integrate_scans check their parameters before their handle, so each of
those is reachable here (what needs a handle is in tests/test_gpu_gridmap.py); no CPU fallback."""
import ctypes as C
import math

import numpy as np
import pytest

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi

INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -4
NAMES = ("srrg2_gridmap_create", "srrg2_gridmap_destroy", "srrg2_gridmap_default_params", "srrg2_gridmap_default_scan_params",
         "srrg2_gridmap_reset", "srrg2_gridmap_integrate_scans", "srrg2_gridmap_get_counts", "srrg2_gridmap_device_arrays",
         "srrg2_gridmap_render", "srrg2_gridmap_to_scene")
F = np.float32


def _grid(**kw):
    p = abi.GridMapParams()
    _capi.lib().srrg2_gridmap_default_params(C.byref(p))
    p.rows, p.cols = 64, 48
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def _scan(**kw):
    p = abi.GridMapScanParams()
    _capi.lib().srrg2_gridmap_default_scan_params(C.byref(p))
    p.angle_min, p.angle_increment, p.num_beams = -2.35619, 4.71238 / 1080, 1081
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def test_exports_struct_sizes_and_defaults():
    lib = _capi.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert lib.srrg2_amd_abi_version() == 4 == abi.ABI_VERSION  # additions do not bump it
    assert C.sizeof(abi.GridMapParams) == 20 and C.sizeof(abi.GridMapScanParams) == 72 and C.sizeof(abi.GridMapResult) == 48
    assert abi.GridMapScanParams.sensor_in_robot.offset == 28 and abi.GridMapScanParams.clear_beyond_max.offset == 64
    p = abi.GridMapParams()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    lib.srrg2_gridmap_default_params(C.byref(p))
    assert (p.rows, p.cols, list(p.origin)) == (0, 0, [0.0, 0.0]) and p.resolution == F(0.05)
    s = abi.GridMapScanParams()
    C.memset(C.byref(s), 0xff, C.sizeof(s))
    lib.srrg2_gridmap_default_scan_params(C.byref(s))
    assert (s.angle_min, s.angle_increment, s.num_beams, s.clear_beyond_max) == (0.0, 0.0, 0, 1)
    assert s.range_min == F(0.05) and s.range_max == 30.0 and list(s.sensor_in_robot) == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    lib.srrg2_gridmap_default_params(None)  # (a null pointer is ignored)
    lib.srrg2_gridmap_default_scan_params(None)
    assert lib.srrg2_gridmap_destroy(None) == 0


def test_reset_refuses_its_parameters_before_its_handle():
    lib = _capi.lib()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(rows=-1), dict(cols=-1), dict(rows=32769), dict(cols=32769), dict(resolution=0.0), dict(resolution=-0.05),
               dict(resolution=nan), dict(resolution=inf), dict(origin=(0, nan)), dict(origin=(1, inf)), dict(origin=(1, -inf))):
        assert lib.srrg2_gridmap_reset(None, C.byref(_grid(**kw))) == INVALID, kw
        msg = lib.srrg2_amd_last_error()
        assert b"gridmap_reset" in msg and b"null handle" not in msg, (kw, msg)
    # at their limits the parameters pass: only the handle is missing
    for kw in (dict(), dict(rows=0), dict(rows=0, cols=0), dict(rows=32768, cols=32768), dict(resolution=1e-6), dict(origin=(0, -1e9))):
        assert lib.srrg2_gridmap_reset(None, C.byref(_grid(**kw))) == INVALID, kw
        assert b"null handle" in lib.srrg2_amd_last_error(), kw
    assert lib.srrg2_gridmap_reset(None, None) == INVALID and b"null params" in lib.srrg2_amd_last_error()


def _integrate(p, ranges=None, K=2, poses=None, mem=abi.MEM_HOST, weight=1, out=None):
    lib = _capi.lib()
    nb = max(p.num_beams, 0) if p is not None else 0
    r = np.full(max(K, 0) * nb + 1, 1.0, F) if ranges is None else ranges
    t = np.tile(np.eye(3, dtype=F).reshape(-1), max(K, 0) + 1) if poses is None else poses
    rp = r.ctypes.data if isinstance(r, np.ndarray) else r
    tp = t.ctypes.data if isinstance(t, np.ndarray) else t
    return lib.srrg2_gridmap_integrate_scans(None, C.c_void_p(rp), K, C.c_void_p(tp), mem, None if p is None else C.byref(p), weight,
                                             None if out is None else C.byref(out))


def test_integrate_refuses_its_parameters_before_its_handle():
    lib = _capi.lib()
    nan, inf, two_pi = float("nan"), float("inf"), 2 * math.pi
    out = abi.GridMapResult()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    before = bytes(out)
    calls = [dict(weight=0), dict(weight=2), dict(weight=-2), dict(K=-1), dict(mem=2), dict(mem=7), dict(mem=-1), dict(ranges=0),
             dict(poses=0)]
    scans = [dict(num_beams=-1), dict(clear_beyond_max=2), dict(clear_beyond_max=-1), dict(angle_increment=0.0),
             dict(angle_increment=nan), dict(angle_increment=inf), dict(angle_min=nan), dict(angle_min=inf), dict(angle_min=6.3),
             dict(angle_min=-6.3), dict(num_beams=1442), dict(angle_increment=-4.71238 / 1080, num_beams=1442),
             dict(range_min=0.0), dict(range_min=-1.0), dict(range_min=nan), dict(range_max=0.01), dict(range_max=nan)] + \
            [dict(sensor_in_robot=(i, v)) for i in range(9) for v in (nan, inf)]
    for kw, skw in [(kw, {}) for kw in calls] + [({}, skw) for skw in scans]:
        assert _integrate(_scan(**skw), out=out, **kw) == INVALID, (kw, skw)
        msg = lib.srrg2_amd_last_error()
        assert b"gridmap_integrate_scans" in msg and b"null handle" not in msg, (kw, skw, msg)
        assert bytes(out) == before
    # misaligned data
    buf = np.zeros(16 + 4 * 2 * 1081, np.uint8)
    assert _integrate(_scan(), ranges=buf.ctypes.data + 1, out=out) == INVALID and b"misaligned" in lib.srrg2_amd_last_error()
    assert _integrate(_scan(), poses=buf.ctypes.data + 2, out=out) == INVALID and b"misaligned" in lib.srrg2_amd_last_error()
    assert _integrate(None) == INVALID and b"null params" in lib.srrg2_amd_last_error()
    assert _integrate(_scan(num_beams=1081), K=2 * 10 ** 6) == UNSUPPORTED and b"int32" in lib.srrg2_amd_last_error()
    assert bytes(out) == before
    # at their limits the parameters pass: only the handle is missing
    for skw, kw in ((dict(), dict()), (dict(), dict(weight=-1)), (dict(num_beams=0), dict()), (dict(), dict(K=0, ranges=0, poses=0)),
                    (dict(num_beams=0), dict(ranges=0, poses=0)), (dict(angle_min=two_pi), dict()), (dict(num_beams=1441), dict()),
                    (dict(angle_min=math.pi, angle_increment=-two_pi / 360, num_beams=361), dict()),
                    (dict(range_min=1e-3, range_max=1e-3), dict()), (dict(range_max=inf), dict()), (dict(clear_beyond_max=0), dict()),
                    (dict(), dict(mem=abi.MEM_DEVICE))):
        assert _integrate(_scan(**skw), out=out, **kw) == INVALID, (skw, kw)
        assert b"null handle" in lib.srrg2_amd_last_error(), (skw, kw)
    assert bytes(out) == before


def test_reading_calls_refuse_a_null_handle_and_leave_the_destination():
    lib = _capi.lib()
    hits, misses = np.full(12, 7, np.int32), np.full(12, 9, np.int32)
    img = np.full((3, 4), 0xaa, np.uint8)
    i32 = C.POINTER(C.c_int32)
    a, b = i32(), i32()
    assert lib.srrg2_gridmap_get_counts(None, hits.ctypes.data, misses.ctypes.data, abi.MEM_HOST) == INVALID
    assert b"gridmap_get_counts" in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_get_counts(None, hits.ctypes.data, misses.ctypes.data, 5) == INVALID and b"bad mem" in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_device_arrays(None, C.byref(a), C.byref(b)) == INVALID and not a and not b
    assert lib.srrg2_gridmap_device_arrays(None, None, None) == INVALID
    assert lib.srrg2_gridmap_render(None, 1, img.ctypes.data, 4, abi.MEM_HOST) == INVALID and b"gridmap_render" in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_render(None, 1, img.ctypes.data, 4, 3) == INVALID and b"bad mem" in lib.srrg2_amd_last_error()
    for pct in (-1, 101):
        assert lib.srrg2_gridmap_to_scene(None, 1, pct, None) == INVALID and b"occupied_percent" in lib.srrg2_amd_last_error()
    assert lib.srrg2_gridmap_to_scene(None, 1, 50, None) == INVALID and b"null handle" in lib.srrg2_amd_last_error()
    assert (hits == 7).all() and (misses == 9).all() and (img == 0xaa).all()
    assert lib.srrg2_gridmap_create(0, None) == INVALID


def test_no_cpu_fallback_without_a_device():
    lib = _capi.lib()
    h = C.c_void_p()
    rc_ = lib.srrg2_gridmap_create(0, C.byref(h))
    said = lib.srrg2_amd_last_error()
    if _capi.device_count() > 0:
        assert rc_ == 0 and h
        assert lib.srrg2_gridmap_create(-1, C.byref(C.c_void_p())) == INVALID
        assert lib.srrg2_gridmap_destroy(h) == 0
    else:
        assert rc_ == NO_DEVICE and not h and b"no HIP device" in said
        import srrg2_slam_interfaces_amd as pkg

        with pytest.raises(RuntimeError, match="no HIP device"):
            pkg.OccupancyGrid()
