"""CPU: the C ABI of the lidar sweep adaptor and the spherical clipper -- declared in include/srrg2_slam_amd.h, exported by the
built library, mirrored by ctypes structs of the right size, defaults as documented, the full-turn helper against float64
arithmetic done here.  Needs no GPU."""
import ctypes as C
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srrg2_adapt_lidar_sweep", "srrg2_scene_clip_spherical", "srrg2_spherical_model_full_turn")
DEFAULTS = ("srrg2_adapt_default_lidar_params", "srrg2_clip_default_spherical_params")


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls():
    h = _header()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    for name in DEFAULTS:
        assert re.search(r"\bvoid\s+%s\s*\(" % name, h), name
    for struct in ("srrg2_spherical_model", "srrg2_lidar_adaptor_params", "srrg2_spherical_clip_params"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, h), struct
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for name in CALLS + DEFAULTS:
        assert hasattr(lib, name), name
    assert lib.srrg2_amd_abi_version() == 4


def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors, mapping

    assert C.sizeof(abi.SphericalModel) == 48 and C.sizeof(abi.LidarAdaptorParams) == 72
    assert C.sizeof(abi.SphericalClipParams) == 104
    assert mapping.SphericalClipParams is abi.SphericalClipParams and mapping.SphericalModel is abi.SphericalModel
    lib = _capi.lib()
    p = adaptors.default_lidar_params()
    m = p.model
    assert (m.azimuth_min, m.azimuth_increment, m.elevation_min, m.elevation_increment, m.rows, m.cols) == (0, 0, 0, 0, 0, 0)
    assert (m.range_min, m.range_max) == (0.5, 120.0)
    assert (p.normal_col_gap, p.normal_row_gap, p.normal_max_distance_squared) == (1, 1, 1.0)
    assert (p.drop_points_without_normal, p.compact, p.reserved) == (1, 0, 0)
    c = mapping.default_spherical_clip_params()
    assert (c.model.range_min, c.model.range_max, c.model.rows, c.model.cols) == (0.5, 120.0, 0, 0)
    assert list(c.sensor_in_robot) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and c.occlusion_margin == -1.0 and c.reserved == 0
    # the defaults overwrite whatever the struct held
    q = abi.LidarAdaptorParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))
    lib.srrg2_adapt_default_lidar_params(C.byref(q))
    assert bytes(q) == bytes(p)
    d = abi.SphericalClipParams()
    C.memset(C.byref(d), 0xFF, C.sizeof(d))
    lib.srrg2_clip_default_spherical_params(C.byref(d))
    assert bytes(d) == bytes(c)
    lib.srrg2_adapt_default_lidar_params(None)  # (a null pointer is ignored)
    lib.srrg2_clip_default_spherical_params(None)


def test_full_turn_model_against_float64():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    for rows, cols, first, last in ((16, 360, math.radians(-15), math.radians(15)), (64, 2048, math.radians(2), math.radians(-24.8)),
                                    (2, 1, -0.1, 0.1), (32, 1024, -math.pi / 2, math.pi / 2)):
        m = abi.SphericalModel()
        C.memset(C.byref(m), 0xFF, C.sizeof(m))
        assert lib.srrg2_spherical_model_full_turn(C.byref(m), rows, cols, first, last) == 0
        assert m.azimuth_increment == (2.0 * math.pi) / cols and m.azimuth_min == -math.pi + math.pi / cols
        assert m.elevation_min == first and m.elevation_increment == (last - first) / (rows - 1)
        assert (m.rows, m.cols, m.range_min, m.range_max) == (rows, cols, 0.5, 120.0)
        w = adaptors.spherical_model_full_turn(rows, cols, first, last)
        assert bytes(w) == bytes(m)
        # the columns tile [-pi, pi): the last one ends half an increment past its centre, at +pi
        assert abs(m.azimuth_min + (cols - 0.5) * m.azimuth_increment - math.pi) < 1e-12
    keep = abi.SphericalModel()
    C.memset(C.byref(keep), 0x5A, C.sizeof(keep))
    before = bytes(keep)
    for rows, cols, first, last in ((1, 8, -0.1, 0.1), (4, 0, -0.1, 0.1), (4, 8, float("nan"), 0.1), (4, 8, 0.1, float("inf")),
                                    (4, 8, 0.2, 0.2)):
        assert lib.srrg2_spherical_model_full_turn(C.byref(keep), rows, cols, first, last) == -1, (rows, cols, first, last)
        assert b"spherical_model_full_turn" in lib.srrg2_amd_last_error() and bytes(keep) == before
    assert lib.srrg2_spherical_model_full_turn(None, 4, 8, -0.1, 0.1) == -1
    import pytest

    with pytest.raises(ValueError, match="full_turn"):
        adaptors.spherical_model_full_turn(1, 8, -0.1, 0.1)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """null handles and params: SRRG2_E_INVALID with a message naming the call, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, adaptors, mapping

    lib = _capi.lib()
    p = adaptors.default_lidar_params()
    assert lib.srrg2_adapt_lidar_sweep(None, None, 12, None, 0, 0, 0, C.byref(p), None) == -1
    assert b"adapt_lidar_sweep" in lib.srrg2_amd_last_error()
    c = mapping.default_spherical_clip_params()
    assert lib.srrg2_scene_clip_spherical(None, None, C.byref(c), None, None) == -1
    assert b"scene_clip_spherical" in lib.srrg2_amd_last_error()
