"""CPU: the C ABI of the stereo-feature adaptor -- declared in include/srrg2_slam_amd.h, exported by the built library, mirrored
by ctypes structs of the right size, defaults as documented.  Needs no GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srrg2_adapt_default_stereo_params", "srrg2_adapt_stereo_features")


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls():
    h = _header()
    assert re.search(r"\bvoid\s+srrg2_adapt_default_stereo_params\s*\(", h)
    assert re.search(r"\bint\s+srrg2_adapt_stereo_features\s*\(", h)
    for name in ("srrg2_stereo_params", "srrg2_stereo_match", "srrg2_stereo_result"):
        assert re.search(r"\}\s*%s\s*;" % name, h), name
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


def test_header_says_which_defaults_are_untuned():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    for field in ("max_disparity", "max_distance"):
        assert re.search(r"int32_t\s+%s;[^\n]*untuned" % field, txt), field


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name
    assert lib.srrg2_amd_abi_version() == 4


def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    assert C.sizeof(abi.StereoParams) == 32 and C.sizeof(abi.StereoMatch) == 16 and C.sizeof(abi.StereoResult) == 32
    p = adaptors.default_stereo_params()
    assert (p.baseline, p.min_disparity, p.max_disparity, p.row_tolerance, p.max_distance, p.cross_check, p.subpixel,
            p.reserved) == (0.0, 1, 128, 1, 48, 1, 1, 0)
    q = abi.StereoParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))  # the defaults overwrite whatever the struct held
    _capi.lib().srrg2_adapt_default_stereo_params(C.byref(q))
    assert bytes(q) == bytes(p)
    _capi.lib().srrg2_adapt_default_stereo_params(None)  # (a null pointer is ignored)
    assert adaptors.MATCH_DTYPE.itemsize == C.sizeof(abi.StereoMatch)
    assert [adaptors.MATCH_DTYPE.fields[n][1] for n, _ in abi.StereoMatch._fields_] == [0, 4, 8, 12]


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """null handle: SRRG2_E_INVALID with a message, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    fp, cam, sp = adaptors.default_feature_params(), adaptors.default_depth_params(), adaptors.default_stereo_params()
    sp.baseline = 0.1
    assert lib.srrg2_adapt_stereo_features(None, None, 0, None, 0, 0, C.byref(cam), C.byref(fp), C.byref(sp), None, 0, None, 0,
                                           None) == -1
    assert b"adapt_stereo_features" in lib.srrg2_amd_last_error()
