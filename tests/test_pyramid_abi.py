"""CPU: the C ABI of the scale-pyramid feature adaptor -- declared in include/srrg2_slam_amd.h, exported by the built library,
mirrored by ctypes structs of the right size, defaults as documented, bad arguments refused before a device is touched.  Needs no
GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srrg2_adapt_default_pyramid_params", "srrg2_adapt_image_features_pyramid")


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls():
    h = _header()
    assert re.search(r"\bvoid\s+srrg2_adapt_default_pyramid_params\s*\(", h)
    assert re.search(r"\bint\s+srrg2_adapt_image_features_pyramid\s*\(", h)
    for name in ("srrg2_pyramid_params", "srrg2_pyramid_keypoint", "srrg2_pyramid_result"):
        assert re.search(r"\}\s*%s\s*;" % name, h), name
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h  # append-only: the version stays


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name
    assert lib.srrg2_amd_abi_version() == 4


def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    assert C.sizeof(abi.PyramidParams) == 16 and C.sizeof(abi.PyramidKeypoint) == 32
    assert C.sizeof(abi.PyramidResult) == 4 * 4 + 7 * 8 * 4 and adaptors.PYRAMID_KEYPOINT_DTYPE.itemsize == 32
    assert [n for n, _ in abi.PyramidKeypoint._fields_] == ["pixel", "score", "angle_bin", "level", "level_pixel", "u_q8", "v_q8",
                                                           "reserved"]
    p = adaptors.default_pyramid_params()
    assert (p.num_levels, p.scale_num, p.scale_den, p.reserved) == (4, 6, 5, 0)
    q = abi.PyramidParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))  # the defaults overwrite whatever the struct held
    _capi.lib().srrg2_adapt_default_pyramid_params(C.byref(q))
    assert bytes(q) == bytes(p)
    _capi.lib().srrg2_adapt_default_pyramid_params(None)  # (a null pointer is ignored)
    r = abi.PyramidResult()
    r.num_levels_built, r.rows[0], r.rows[1], r.quota[1] = 2, 48, 40, 9
    assert r.as_dict()["rows"] == [48, 40] and r.as_dict()["quota"] == [0, 9] and r.as_dict()["num_levels_built"] == 2


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """a null handle, null params: SRRG2_E_INVALID with the call's name in the message, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    p, cam, pyr = adaptors.default_feature_params(), adaptors.default_depth_params(), adaptors.default_pyramid_params()
    call = lib.srrg2_adapt_image_features_pyramid
    assert call(None, None, 1, 0, None, 0, 0, 0, C.byref(cam), C.byref(p), C.byref(pyr), None, 0, None) == -1
    assert b"adapt_image_features_pyramid" in lib.srrg2_amd_last_error()


def test_python_adaptor_is_the_plain_one_with_a_pyramid():
    from srrg2_slam_interfaces_amd import adaptors
    import srrg2_slam_interfaces_amd as pkg

    ad = pkg.MeasurementAdaptorImageFeaturesPyramid()
    assert isinstance(ad, adaptors.MeasurementAdaptorImageFeatures) and ad.pyramid.num_levels == 4
    assert ad.keypoints().dtype == adaptors.PYRAMID_KEYPOINT_DTYPE and len(ad.keypoints()) == 0
