"""CPU: the C ABI of the image-feature adaptor -- declared in include/srrg2_slam_amd.h, exported by the built library, mirrored
by ctypes structs of the right size, defaults as documented, the pattern as the restatement generates it.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srrg2_adapt_default_feature_params", "srrg2_adapt_image_features", "srrg2_feature_pattern")


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls():
    h = _header()
    assert re.search(r"\bvoid\s+srrg2_adapt_default_feature_params\s*\(", h)
    assert re.search(r"\bint\s+srrg2_adapt_image_features\s*\(", h)
    assert re.search(r"\bint\s+srrg2_feature_pattern\s*\(", h)
    for name in ("srrg2_feature_params", "srrg2_keypoint", "srrg2_feature_result"):
        assert re.search(r"\}\s*%s\s*;" % name, h), name
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for name in CALLS:
        assert hasattr(lib, name), name
    assert lib.srrg2_amd_abi_version() == 4


def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    assert C.sizeof(abi.FeatureParams) == 16 and C.sizeof(abi.Keypoint) == 16 and C.sizeof(abi.FeatureResult) == 28
    p = adaptors.default_feature_params()
    assert (p.fast_threshold, p.max_features, p.oriented, p.reserved) == (20, 1000, 1, 0)
    q = abi.FeatureParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))  # the defaults overwrite whatever the struct held
    _capi.lib().srrg2_adapt_default_feature_params(C.byref(q))
    assert bytes(q) == bytes(p)
    _capi.lib().srrg2_adapt_default_feature_params(None)  # (a null pointer is ignored)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """null handle: SRRG2_E_INVALID with a message, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    p, cam = adaptors.default_feature_params(), adaptors.default_depth_params()
    assert lib.srrg2_adapt_image_features(None, None, 1, 0, None, 0, 0, 0, C.byref(cam), C.byref(p), None, 0, None) == -1
    assert b"adapt_image_features" in lib.srrg2_amd_last_error()
    buf = np.zeros(1024, np.int8)
    assert lib.srrg2_feature_pattern(32, buf.ctypes.data_as(C.POINTER(C.c_int8))) == -1
    assert lib.srrg2_feature_pattern(-1, buf.ctypes.data_as(C.POINTER(C.c_int8))) == -1
    assert lib.srrg2_feature_pattern(0, None) == -1
    assert b"feature_pattern" in lib.srrg2_amd_last_error()


def test_pattern_equals_the_restatement_for_every_bin():
    import features_restatement as fr
    from srrg2_slam_interfaces_amd import adaptors

    for k in range(32):
        got = adaptors.feature_pattern(k)
        assert got.dtype == np.int8 and got.shape == (256, 4)
        assert np.array_equal(got.astype(np.int64), fr.rotated_pattern(k)), k
