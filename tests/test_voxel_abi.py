"""CPU: the C ABI of the voxel-grid decimation -- declared in include/srrg2_slam_amd.h, exported by the built library, mirrored
by ctypes structs of the right size, defaults as documented.  Needs no GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls():
    h = _header()
    assert re.search(r"\bint\s+srrg2_scene_voxelize\s*\(", h)
    assert re.search(r"\bvoid\s+srrg2_voxel_default_params\s*\(", h)
    assert re.search(r"SRRG2_VOXEL_CENTROID\s*=\s*0", h) and re.search(r"SRRG2_VOXEL_FIRST\s*=\s*1", h)
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    assert hasattr(lib, "srrg2_scene_voxelize") and hasattr(lib, "srrg2_voxel_default_params")
    assert lib.srrg2_amd_abi_version() == 4


def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import mapping

    assert C.sizeof(abi.VoxelParams) == 32 and C.sizeof(abi.VoxelResult) == 24
    assert mapping.VoxelParams is abi.VoxelParams and mapping.VoxelResult is abi.VoxelResult
    p = mapping.default_voxel_params()
    assert p.leaf_size == C.c_float(0.05).value
    assert list(p.origin) == [0.0, 0.0, 0.0]
    assert p.mode == abi.VOXEL_CENTROID == 0 and abi.VOXEL_FIRST == 1
    assert p.min_points_per_voxel == 1 and list(p.reserved) == [0, 0]
    # the defaults overwrite whatever the struct held
    from srrg2_slam_interfaces_amd import _capi

    q = abi.VoxelParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))
    _capi.lib().srrg2_voxel_default_params(C.byref(q))
    assert bytes(q) == bytes(p)
    _capi.lib().srrg2_voxel_default_params(None)  # (a null pointer is ignored)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """null handles and params: SRRG2_E_INVALID with a message, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, mapping

    lib = _capi.lib()
    p = mapping.default_voxel_params()
    assert lib.srrg2_scene_voxelize(None, C.byref(p), None, None, None) == -1
    assert b"voxelize" in lib.srrg2_amd_last_error()
