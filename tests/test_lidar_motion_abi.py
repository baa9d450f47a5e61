"""CPU: the C ABI of the ring-table / de-skew extension of the lidar frame -- srrg2_lidar_sweep_extras, srrg2_adapt_lidar_sweep_ex,
srrg2_scene_clip_spherical_rings: declared in include/srrg2_slam_amd.h, exported by the built library, the ctypes struct of the
size a C compiler gives it, defaults as documented, null arguments refused before any device is touched.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("srrg2_adapt_lidar_sweep_ex", "srrg2_scene_clip_spherical_rings")
DEFAULTS = ("srrg2_adapt_default_lidar_sweep_extras",)
FIELDS = ("ring_elevations", "times", "time_stride_bytes", "deskew", "time_begin", "time_end", "reference", "motion", "reserved")


def _header():
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_calls_and_the_struct():
    h = _header()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    for name in DEFAULTS:
        assert re.search(r"\bvoid\s+%s\s*\(" % name, h), name
    body = re.search(r"typedef\s+struct\s+srrg2_lidar_sweep_extras\s*\{(.*?)\}\s*srrg2_lidar_sweep_extras\s*;", h, flags=re.S)
    assert body
    for field in FIELDS:
        assert re.search(r"\b%s\b" % field, body.group(1)), field
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


def test_library_exports_the_calls():
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for name in CALLS + DEFAULTS:
        assert hasattr(lib, name), name
    assert lib.srrg2_amd_abi_version() == 4


def test_ctypes_size_is_the_compilers(tmp_path):
    from srrg2_slam_interfaces_amd import _abi as abi

    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "srrg2_slam_amd.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(srrg2_lidar_sweep_extras),\n'
                   "         offsetof(srrg2_lidar_sweep_extras, deskew), offsetof(srrg2_lidar_sweep_extras, time_begin),\n"
                   "         offsetof(srrg2_lidar_sweep_extras, reference), offsetof(srrg2_lidar_sweep_extras, motion),\n"
                   "         offsetof(srrg2_lidar_sweep_extras, reserved), sizeof(srrg2_lidar_adaptor_params));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(w) for w in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()]
    X = abi.LidarSweepExtras
    assert got == [C.sizeof(X), X.deskew.offset, X.time_begin.offset, X.reference.offset, X.motion.offset, X.reserved.offset,
                   C.sizeof(abi.LidarAdaptorParams)]
    assert C.sizeof(abi.SphericalModel) == 48 and C.sizeof(abi.LidarAdaptorParams) == 72 and C.sizeof(abi.SphericalClipParams) == 104


def test_defaults_overwrite_the_struct():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    x = adaptors.default_lidar_sweep_extras()
    assert not x.ring_elevations and x.times is None and (x.time_stride_bytes, x.deskew) == (0, 0)
    assert (x.time_begin, x.time_end, x.reference) == (0.0, 0.0, 1.0)
    assert list(x.motion) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and list(x.reserved) == [0, 0]
    y = abi.LidarSweepExtras()
    C.memset(C.byref(y), 0xFF, C.sizeof(y))
    lib.srrg2_adapt_default_lidar_sweep_extras(C.byref(y))
    assert bytes(y) == bytes(x)
    lib.srrg2_adapt_default_lidar_sweep_extras(None)  # (a null pointer is ignored)


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """null handles and params: SRRG2_E_INVALID with a message naming the call, no GPU needed"""
    from srrg2_slam_interfaces_amd import _capi, adaptors, mapping

    lib = _capi.lib()
    p, x = adaptors.default_lidar_params(), adaptors.default_lidar_sweep_extras()
    for extras in (None, C.byref(x)):
        assert lib.srrg2_adapt_lidar_sweep_ex(None, None, 12, None, 0, 0, 0, C.byref(p), extras, None) == -1
        assert b"adapt_lidar_sweep_ex" in lib.srrg2_amd_last_error()
    c = mapping.default_spherical_clip_params()
    table = (C.c_double * 4)(-0.3, -0.1, 0.1, 0.3)
    for rings in (None, table):
        assert lib.srrg2_scene_clip_spherical_rings(None, None, C.byref(c), rings, None, None) == -1
        assert b"scene_clip_spherical_rings" in lib.srrg2_amd_last_error()
    # the plain calls keep their own names
    assert lib.srrg2_adapt_lidar_sweep(None, None, 12, None, 0, 0, 0, C.byref(p), None) == -1
    assert b"adapt_lidar_sweep:" in lib.srrg2_amd_last_error()
