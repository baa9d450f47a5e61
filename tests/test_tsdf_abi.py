"""CPU: the srrg2_tsdf_* surface of the C ABI without a device: the symbols exist, the ctypes mirrors have the header's layout,
the defaults are the documented ones, and everything that is refused for its parameters is refused BEFORE the handle is looked at
-- with the documented code, a message that names the parameter, and every destination left as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -4
ROWS, COLS = 6, 8
NAMES = ("create", "destroy", "default_params", "default_frame_params", "default_raycast_params", "reset", "integrate_frames",
         "raycast", "to_scene", "get_planes", "device_arrays")


@pytest.fixture(scope="module")
def lib():
    return _capi.lib()


def _error(lib):
    return (lib.srrg2_amd_last_error() or b"").decode()


def test_symbols_layouts_and_defaults(lib):
    header = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    declared = sorted(set(re.findall(r"\bsrrg2_tsdf_([a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(NAMES)
    for n in NAMES:
        assert hasattr(lib, "srrg2_tsdf_" + n), n
    assert lib.srrg2_amd_abi_version() == 4  # (additive: the version stays)
    assert [C.sizeof(t) for t in (abi.TsdfParams, abi.TsdfFrameParams, abi.TsdfRaycastParams, abi.TsdfResult, abi.TsdfRaycastResult,
                                  abi.TsdfExportResult)] == [32, 8, 16, 32, 28, 8]
    p, f, r = abi.TsdfParams(), abi.TsdfFrameParams(), abi.TsdfRaycastParams()
    p.nx = f.reserved = r.reserved = 9
    lib.srrg2_tsdf_default_params(C.byref(p))
    lib.srrg2_tsdf_default_frame_params(C.byref(f))
    lib.srrg2_tsdf_default_raycast_params(C.byref(r))
    assert (p.nx, p.ny, p.nz, p.with_intensity, list(p.origin)) == (0, 0, 0, 0, [0.0, 0.0, 0.0]) and p.voxel_size == np.float32(0.02)
    assert f.mu == np.float32(0.06) and f.reserved == 0
    assert (r.min_weight, r.skip_empty, r.reserved) == (1, 0, 0) and r.step == np.float32(0.02)
    for fn in (lib.srrg2_tsdf_default_params, lib.srrg2_tsdf_default_frame_params, lib.srrg2_tsdf_default_raycast_params):
        fn(None)  # (null: nothing to do)
    assert lib.srrg2_tsdf_destroy(None) == 0


def _camera(lib):
    c = abi.DepthAdaptorParams()
    lib.srrg2_adapt_default_depth_params(C.byref(c))
    for i, v in enumerate((10.0, 0, 3.5, 0, 10.0, 2.5, 0, 0, 1)):
        c.camera_matrix[i] = v
    c.rows, c.cols = ROWS, COLS
    return c


def test_reset_refuses_its_parameters_before_the_handle(lib):
    def reset(**kw):
        p = abi.TsdfParams()
        lib.srrg2_tsdf_default_params(C.byref(p))
        p.nx = p.ny = p.nz = 4
        for k, v in kw.items():
            if k == "origin":
                p.origin[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return lib.srrg2_tsdf_reset(None, C.byref(p)), _error(lib)

    assert reset() == (E_INVALID, "tsdf_reset: null handle")  # (good parameters: only the handle is missing)
    for kw, word in ((dict(nx=-1), "2048"), (dict(ny=2049), "2048"), (dict(nz=-5), "2048"), (dict(voxel_size=0.0), "voxel_size"),
                     (dict(voxel_size=-1.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"),
                     (dict(voxel_size=float("inf")), "voxel_size"), (dict(origin=(1, float("nan"))), "origin"),
                     (dict(origin=(2, float("-inf"))), "origin"), (dict(with_intensity=2), "with_intensity")):
        rc, msg = reset(**kw)
        assert rc == E_INVALID and word in msg and "handle" not in msg, (kw, msg)
    rc, msg = reset(nx=2048, ny=2048, nz=2048)
    assert rc == E_UNSUPPORTED and "int32" in msg
    assert lib.srrg2_tsdf_reset(None, None) == E_INVALID and "null params" in _error(lib)


def test_integrate_refuses_its_parameters_before_the_handle(lib):
    depth = np.full((2, ROWS, COLS), 1.0, np.float32)
    poses = np.tile(np.eye(3, 4, dtype=np.float32), (2, 1, 1))
    good = dict(depth=C.c_void_p(depth.ctypes.data), depth_type=abi.IMAGE_F32, stride=4 * COLS, inten=None, inten_type=abi.IMAGE_NONE,
                inten_stride=0, k=2, poses=C.c_void_p(poses.ctypes.data), mem=abi.MEM_HOST, mu=0.1, weight=1)

    def call(cam=None, fp="default", **kw):
        a = dict(good)
        a.update(kw)
        f = abi.TsdfFrameParams()
        f.mu = a["mu"]
        out = abi.TsdfResult()
        out.num_frames = out.num_voxel_updates = -7
        rc = lib.srrg2_tsdf_integrate_frames(None, a["depth"], a["depth_type"], a["stride"], a["inten"], a["inten_type"], a["inten_stride"],
                                             a["k"], a["poses"], a["mem"], C.byref(cam if cam is not None else _camera(lib)),
                                             None if fp is None else C.byref(f), a["weight"], C.byref(out))
        assert (out.num_frames, out.num_voxel_updates) == (-7, -7)  # (refused: the result is untouched)
        return rc, _error(lib)

    assert call() == (E_INVALID, "tsdf_integrate_frames: null handle")
    bad_pose = poses.copy()
    bad_pose[1, 2, 3] = np.nan
    u8 = np.zeros((2, ROWS, COLS), np.uint8)
    odd = np.zeros(4 * 2 * ROWS * COLS + 8, np.uint8)
    for kw, word in ((dict(weight=0), "weight"), (dict(weight=2), "weight"), (dict(weight=-2), "weight"), (dict(k=-1), "num_frames"),
                     (dict(depth_type=abi.IMAGE_U8), "depth_type"), (dict(depth_type=abi.IMAGE_NONE), "depth_type"),
                     (dict(inten_type=abi.IMAGE_U16), "intensity_type"), (dict(mu=0.0), "mu"), (dict(mu=float("nan")), "mu"),
                     (dict(mu=float("inf")), "mu"), (dict(mem=abi.MEM_DEVICE_KEPT), "mem"), (dict(stride=4 * COLS - 4), "stride"),
                     (dict(stride=4 * COLS + 2), "stride"), (dict(depth=C.c_void_p(odd.ctypes.data + 1)), "aligned"),
                     (dict(depth=None), "null image"), (dict(poses=None), "null poses"),
                     (dict(poses=C.c_void_p(bad_pose.ctypes.data)), "finite"),
                     (dict(inten=None, inten_type=abi.IMAGE_U8, inten_stride=COLS), "null image"),
                     (dict(inten=C.c_void_p(u8.ctypes.data), inten_type=abi.IMAGE_U8, inten_stride=COLS - 1), "intensity row stride")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and word in msg and "handle" not in msg, (kw, msg)
    assert call(fp=None)[0] == E_INVALID
    # the depth adaptor's camera refusals, with its codes
    for field, value, code in (("rows", -1, E_INVALID), ("cols", -1, E_INVALID), ("fx", 0.0, E_INVALID), ("fy", float("inf"), E_INVALID),
                               ("skew", 0.25, E_UNSUPPORTED)):
        cam = _camera(lib)
        if field in ("rows", "cols"):
            setattr(cam, field, value)
        else:
            cam.camera_matrix[{"fx": 0, "fy": 4, "skew": 1}[field]] = value
        rc, msg = call(cam=cam)
        assert rc == code and "handle" not in msg, (field, msg)
    # zero frames and zero pixels have nothing to check of their data pointers: only the handle is missing
    assert call(k=0, depth=None, poses=None)[1].endswith("null handle")
    empty = _camera(lib)
    empty.rows = 0
    assert call(cam=empty, depth=None)[1].endswith("null handle")


def test_raycast_and_export_refuse_their_parameters_before_the_handle(lib):
    pose = np.eye(3, 4, dtype=np.float32)
    image = np.full((ROWS, COLS), 7.0, np.float32)

    def call(cam=None, pose_=pose, mem=abi.MEM_HOST, **kw):
        r = abi.TsdfRaycastParams()
        lib.srrg2_tsdf_default_raycast_params(C.byref(r))
        for k, v in kw.items():
            setattr(r, k, v)
        out = abi.TsdfRaycastResult()
        out.num_pixels = -7
        rc = lib.srrg2_tsdf_raycast(None, None if pose_ is None else C.c_void_p(pose_.ctypes.data), C.byref(cam if cam is not None else _camera(lib)),
                                    C.byref(r), None, C.c_void_p(image.ctypes.data), mem, C.byref(out))
        assert out.num_pixels == -7 and np.all(image == 7.0)
        return rc, _error(lib)

    assert call() == (E_INVALID, "tsdf_raycast: null handle")
    bad_pose = pose.copy()
    bad_pose[0, 0] = np.inf
    for kw, word in ((dict(step=0.0), "step"), (dict(step=-0.1), "step"), (dict(step=float("nan")), "step"), (dict(min_weight=0), "min_weight"),
                     (dict(skip_empty=2), "skip_empty"), (dict(reserved=1), "reserved"), (dict(pose_=None), "null pose"),
                     (dict(pose_=bad_pose), "finite"), (dict(mem=5), "mem"), (dict(step=1e-7), "2^20")):
        rc, msg = call(**kw)
        assert rc == E_INVALID and word in msg and "handle" not in msg, (kw, msg)
    cam = _camera(lib)
    cam.normal_col_gap = 0  # (exactly one gap 0: the adaptor would refuse the image afterwards)
    rc, msg = call(cam=cam)
    assert rc == E_INVALID and "gaps" in msg
    cam = _camera(lib)
    cam.depth_max = float("nan")
    assert call(cam=cam)[0] == E_INVALID
    cam = _camera(lib)
    cam.camera_matrix[1] = 1.0
    assert call(cam=cam)[0] == E_UNSUPPORTED
    assert lib.srrg2_tsdf_to_scene(None, 0, None, None) == E_INVALID and "min_weight" in _error(lib)
    assert lib.srrg2_tsdf_to_scene(None, 1, None, None) == E_INVALID and "null handle" in _error(lib)
    words = np.full(4, 7, np.int32)
    ptr = C.c_void_p(words.ctypes.data)
    assert lib.srrg2_tsdf_get_planes(None, ptr, ptr, ptr, 7) == E_INVALID and "mem" in _error(lib)
    assert lib.srrg2_tsdf_get_planes(None, ptr, ptr, ptr, abi.MEM_HOST) == E_INVALID and "null handle" in _error(lib)
    assert lib.srrg2_tsdf_device_arrays(None, None, None, None) == E_INVALID
    assert np.all(words == 7)
    assert lib.srrg2_tsdf_create(0, None) == E_INVALID
