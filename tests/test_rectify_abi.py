"""CPU: the C surface of the rectification stage -- exports, struct sizes, defaults, every refusal that needs no device (the
parameters of srrg2_rectifier_set are checked before its handle, so each of them is reachable here; what needs a handle is in
tests/test_gpu_rectify.py) and srrg2_stereo_rectify, which touches no device, bit for bit against the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import rectify_cases as rc
import rectify_restatement as rr
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi

INVALID, UNSUPPORTED, NO_DEVICE = -1, -4, -2
NAMES = ("srrg2_rectifier_create", "srrg2_rectifier_destroy", "srrg2_rectifier_default_params", "srrg2_rectifier_set",
         "srrg2_rectifier_get_map", "srrg2_rectifier_camera", "srrg2_rectify_image", "srrg2_rectify_pair", "srrg2_stereo_rectify")


def _params(**kw):
    p = abi.RectifierParams()
    _capi.lib().srrg2_rectifier_default_params(C.byref(p))
    for i, v in enumerate(rc.K3(40.0, 41.0, 26.2, 18.4).reshape(9)):
        p.camera_matrix[i] = p.new_camera_matrix[i] = v
    p.src_rows, p.src_cols, p.dst_rows, p.dst_cols = 37, 53, 37, 53
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
    assert not any(n.startswith("srrg2_aligner_") for n in NAMES) and lib.srrg2_amd_abi_version() == 4
    assert C.sizeof(abi.RectifierParams) == 35 * 8 + 16 and C.sizeof(abi.RectifierInfo) == 24
    p = abi.RectifierParams()
    C.memset(C.byref(p), 0xff, C.sizeof(p))
    lib.srrg2_rectifier_default_params(C.byref(p))
    assert list(p.camera_matrix) == [0.0] * 9 and list(p.new_camera_matrix) == [0.0] * 9 and list(p.distortion) == [0.0] * 8
    assert list(p.rotation) == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    assert (p.src_rows, p.src_cols, p.dst_rows, p.dst_cols) == (0, 0, 0, 0)
    lib.srrg2_rectifier_default_params(None)  # (a null pointer is ignored)
    assert lib.srrg2_rectifier_destroy(None) == 0


def test_set_refuses_its_parameters_before_its_handle():
    lib = _capi.lib()
    nan, inf = float("nan"), float("inf")
    invalid = [dict(src_rows=-1), dict(src_cols=-1), dict(dst_rows=-1), dict(dst_cols=-1),
               dict(src_rows=50000, src_cols=50000), dict(dst_rows=65536, dst_cols=32768),
               dict(camera_matrix=(0, 0.0)), dict(camera_matrix=(4, 0.0)), dict(new_camera_matrix=(0, 0.0)),
               dict(new_camera_matrix=(4, 0.0)), dict(camera_matrix=(0, nan)), dict(camera_matrix=(4, inf)),
               dict(new_camera_matrix=(0, -inf)), dict(new_camera_matrix=(4, nan)), dict(camera_matrix=(2, nan)),
               dict(camera_matrix=(5, inf)), dict(new_camera_matrix=(2, inf)), dict(new_camera_matrix=(5, nan)),
               dict(camera_matrix=(8, nan)), dict(rotation=(3, nan)), dict(rotation=(8, inf))] + \
              [dict(distortion=(i, nan)) for i in range(8)] + [dict(distortion=(7, inf))]
    unsupported = [dict(camera_matrix=(1, 0.25)), dict(new_camera_matrix=(1, -1e-9)), dict(src_rows=4194305, src_cols=1),
                   dict(src_rows=1, src_cols=4194305)]
    for code, cases in ((INVALID, invalid), (UNSUPPORTED, unsupported)):
        for kw in cases:
            assert lib.srrg2_rectifier_set(None, C.byref(_params(**kw)), None) == code, kw
            msg = lib.srrg2_amd_last_error()
            assert b"rectifier_set" in msg and b"null handle" not in msg, (kw, msg)
    # the sides at their limit pass the parameter checks: only the handle is missing
    for kw in (dict(), dict(src_rows=4194304, src_cols=1), dict(src_rows=0, src_cols=0), dict(dst_rows=0), dict(dst_rows=32768, dst_cols=65535)):
        assert lib.srrg2_rectifier_set(None, C.byref(_params(**kw)), None) == INVALID, kw
        assert b"null handle" in lib.srrg2_amd_last_error(), kw
    assert lib.srrg2_rectifier_set(None, None, None) == INVALID and b"null params" in lib.srrg2_amd_last_error()


def test_calls_refuse_a_null_handle_and_leave_the_destination():
    lib = _capi.lib()
    dst = np.full((37, 53), 0xaa, np.uint8)
    src = np.zeros((37, 53), np.uint8)
    uv = np.full(2 * 37 * 53, 7, np.int32)
    cam = abi.DepthAdaptorParams()
    assert lib.srrg2_rectifier_get_map(None, uv.ctypes.data_as(C.POINTER(C.c_int32)), uv.size) == INVALID
    assert lib.srrg2_rectifier_camera(None, C.byref(cam)) == INVALID
    assert lib.srrg2_rectify_image(None, None, src.ctypes.data, abi.IMAGE_U8, 53, abi.MEM_HOST, dst.ctypes.data, 53, abi.MEM_HOST, 0) == INVALID
    assert b"rectify_image" in lib.srrg2_amd_last_error()
    assert lib.srrg2_rectify_pair(None, None, None, src.ctypes.data, 53, src.ctypes.data, 53, abi.MEM_HOST, dst.ctypes.data, 53,
                                  dst.ctypes.data, 53, abi.MEM_HOST, 0) == INVALID
    assert b"rectify_pair" in lib.srrg2_amd_last_error()
    assert (dst == 0xaa).all() and (uv == 7).all()
    assert lib.srrg2_rectifier_create(0, None) == INVALID


def test_no_cpu_fallback_without_a_device():
    lib = _capi.lib()
    h = C.c_void_p()
    rc_ = lib.srrg2_rectifier_create(0, C.byref(h))
    said = lib.srrg2_amd_last_error()
    if _capi.device_count() > 0:
        assert rc_ == 0 and h
        assert lib.srrg2_rectifier_create(-1, C.byref(C.c_void_p())) == INVALID
        assert lib.srrg2_rectifier_destroy(h) == 0
    else:
        assert rc_ == NO_DEVICE and not h and b"no HIP device" in said
        import srrg2_slam_interfaces_amd as pkg

        with pytest.raises(RuntimeError, match="no HIP device"):
            pkg.ImageRectifier()


def _stereo_rectify(KL, KR, R, t):
    lib = _capi.lib()
    dp = C.POINTER(C.c_double)
    a = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1)) for v in (KL, KR, R, t)]
    R1, R2, Kn = (np.full(9, 7.0) for _ in range(3))
    b = C.c_double(7.0)
    code = lib.srrg2_stereo_rectify(*[v.ctypes.data_as(dp) for v in a], R1.ctypes.data_as(dp), R2.ctypes.data_as(dp),
                                    Kn.ctypes.data_as(dp), C.byref(b))
    return code, R1.reshape(3, 3), R2.reshape(3, 3), Kn.reshape(3, 3), b.value


def test_stereo_rectify_through_ctypes_bit_for_bit():
    rng = np.random.default_rng(11)
    cases = [(rc.RIG_K, rc.RIG_K, rc.RIG_R, rc.RIG_T), (rc.RIG_K, rc.RIG_K, np.eye(3), np.array([-0.3, 0.0, 0.0]))]
    for _ in range(20):
        R = rc.rotation("x", rng.uniform(-0.2, 0.2)) @ rc.rotation("y", rng.uniform(-0.2, 0.2)) @ rc.rotation("x", rng.uniform(-0.1, 0.1))
        t = rng.uniform(-0.5, 0.5, 3)
        cases.append((rc.K3(*rng.uniform(300, 700, 4)), rc.K3(*rng.uniform(300, 700, 4)), R, t))
    for KL, KR, R, t in cases:
        want = rr.stereo_rectify(KL, KR, R, t)
        code, R1, R2, Kn, b = _stereo_rectify(KL, KR, R, t)
        assert code == 0 and want is not None
        assert R1.tobytes() == want[0].tobytes() and R2.tobytes() == want[1].tobytes() and Kn.tobytes() == want[2].tobytes()
        assert b == want[3]
    from srrg2_slam_interfaces_amd import rectify

    R1, R2, Kn, b = rectify.stereo_rectify(*cases[0])  # the Python mirror
    want = rr.stereo_rectify(*cases[0])
    assert R1.tobytes() == want[0].tobytes() and R2.tobytes() == want[1].tobytes() and Kn.tobytes() == want[2].tobytes() and b == want[3]


def test_stereo_rectify_refusals_write_nothing():
    lib = _capi.lib()
    K = rc.RIG_K
    degenerate = [(np.eye(3), np.zeros(3)), (np.eye(3), np.array([0.0, 0.0, -0.3])), (np.eye(3), np.array([math.nan, 0.0, 0.0])),
                  (np.full((3, 3), math.inf), np.array([0.1, 0.0, 0.0]))]
    for R, t in degenerate:
        code, R1, R2, Kn, b = _stereo_rectify(K, K, R, t)
        assert code == INVALID and b"stereo_rectify" in lib.srrg2_amd_last_error()
        assert (R1 == 7.0).all() and (R2 == 7.0).all() and (Kn == 7.0).all() and b == 7.0
        if np.isfinite(R).all() and np.isfinite(t).all():
            assert rr.stereo_rectify(K, K, R, t) is None
    with pytest.raises(ValueError, match="stereo_rectify"):
        from srrg2_slam_interfaces_amd import rectify

        rectify.stereo_rectify(K, K, np.eye(3), np.zeros(3))
    assert lib.srrg2_stereo_rectify(None, None, None, None, None, None, None, None) == INVALID
    dp = C.POINTER(C.c_double)
    a = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1)) for v in (K, K, np.eye(3), [-0.3, 0.0, 0.0])]
    assert lib.srrg2_stereo_rectify(*[v.ctypes.data_as(dp) for v in a], None, None, None, None) == 0  # (every output may be NULL)
