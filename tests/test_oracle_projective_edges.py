"""CPU: the oracle's projective finder and factors against the independent restatement (tests/projective_restatement.py)
over seeded random organised RGB-D pairs and named edges: image shapes down to one pixel row or column, principal points
outside the image, depth bounds hit exactly, z-buffer ties, both SE(3) kinds, every robustifier, the normal gate and a
sensor offset -- and the fixed-point range contract that the bit-for-bit comparisons cannot see."""
import numpy as np
import pytest

import projective_restatement as pr
from helpers import projective_config
from srrg2_slam_interfaces_amd import _abi as abi


def run_oracle(oracle, d, X, par, S=None, moving_normals=True, max_iterations=1):
    al = oracle.OracleAligner(par["kind"])
    al.set_params(max_iterations=max_iterations, min_num_inliers=0)
    si = al.add_slice(projective_config(par["kind"], par["slice_kind"], d, gate=par["gate"], robust=par["robust"],
                                        thr=par["thr"], normal_cos=par["normal_cos"]))
    if S is not None:
        al.set_sensor_in_robot(si, S)
    al.set_fixed(si, d["fixed"], d["fixed_normals"])
    al.set_moving(si, d["moving"], d.get("moving_normals") if moving_normals else None)
    al.set_moving_in_fixed(X)
    return al


def check_against_restatement(oracle, d, X, par, S=None, moving_normals=True):
    """one configuration: association bit for bit, counts, H of the first iteration, the first step, the range"""
    moving_normals = moving_normals and "moving_normals" in d
    fi, mi, resp, lin = pr.expected(d, X, par, S, moving_normals)
    al = run_oracle(oracle, d, X, par, S, moving_normals)
    _, k = al.linearize_once(0)
    assert k == lin["k"], "fixed-point exponent differs from DESIGN.md's formula"
    c = al.correspondences(0)
    assert np.array_equal(c["fixed_idx"], fi) and np.array_equal(c["moving_idx"], mi)
    assert c["response"].tobytes() == resp.tobytes()
    assert np.array_equal(al.factor_status(0), lin["status"])
    # range contract: every scaled term < 2^51 (exact FMA onto 1.5 * 2^52), every scaled sum < 2^62 (no wrap)
    assert lin["max_scaled_term"] < 2.0 ** 51, np.log2(lin["max_scaled_term"])
    assert lin["max_scaled_sum"] < 2.0 ** 62, np.log2(lin["max_scaled_sum"])

    al = run_oracle(oracle, d, X, par, S, moving_normals)
    al.compute()
    st = al.iteration_stats()
    if len(fi) == 0:
        assert al.status() in (abi.NOT_ENOUGH_CORRESPONDENCES, abi.FAIL) and len(st) == 0
        return lin
    assert len(st) == 1
    s0 = st[0]
    for key in ("num_inliers", "num_outliers", "num_suppressed", "num_correspondences"):
        assert s0[key] == lin[key], (key, s0[key], lin[key])
    for key, n in (("chi_inliers", lin["num_inliers"]), ("chi_outliers", lin["num_outliers"])):
        # one rounding onto the grid 2^-k per factor, then float32
        assert abs(s0[key] - lin[key]) <= n * 2.0 ** (-lin["k"] - 1) + 1e-6 * lin[key], (key, s0[key], lin[key])
    H64 = lin["H"]
    Hs = np.abs(H64).max()
    assert np.abs(al.information().astype(np.float64) - H64).max() <= 1e-6 * Hs + 1e-300
    if s0["solver_status"] == 0 and Hs > 0 and np.linalg.cond(H64) < 1e6:
        X1 = pr.gauss_newton_step(X, H64, lin["b"], par["kind"])
        assert np.abs(al.moving_in_fixed().astype(np.float64) - X1).max() <= 1e-5
    return lin


@pytest.mark.parametrize("seed", range(40))
def test_random_configurations(oracle, seed):
    gen, par = pr.random_config(seed)
    d, X, S = pr.make_case(gen, par, seed)
    check_against_restatement(oracle, d, X, par, S)


@pytest.mark.parametrize("shape", [(1, 64), (64, 1), (7, 13), (257, 3), (120, 160)])
@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("slice_kind", [abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION])
def test_image_shapes(oracle, shape, kind, slice_kind):
    rows, cols = shape
    d = pr.rgbd_case(7, rows=rows, cols=cols, fx=90.0, fy=70.0, density=2.0, duplicates=0.05, equal_depth=0.05,
                     on_bounds=9, holes=0.05, nan_normals=0.05, motion=(0.0, 0.0))
    par = dict(kind=kind, slice_kind=slice_kind, robust=abi.ROBUST_CAUCHY, gate=0.05, normal_cos=-2.0,
               thr=0.5 if slice_kind == abi.SLICE_REPROJECTION else 1e-5)
    check_against_restatement(oracle, d, np.eye(4, dtype=np.float32)[:3], par)


@pytest.mark.parametrize("robust", pr.ROBUST)
@pytest.mark.parametrize("slice_kind", [abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION])
def test_robustifiers(oracle, robust, slice_kind):
    d = pr.rgbd_case(11, rows=48, cols=64, fx=80.0, density=1.5)
    par = dict(kind=abi.SE3_QUAT_RIGHT, slice_kind=slice_kind, robust=robust, gate=0.1, normal_cos=-2.0,
               thr=0.3 if slice_kind == abi.SLICE_REPROJECTION else 2e-6)
    lin = check_against_restatement(oracle, d, _perturbed(d), par)
    if robust != abi.ROBUST_NONE:
        assert lin["num_inliers"] > 0 and lin["num_outliers"] > 0  # both classes present


def _perturbed(d):
    P = pr._se3(np.array([0.006, -0.004, 0.003]), np.deg2rad([0.3, -0.2, 0.25]))
    X = np.asarray(d["X_gt"], np.float64)
    return np.concatenate([X[:, :3] @ P[:, :3], (X[:, :3] @ P[:, 3] + X[:, 3])[:, None]], 1).astype(np.float32)


@pytest.mark.parametrize("normal_cos", [-2.0, 0.8])
@pytest.mark.parametrize("moving_normals", [True, False])
@pytest.mark.parametrize("sensor", [False, True])
def test_normal_gate_and_sensor(oracle, normal_cos, moving_normals, sensor):
    """the normal gate needs fixed normals, moving normals and normal_cos > -1; NaN normals at finite fixed pixels"""
    d = pr.rgbd_case(13, rows=40, cols=56, fx=70.0, density=1.2, nan_normals=0.1)
    d["moving_normals"][::3] = -d["moving_normals"][::3]  # a third face away: the gate drops them
    par = dict(kind=abi.SE3_QUAT_RIGHT, slice_kind=abi.SLICE_P2PLANE, robust=abi.ROBUST_NONE, gate=0.05,
               normal_cos=normal_cos, thr=1.0, guess="gt", sensor=sensor)
    X, S = _with_sensor(d, sensor)
    lin = check_against_restatement(oracle, d, X, par, S, moving_normals)
    with_gate = pr.associate(d, X, par["gate"], normal_cos, S, moving_normals)[0].size
    without = pr.associate(d, X, par["gate"], -2.0, S, moving_normals)[0].size
    assert (with_gate < without) == (normal_cos > -1 and moving_normals)
    if not (normal_cos > -1 and moving_normals):
        assert lin["num_suppressed"] > 0  # NaN fixed normals: the factor is suppressed, the correspondence kept


def _with_sensor(d, sensor):
    X_cam = np.asarray(d["X_gt"], np.float64)
    if not sensor:
        return X_cam.astype(np.float32), None
    S = pr.sensor_offset(2)
    S64 = S.astype(np.float64)
    X = np.concatenate([S64[:, :3] @ X_cam[:, :3], (S64[:, :3] @ X_cam[:, 3] + S64[:, 3])[:, None]], 1)
    return X.astype(np.float32), S


def test_edges_are_hit(oracle):
    """the generator's edges really occur: ties in the z-buffer, points exactly on u + 0.5 == cols, q_z == depth_min and
    q_z == depth_max, points behind the camera and non-finite points"""
    d = pr.rgbd_case(5, rows=30, cols=40, fx=50.0, density=3.0, duplicates=0.1, equal_depth=0.1, on_bounds=30,
                     behind=0.05, nonfinite=0.02, motion=(0.0, 0.0))
    P = d["moving"]
    T = pr.finder_transform(np.eye(4, dtype=np.float32)[:3])
    with np.errstate(all="ignore"):
        q = pr._xform(T, P)
        pix, u, v = pr.project(d, q)
    assert np.any(u + np.float32(0.5) == np.float32(d["cols"]))
    assert np.any(q[:, 2] == np.float32(d["depth_min"])) and np.any(q[:, 2] == np.float32(d["depth_max"]))
    assert np.any(q[:, 2] < 0) and np.any(~np.isfinite(P).all(1))
    ok = pix >= 0
    key = pix[ok].astype(np.int64) * 2 ** 32 + q[ok, 2].view(np.uint32)
    assert np.unique(key).size < key.size  # two points on one pixel at one depth
    par = dict(kind=abi.SE3_EULER_RIGHT, slice_kind=abi.SLICE_P2PLANE, robust=abi.ROBUST_NONE, gate=0.2,
               normal_cos=-2.0, thr=1.0)
    check_against_restatement(oracle, d, np.eye(4, dtype=np.float32)[:3], par)


# ---- configurations that push the fixed-point range -----------------------------------------------------------------
BOUND_CASES = {
    # the principal point far outside the image: |u - c_x| is not bounded by the image width (the exponent used to assume so;
    # at c_x = -10000 px the reprojection terms left the grid and H was 48 % off, in the oracle and on the device alike)
    "principal_point_outside": dict(rows=60, cols=80, fx=300.0, cx=-10000.0, depth_min=0.4, depth_range=(0.4, 0.45),
                                    density=0.15),
    "principal_point_far_right": dict(rows=60, cols=80, fx=300.0, cx=3000.0, cy=-900.0, depth_min=0.4,
                                      depth_range=(0.4, 0.5), density=0.15),
    "depth_min_0.05": dict(rows=60, cols=80, fx=120.0, depth_min=0.05, depth_range=(0.05, 0.08), density=0.3,
                           on_bounds=30),
    "fx_5000": dict(rows=60, cols=80, fx=5000.0, fy=4000.0, depth_min=0.3, depth_range=(0.3, 0.4), density=0.3),
    "far_from_origin": dict(rows=60, cols=80, fx=150.0, density=0.3, moving_offset=50.0),
    "full_640x480": dict(rows=480, cols=640, fx=525.0, density=1.0, duplicates=0.01),
}


@pytest.mark.parametrize("name", sorted(BOUND_CASES))
@pytest.mark.parametrize("slice_kind", [abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION])
def test_fixed_point_range(oracle, name, slice_kind):
    gen = dict(BOUND_CASES[name])
    gen.setdefault("motion", (0.0, 0.0) if gen.get("on_bounds") else (0.01, 0.02))
    d = pr.rgbd_case(17, **gen)
    X = np.eye(4, dtype=np.float32)[:3] if gen.get("on_bounds") else d["X_gt"]
    par = dict(kind=abi.SE3_QUAT_RIGHT, slice_kind=slice_kind, robust=abi.ROBUST_NONE, gate=0.05, normal_cos=-2.0,
               thr=1.0)
    lin = check_against_restatement(oracle, d, X, par)
    assert lin["num_correspondences"] > 20


@pytest.mark.parametrize("kind", pr.KINDS)
def test_fixed_points_behind_the_camera(oracle, kind):
    """reprojection factors with f_z <= 0 are suppressed: fixed pixels mirrored behind the camera project to their own pixel,
    pass the depth and distance gates at a small depth_min and give a small residual"""
    d = pr.rgbd_case(23, rows=40, cols=50, fx=60.0, depth_min=0.05, depth_range=(0.05, 0.1), density=1.0,
                     fixed_behind=0.2, motion=(0.0, 0.0))
    par = dict(kind=kind, slice_kind=abi.SLICE_REPROJECTION, robust=abi.ROBUST_NONE, gate=0.2, normal_cos=-2.0, thr=1.0)
    lin = check_against_restatement(oracle, d, np.eye(4, dtype=np.float32)[:3], par)
    fi = pr.associate(d, np.eye(4, dtype=np.float32)[:3], 0.2)[0]
    behind = d["fixed"][fi, 2] <= 0
    assert behind.sum() > 20 and lin["num_suppressed"] >= behind.sum()

def test_exponent_unchanged_inside_the_image():
    """the extent of |u - c_x| is the image size while the principal point lies in the image: the exponent of every
    configuration with a principal point inside the image is the one it always was"""
    for n in (1, 3, 80, 640):
        for c in (-0.5, 0.0, (n - 1) / 2.0, n - 0.5):
            assert pr.proj_extent(n, c) == np.float32(n)
    assert pr.proj_extent(80, -10000.0) == np.float32(10079.5)
    assert pr.proj_extent(80, 3000.0) == np.float32(3000.5)
