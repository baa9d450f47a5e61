"""GPU: the projective path on the edges of tests/test_oracle_projective_edges.py, through every launch shape the host picks
(one slice, a pack of 2-4 unshared slices, 2-4 slices on one shared association, 5-8 slices launched one by one, the pack
split by SRRG2_TUNE_PROJ_SEPARATE_LAUNCHES (bit 17), fused control on and off, the k_icp_init launch in front
(SRRG2_TUNE_INIT_LAUNCH, bit 23), prior slices either side), one handle over many compute() calls, and compute_batch with a projective cue slice.
Every run is the oracle's bit for bit; the first iteration is the float64 restatement's."""
import numpy as np
import pytest

import projective_restatement as pr
from helpers import assert_same_run, prior_config, projective_config
from srrg2_slam_interfaces_amd import _abi as abi

pytestmark = pytest.mark.gpu

QUAT, EULER = abi.SE3_QUAT_RIGHT, abi.SE3_EULER_RIGHT
I3 = np.eye(4, dtype=np.float32)[:3]


def _cfg(kind, sk, d, gate=0.05, robust=abi.ROBUST_CAUCHY, normal_cos=-2.0):
    thr = 0.5 if sk == abi.SLICE_REPROJECTION else 1e-5
    return projective_config(kind, sk, d, gate=gate, robust=robust, thr=thr, normal_cos=normal_cos)


def _add_cues(al, oracle, d, kind, kinds, shared, gates=None, S=None, robusts=None):
    """projective slices on one pair; shared: slices after the first read its clouds (one association)"""
    first = None
    out = []
    for z, sk in enumerate(kinds):
        gate = gates[z] if gates else 0.05
        robust = robusts[z] if robusts else abi.ROBUST_CAUCHY
        si = al.add_slice(_cfg(kind, sk, d, gate=gate, robust=robust))
        if S is not None:
            al.set_sensor_in_robot(si, S)
        if first is None or not shared or isinstance(al, oracle.OracleAligner):
            # (unshared slices get the moving points in another order: another z-buffer, other winners per pixel)
            perm = np.arange(d["moving"].shape[0]) if shared or z == 0 else np.random.default_rng(z).permutation(d["moving"].shape[0])
            al.set_fixed(si, d["fixed"], d["fixed_normals"])
            al.set_moving(si, d["moving"][perm], d["moving_normals"][perm] if "moving_normals" in d else None)
        else:
            al.share_clouds(si, first)
        first = si if first is None else first
        out.append(si)
    return tuple(out)


def _compare(ref, got):
    assert ref.information().tobytes() == got.information().tobytes()


# ---- launch shapes --------------------------------------------------------------------------------------------------
P, R = abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION
SHAPES = {
    "one": dict(kinds=(P,), shared=False),
    "one_repro": dict(kinds=(R,), shared=False),
    "pack2": dict(kinds=(P, R), shared=False),
    "pack3": dict(kinds=(P, R, P), shared=False, gates=(0.05, 0.05, 0.1)),
    "pack4": dict(kinds=(P, R, R, P), shared=False, gates=(0.05, 0.1, 0.05, 0.02)),
    "fused2": dict(kinds=(P, R), shared=True),
    "fused3": dict(kinds=(P, R, P), shared=True, robusts=(abi.ROBUST_CAUCHY, abi.ROBUST_SATURATED, abi.ROBUST_CLAMP)),
    "fused4": dict(kinds=(P, R, R, P), shared=True),
    "separate5": dict(kinds=(P, R, P, R, P), shared=False),
    "separate8": dict(kinds=(P, R) * 4, shared=True),
    "pack3_bit17": dict(kinds=(P, R, P), shared=False, knobs={"strategy_mask": abi.TUNE_PROJ_SEPARATE_LAUNCHES}),
    "fused2_bit17": dict(kinds=(P, R), shared=True, knobs={"strategy_mask": abi.TUNE_PROJ_SEPARATE_LAUNCHES}),
    "fused2_control0": dict(kinds=(P, R), shared=True, knobs={"fused_control": 0}),
    "fused2_control1": dict(kinds=(P, R), shared=True, knobs={"fused_control": 1}),
    "fused3_bit23": dict(kinds=(P, R, P), shared=True, knobs={"fused_control": 1, "strategy_mask": abi.TUNE_INIT_LAUNCH}),
    "prior_before_fused": dict(kinds=(P, R), shared=True, prior="before"),
    "prior_after_pack": dict(kinds=(P, R), shared=False, prior="after"),
    "prior_after_fused": dict(kinds=(P, R, P), shared=True, prior="after"),
}


def _fused_expected(sh):
    """the host fuses the control steps into the passes of projective slices that share one association (2-4 of them)"""
    knobs = sh.get("knobs", {})
    n = len(sh["kinds"])
    return sh["shared"] and 2 <= n <= 4 and knobs.get("fused_control", 1) != 0 and not (
        knobs.get("strategy_mask", 0) & abi.TUNE_PROJ_SEPARATE_LAUNCHES)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("case", ["edges_quat", "edges_euler", "outside_pp"])
def test_launch_shapes(oracle, product, shape, case):
    sh = SHAPES[shape]
    kind = EULER if case == "edges_euler" and "prior" not in sh else QUAT  # (SE(3) priors: the quaternion variable only)
    if case == "outside_pp":
        d = pr.rgbd_case(41, rows=45, cols=61, fx=300.0, cx=-3000.0, cy=-40.0, depth_min=0.4, depth_range=(0.4, 0.6),
                         density=0.4, motion=(0.002, 0.002))
        guess = d["X_gt"]
    else:
        d = pr.rgbd_case(40, rows=61, cols=83, fx=95.0, fy=80.0, cx=2.0, cy=55.0, density=2.0, duplicates=0.05,
                         equal_depth=0.05, behind=0.01, nonfinite=0.01, holes=0.05, nan_normals=0.03,
                         motion=(0.003, 0.005))
        guess = I3
    Z = d["X_gt"]
    runs = []
    for al in (oracle.OracleAligner(kind), product.MultiAligner(kind)):
        if not isinstance(al, oracle.OracleAligner) and sh.get("knobs"):
            al.set_tuning(**sh["knobs"])
        al.set_params(max_iterations=6, min_num_inliers=10)
        if sh.get("prior") == "before":
            pi = al.add_slice(prior_config(kind, info=[10, 10, 10, 100, 100, 100], sets_guess=0))
            al.set_prior_measurement(pi, Z)
        cues = _add_cues(al, oracle, d, kind, sh["kinds"], sh["shared"], sh.get("gates"), robusts=sh.get("robusts"))
        if sh.get("prior") == "after":
            pi = al.add_slice(prior_config(kind, info=[10, 10, 10, 100, 100, 100], sets_guess=0))
            al.set_prior_measurement(pi, Z)
        paths = []
        for g in (guess, guess):  # twice: the second compute() may fold the prologue into the first pass
            al.set_moving_in_fixed(g)
            al.compute()
            paths.append(al.last_compute_path())
        runs.append((al, cues, paths))
    (ref, cues, _), (got, _, paths) = runs
    assert ref.status() == abi.SUCCESS
    assert_same_run(ref, got, slices=cues)
    _compare(ref, got)
    fused = _fused_expected(sh)
    knobs = sh.get("knobs", {})
    for k, path in enumerate(paths):
        assert bool(path & abi.PATH_FUSED_CONTROL) == fused, (shape, path)
        if fused:
            assert path & abi.PATH_FINAL_WAVE, (shape, path)
            prologue = k > 0 and not knobs.get("strategy_mask", 0) & abi.TUNE_INIT_LAUNCH
            assert bool(path & abi.PATH_PROLOGUE_IN_PASS) == prologue, (shape, k, path)
            assert bool(path & abi.PATH_PRIORS_FUSED) == ("prior" in sh), (shape, path)


@pytest.mark.parametrize("seed", range(0, 40, 3))
def test_random_configurations_first_iteration(oracle, product, seed):
    """the CPU module's random configurations: the first iteration equals the restatement, the whole run the oracle"""
    gen, par = pr.random_config(seed)
    d, X, S = pr.make_case(gen, par, seed)
    fi, mi, resp, lin = pr.expected(d, X, par, S, "moving_normals" in d)
    runs = []
    for al in (oracle.OracleAligner(par["kind"]), product.MultiAligner(par["kind"])):
        al.set_params(max_iterations=1, min_num_inliers=0)
        si = al.add_slice(projective_config(par["kind"], par["slice_kind"], d, gate=par["gate"], robust=par["robust"],
                                            thr=par["thr"], normal_cos=par["normal_cos"]))
        if S is not None:
            al.set_sensor_in_robot(si, S)
        al.set_fixed(si, d["fixed"], d["fixed_normals"])
        al.set_moving(si, d["moving"], d.get("moving_normals"))
        al.set_moving_in_fixed(X)
        al.compute()
        runs.append(al)
    ref, got = runs
    assert_same_run(ref, got)
    if len(fi) == 0:
        return
    _compare(ref, got)
    c = got.correspondences(0)
    assert np.array_equal(c["fixed_idx"], fi) and np.array_equal(c["moving_idx"], mi)
    assert c["response"].tobytes() == resp.tobytes()
    assert np.array_equal(got.factor_status(0), lin["status"])
    s0 = got.iteration_stats()[0]
    for key in ("num_inliers", "num_outliers", "num_suppressed", "num_correspondences"):
        assert s0[key] == lin[key], key
    H64 = lin["H"]
    assert np.abs(got.information().astype(np.float64) - H64).max() <= 1e-6 * np.abs(H64).max() + 1e-300


@pytest.mark.parametrize("name", ["principal_point_outside", "depth_min_0.05", "fx_5000", "full_640x480"])
def test_fixed_point_range_cases(oracle, product, name):
    """the configurations that push the fixed-point range: the device's H is the oracle's bits and the float64 sum"""
    from test_oracle_projective_edges import BOUND_CASES

    gen = dict(BOUND_CASES[name])
    gen.setdefault("motion", (0.0, 0.0) if gen.get("on_bounds") else (0.01, 0.02))
    d = pr.rgbd_case(17, **gen)
    X = I3 if gen.get("on_bounds") else d["X_gt"]
    runs = []
    for al in (oracle.OracleAligner(QUAT), product.MultiAligner(QUAT)):
        al.set_params(max_iterations=1, min_num_inliers=0)
        _add_cues(al, oracle, d, QUAT, (P, R), shared=True, robusts=(abi.ROBUST_NONE, abi.ROBUST_NONE))
        al.set_moving_in_fixed(X)
        al.compute()
        runs.append(al)
    ref, got = runs
    assert_same_run(ref, got, slices=(0, 1))
    _compare(ref, got)
    H64 = np.zeros((6, 6))
    for sk, si in ((P, 0), (R, 1)):
        c = got.correspondences(si)
        par = dict(kind=QUAT, slice_kind=sk, robust=abi.ROBUST_NONE, thr=1.0, gate=0.05, normal_cos=-2.0)
        lin = pr.linearize(d, X, c["fixed_idx"], c["moving_idx"], sk, QUAT, gate=0.05)
        assert lin["max_scaled_term"] < 2.0 ** 51 and lin["max_scaled_sum"] < 2.0 ** 62
        H64 += lin["H"]
    assert np.abs(got.information().astype(np.float64) - H64).max() <= 1e-6 * np.abs(H64).max()


def test_one_handle_many_computes(oracle, product):
    """one handle, many compute() calls: guesses, moving clouds of different sizes, a run stopped by the termination
    criterion, an inlier-only run, keep_only_inlier_correspondences; every compute is a fresh oracle's, and
    correspondences() after each one (the z-buffer's parity and reset across runs, k_proj_zbuf_last, k_proj_records)"""
    kind = QUAT
    d = pr.rgbd_case(50, rows=60, cols=80, fx=90.0, density=2.0, duplicates=0.05, equal_depth=0.05, holes=0.03,
                     motion=(0.01, 0.01))
    n = d["moving"].shape[0]
    steps = [  # (moving subset, guess, params, termination)
        (slice(None), I3, dict(max_iterations=5), None),
        (slice(0, n // 3), d["X_gt"], dict(max_iterations=3), None),
        (slice(None), I3, dict(max_iterations=12), abi.default_termination_params()),
        (slice(n // 4, n), I3, dict(max_iterations=6, enable_inlier_only_runs=True), None),
        (slice(None), d["X_gt"], dict(max_iterations=4, keep_only_inlier_correspondences=True), None),
        (slice(0, 7), I3, dict(max_iterations=2), None),
        (slice(None), I3, dict(max_iterations=7), None),
    ]
    for shared in (False, True):
        got = product.MultiAligner(kind)
        cues = _add_cues(got, oracle, d, kind, (P, R), shared)
        for k, (sub, guess, params, term) in enumerate(steps):
            ref = oracle.OracleAligner(kind)
            _add_cues(ref, oracle, d, kind, (P, R), shared)
            for al in (ref, got):
                al.set_params(min_num_inliers=10, **params)
                al.set_termination_criteria(term)
                if k > 0:
                    for si in cues if (not shared or al is ref) else cues[:1]:
                        al.set_moving(si, d["moving"][sub], d["moving_normals"][sub])
                al.set_moving_in_fixed(guess)
                al.compute()
            assert_same_run(ref, got, slices=cues)
            if ref.iteration_stats():  # (no iteration: information() is not defined by the run)
                _compare(ref, got)


@pytest.mark.parametrize("K", [1, 5, 12])
def test_compute_batch_with_a_projective_cue_slice(oracle, product, K):
    """compute_batch with one projective cue slice: ragged clouds, an empty cloud, a one-point cloud, NaNs"""
    kind = QUAT
    d = pr.rgbd_case(60, rows=48, cols=64, fx=80.0, density=1.5, nonfinite=0.01, motion=(0.005, 0.01))
    rng = np.random.default_rng(K)
    n = d["moving"].shape[0]
    clouds, normals, guesses = [], [], []
    for k in range(K):
        if K > 1 and k == 1:
            sel = np.arange(0)
        elif K > 1 and k == 2:
            sel = np.arange(1)
        else:
            sel = np.sort(rng.choice(n, int(rng.integers(n // 4, n)), replace=False))
        clouds.append(d["moving"][sel])
        normals.append(d["moving_normals"][sel])
        guesses.append(d["X_gt"] if k % 2 else I3)
    res = []
    for al in (oracle.OracleAligner(kind), product.MultiAligner(kind)):
        al.set_params(max_iterations=5, min_num_inliers=10)
        si = al.add_slice(_cfg(kind, P, d))
        al.set_fixed(si, d["fixed"], d["fixed_normals"])
        res.append(al.compute_batch(clouds, guesses, normals))
    r_ref, r_got = res
    assert np.array_equal(r_ref.status, r_got.status)
    assert np.array_equal(r_ref.num_iterations, r_got.num_iterations)
    assert np.array_equal(r_ref.num_correspondences, r_got.num_correspondences)
    assert r_ref.moving_in_fixed.tobytes() == r_got.moving_in_fixed.tobytes()
    assert r_ref.information.tobytes() == r_got.information.tobytes()
    assert (r_got.num_correspondences > 0).sum() >= K - 2


@pytest.mark.parametrize("moving_normals", [True, False])
@pytest.mark.parametrize("shape", ["one", "pack2", "fused2"])
def test_normal_gate_needs_moving_normals(oracle, product, moving_normals, shape):
    """normal_cos > -1 gates only when the fixed AND the moving cloud carry normals (NaN fixed normals at finite pixels)"""
    d = pr.rgbd_case(70, rows=40, cols=56, fx=70.0, density=1.2, nan_normals=0.1, motion=(0.003, 0.005))
    d["moving_normals"][::3] = -d["moving_normals"][::3]
    if not moving_normals:
        del d["moving_normals"]
    sh = SHAPES[shape]
    runs = []
    for al in (oracle.OracleAligner(QUAT), product.MultiAligner(QUAT)):
        al.set_params(max_iterations=4, min_num_inliers=10)
        first = None
        for z, sk in enumerate(sh["kinds"]):
            si = al.add_slice(_cfg(QUAT, sk, d, normal_cos=0.8))
            if first is None or not sh["shared"] or isinstance(al, oracle.OracleAligner):
                al.set_fixed(si, d["fixed"], d["fixed_normals"])
                al.set_moving(si, d["moving"], d.get("moving_normals"))
            else:
                al.share_clouds(si, first)
            first = si if first is None else first
        al.set_moving_in_fixed(I3)
        al.compute()
        runs.append(al)
    ref, got = runs
    cues = tuple(range(len(sh["kinds"])))
    assert_same_run(ref, got, slices=cues)
    _compare(ref, got)
    gated = pr.associate(d, I3, 0.05, 0.8, None, moving_normals)[0].size
    assert (gated < pr.associate(d, I3, 0.05, -2.0)[0].size) == moving_normals


@pytest.mark.parametrize("shape", ["one_repro", "pack2", "fused2"])
def test_fixed_points_behind_the_camera(oracle, product, shape):
    """reprojection factors whose fixed point has f_z <= 0 are suppressed (finite fixed pixels mirrored behind the camera)"""
    d = pr.rgbd_case(23, rows=40, cols=50, fx=60.0, depth_min=0.05, depth_range=(0.05, 0.1), density=1.0,
                     fixed_behind=0.2, motion=(0.0, 0.0))
    sh = SHAPES[shape]
    runs = []
    for al in (oracle.OracleAligner(QUAT), product.MultiAligner(QUAT)):
        al.set_params(max_iterations=3, min_num_inliers=10)
        cues = _add_cues(al, oracle, d, QUAT, sh["kinds"], sh["shared"], gates=(0.2,) * len(sh["kinds"]),
                         robusts=(abi.ROBUST_NONE,) * len(sh["kinds"]))
        al.set_moving_in_fixed(I3)
        al.compute()
        runs.append(al)
    ref, got = runs
    assert_same_run(ref, got, slices=cues)
    _compare(ref, got)
    si = sh["kinds"].index(R)
    st = got.factor_status(si)
    c = got.correspondences(si)
    behind = d["fixed"][c["fixed_idx"], 2] <= 0
    assert behind.sum() > 20 and np.all(st[behind] == abi.FACTOR_SUPPRESSED)
