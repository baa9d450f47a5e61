"""CPU: the float64 Gauss-Newton restatement (tests/posegraph_restatement.py) is pinned before it judges the HIP solver in
tests/test_gpu_posegraph_cycles.py: it reproduces the committed SciPy fixtures, and it agrees with the oracle's dense direct
solve on small graphs with fixed masks, disabled factors, full information matrices, duplicate and reversed factors and damping."""
import os

import numpy as np
import pytest

import posegraph_restatement as PR
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import posegraph as pgm
from srrg2_slam_interfaces_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reproduces_scipy_fixture_se3():
    G = np.load(os.path.join(GOLDEN, "posegraph_golden.npz"))
    g = syn.pose_graph_3d(V=100, E=300, seed=11)
    chi0, dx, after = PR.gn_step(abi.SE3_QUAT_RIGHT, g["poses_init"], g["ij"], g["Z"])
    assert abs(chi0 - float(G["chi0"])) <= 1e-9 * float(G["chi0"])
    assert np.max(np.abs(dx.reshape(-1) - G["dx"])) <= 1e-7 * max(1.0, np.max(np.abs(G["dx"])))
    assert np.max(np.abs(after.astype(np.float32) - G["poses_after_1"])) <= 1e-6


def test_reproduces_scipy_fixture_se2_two_steps():
    """both steps of posegraph_golden_se2.npz: 1 500 poses take the dense path (4 500 unknowns); chi
    within 2e-8 relative (the fixture inverts Z and Xi with np.linalg.inv, the restatement in closed form)"""
    G = np.load(os.path.join(GOLDEN, "posegraph_golden_se2.npz"))
    g = syn.pose_graph_2d(V=1500, E=4500, seed=5300)
    chis, P = PR.gauss_newton(abi.SE2_RIGHT, g["poses_init"], g["ij"], g["Z"], 1)
    assert abs(chis[0] - float(G["chi0"])) <= 2e-8 * float(G["chi0"])
    assert np.max(np.abs(P - G["poses_after_1"])) <= 1e-6
    chi1, dx1, after = PR.gn_step(abi.SE2_RIGHT, G["poses_after_1"], g["ij"], g["Z"])
    assert abs(chi1 - float(G["chi1"])) <= 2e-8 * float(G["chi1"])
    assert abs(np.max(np.abs(dx1)) - float(G["max_abs_dx"][1])) <= 1e-7
    assert np.max(np.abs(after.astype(np.float32) - G["poses_after_2"])) <= 1e-6


def _perturbed_case(kind, seed):
    """a small generator graph plus one duplicate and one reversed factor, full information matrices, 1/6 of the factors
    disabled, three fixed poses (none of them pose 0's only), poses perturbed off the odometry guess"""
    g = syn.pose_graph_2d(V=60, E=150, seed=seed) if kind == abi.SE2_RIGHT else syn.pose_graph_3d(V=60, E=180, seed=seed)
    D = PR.dim(kind)
    ij = np.concatenate([g["ij"], g["ij"][[5]], g["ij"][[9], ::-1]]).astype(np.int32)
    Zr = PR._inv(kind, g["Z"][9].astype(np.float64))
    Z = np.concatenate([g["Z"], g["Z"][[5]], Zr[None].astype(np.float32)]).astype(np.float32)
    E = ij.shape[0]
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(E, D, D)) * 0.3
    om = (np.eye(D) + np.einsum("eab,ecb->eac", A, A)).astype(np.float32)
    en = np.ones(E, np.uint8)
    en[1::6] = 0
    en[:59] = 1  # the odometry keeps the graph connected
    fm = np.zeros(60, np.uint8)
    fm[[0, 17, 44]] = 1
    P = PR.box_plus(kind, g["poses_init"].astype(np.float64), rng.normal(size=(60, D)) * 0.02).astype(np.float32)
    P[fm.astype(bool)] = g["poses_init"][fm.astype(bool)]
    return P, ij, Z, om, en, fm


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("kind", [abi.SE2_RIGHT, abi.SE3_QUAT_RIGHT])
def test_agrees_with_oracle_direct_solve(oracle, kind, damping):
    P, ij, Z, om, en, fm = _perturbed_case(kind, 71 if kind == abi.SE2_RIGHT else 72)
    pg = oracle.OraclePoseGraph(kind)
    pg.set_direct(True)
    pg.set_graph(P, ij, Z, omega=om, fixed_mask=fm, enabled=en)
    p = pgm.default_params()
    p.max_iterations, p.damping = 1, damping
    st = pg.solve(p)
    chi0, dx, after = PR.gn_step(kind, P, ij, Z, omega=om, enabled=en, fixed_mask=fm, damping=damping)
    assert st[0]["solver_status"] == 0 and st[0]["num_factors"] == int(en.sum())
    assert abs(st[0]["chi"] - chi0) <= 1e-6 * chi0
    assert np.max(np.abs(dx)) > 1e-2  # the step moves the poses
    assert np.max(np.abs(pg.poses() - after)) <= 2e-6
    assert np.array_equal(pg.poses()[fm.astype(bool)], P[fm.astype(bool)])


@pytest.mark.parametrize("kind", [abi.SE2_RIGHT, abi.SE3_QUAT_RIGHT])
def test_banded_solve_matches_dense_solve(kind):
    """the block-banded path (an odometry chain in both directions, a duplicate, short closures, fixed poses inside, damping)
    against the dense one on the same system"""
    D = PR.dim(kind)
    rng = np.random.default_rng(5)
    V = 40
    gt = PR.v2t(kind, np.cumsum(rng.normal(size=(V, D)) * 0.3, 0) if kind == abi.SE2_RIGHT else
                np.concatenate([np.cumsum(rng.normal(size=(V, 3)), 0), rng.normal(size=(V, 3)) * 0.1], 1))
    ij = np.stack([np.arange(V - 1), np.arange(1, V)], 1)
    ij[::5] = ij[::5, ::-1]
    ij = np.concatenate([ij, ij[[3]], [[4, 9], [30, 26], [12, 13], [37, 39]]])
    Z = PR._mul(kind, PR._inv(kind, gt[ij[:, 0]]), gt[ij[:, 1]])
    P = PR.box_plus(kind, gt, rng.normal(size=(V, D)) * 0.05)
    fm = np.zeros(V, bool)
    fm[[0, 21, 27]] = True
    om = np.tile(np.eye(D) * 3.0, (ij.shape[0], 1, 1))
    r, Ji, Jj, Om, i, j = PR.linearise(kind, P, ij, Z, om)
    Hii, Hjj, Hij, b = PR._blocks(kind, V, r, Ji, Jj, Om, i, j)
    b[fm] = 0.0
    a = PR._solve_banded(V, D, Hii, Hjj, Hij, i, j, b, fm, 0.25)
    d = PR._solve_dense(V, D, Hii, Hjj, Hij, i, j, b, fm, 0.25)
    assert np.max(np.abs(d)) > 1e-2
    assert np.max(np.abs(a - d)) <= 1e-10 * np.max(np.abs(d))
