"""Iteratively reweighted Gauss-Newton on the pose graph, restated over the unchanged CPU oracle: a GN step with weights w_e
is the plain GN step with information w_e * Omega_e.  Per iteration: chi_e = e^T Omega e from the oracle's edge(e) at the
current poses, w_e = w(chi_e) in numpy (the aligner's formula, include/srrg2_slam_amd.h), then one oracle GN iteration on
the graph with information w * Omega.  Used by tests/test_posegraph_robust_restatement.py (CPU) and
tests/test_gpu_posegraph_robust.py (the HIP solver against it)."""
import numpy as np

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import posegraph as pgm
from srrg2_slam_interfaces_amd import synthetic as syn


def information(kind, E):
    """Omega = diag(1e4 translation, 4e4 rotation) on every factor (the generators' sigma)"""
    d = [1e4, 1e4, 4e4] if kind == abi.SE2_RIGHT else [1e4] * 3 + [4e4] * 3
    return np.tile(np.diag(d).astype(np.float32), (E, 1, 1))


def weights(kinds, thrs, chi):
    """w(chi) per factor, in double: 1 below the threshold; CLAMP 0, SATURATED thr/chi, CAUCHY 1/(1+chi/thr) above it"""
    kinds = np.broadcast_to(np.asarray(kinds), chi.shape)
    thr = np.broadcast_to(np.asarray(thrs, np.float32).astype(np.float64), chi.shape)
    w = np.ones_like(chi)
    over = (kinds != abi.ROBUST_NONE) & (chi >= thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(over & (kinds == abi.ROBUST_CLAMP), 0.0, w)
        w = np.where(over & (kinds == abi.ROBUST_SATURATED), thr / chi, w)
        w = np.where(over & (kinds == abi.ROBUST_CAUCHY), 1.0 / (1.0 + chi / thr), w)
    return w


def factor_chi(pg, omega):
    """chi_e = e^T Omega e of every factor at the oracle graph's current poses (enabled or not)"""
    om = np.asarray(omega, np.float64)
    chi = np.zeros(pg.E)
    for e in range(pg.E):
        err = pg.edge(e)[0]
        chi[e] = err @ om[e] @ err
    return chi


def with_wrong_closures(kind, g, n_wrong, seed=3):
    """g plus n_wrong closures between far-apart poses whose measurement claims a short hop (a wrong place match); the
    wrong ones are the LAST n_wrong factor ids"""
    rng = np.random.default_rng(seed)
    V = g["poses_gt"].shape[0]
    pos = g["poses_gt"][:, :2, 2] if kind == abi.SE2_RIGHT else g["poses_gt"][:, :, 3]
    extent = np.max(np.linalg.norm(pos - pos.mean(0), axis=1))
    ij, Z = [], []
    while len(ij) < n_wrong:
        i, j = (int(x) for x in rng.integers(0, V, 2))
        if i == j or np.linalg.norm(pos[i] - pos[j]) < 0.5 * extent:
            continue
        if kind == abi.SE2_RIGHT:
            z = syn.se2(*(rng.normal(size=3) * [0.3, 0.3, 0.2]))
        else:
            t, r = rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.1
            z = syn.se3(t, r)
        ij.append((i, j))
        Z.append(z)
    out = dict(g)
    out["ij"] = np.concatenate([g["ij"], np.asarray(ij, np.int32)]).astype(np.int32)
    out["Z"] = np.concatenate([g["Z"], np.asarray(Z, np.float32)]).astype(np.float32)
    return out


def reweighted_gn(oracle, kind, poses, ij, Z, omega, kinds, thrs, iterations, enabled=None, pcg_max_iterations=3000):
    """iterations of iteratively reweighted GN through the oracle.  Returns (poses, raw chi per iteration -- sum of
    e^T Omega e over the enabled factors at that iteration's linearisation point --, chi and w per factor at the end)"""
    E = ij.shape[0]
    en = np.ones(E, bool) if enabled is None else np.asarray(enabled, bool)
    pg = oracle.OraclePoseGraph(kind)
    p = pgm.default_params()
    p.max_iterations, p.pcg_tolerance, p.pcg_max_iterations = 1, 1e-10, pcg_max_iterations
    P = np.asarray(poses, np.float32)
    chis = []
    for _ in range(iterations):
        pg.set_graph(P, ij, Z, omega=omega, enabled=enabled)
        chi = factor_chi(pg, omega)
        chis.append(float(np.sum(chi[en])))
        w = weights(kinds, thrs, chi)
        pg.set_graph(P, ij, Z, omega=(w[:, None, None] * np.asarray(omega, np.float64)).astype(np.float32), enabled=enabled)
        st = pg.solve(p)
        assert st[0]["solver_status"] == 0, st
        P = pg.poses().copy()
    pg.set_graph(P, ij, Z, omega=omega, enabled=enabled)
    chi = factor_chi(pg, omega)
    return P, chis, chi, weights(kinds, thrs, chi)


def max_position_error(kind, P, gt):
    if kind == abi.SE2_RIGHT:
        return float(np.max(np.linalg.norm(P[:, :2, 2] - gt[:, :2, 2], axis=1)))
    return float(np.max(np.linalg.norm(P[:, :, 3] - gt[:, :, 3], axis=1)))


def outlier_case(kind, n_wrong=20):
    """the issue's two graphs: SE(2) 400 / 900 and SE(3) 300 / 1000 (seed 21), plus n_wrong wrong closures"""
    g = syn.pose_graph_2d(V=400, E=900) if kind == abi.SE2_RIGHT else syn.pose_graph_3d(V=300, E=1000, seed=21)
    gw = with_wrong_closures(kind, g, n_wrong)
    return g, gw
