"""-m gpu: robust kernels on pose-graph factors (srrg2_posegraph_set_factor_robustifier / set_robustifiers /
evaluate_factors): the HIP solver's iteratively reweighted Gauss-Newton against its restatement over the unchanged oracle
(tests/posegraph_robust_restatement.py), per-factor chi readback, the lifecycle, misuse, and C5 with corrupted closures."""
import ctypes as C

import numpy as np
import pytest

import posegraph_restatement as PR
import posegraph_robust_restatement as R
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import posegraph as pgm
from srrg2_slam_interfaces_amd import synthetic as syn
from srrg2_slam_interfaces_amd.graph_slam import GraphSLAMLifecycle

pytestmark = pytest.mark.gpu

E_INVALID = -1
KINDS = [abi.SE2_RIGHT, abi.SE3_QUAT_RIGHT]


def _tight(iterations=10):
    p = pgm.default_params()
    p.max_iterations = iterations
    p.pcg_tolerance = 1e-10
    p.pcg_max_iterations = 3000
    return p


def _graph(kind):
    return syn.pose_graph_2d(V=400, E=900) if kind == abi.SE2_RIGHT else syn.pose_graph_3d(V=300, E=1000, seed=21)


def _raw(product):
    from srrg2_slam_interfaces_amd import _capi

    return _capi.lib()


@pytest.mark.parametrize("kind", KINDS)
def test_explicit_none_is_bit_identical_to_an_untouched_handle(product, kind):
    g = _graph(kind)
    E = g["ij"].shape[0]
    om = R.information(kind, E)
    a, b = product.PoseGraph(kind), product.PoseGraph(kind)
    for pg in (a, b):
        pg.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om)
    for e in range(0, E, 7):
        b.set_factor_robustifier(e, abi.ROBUST_NONE, 0.0)
    b.set_robustifiers(np.zeros(E, np.int32), np.zeros(E, np.float32))
    sa, sb = a.solve(), b.solve()
    assert sa == sb
    assert np.array_equal(a.poses(), b.poses())
    # a robustifier set and taken back again: the plain path again
    b.set_factor_robustifier(3, abi.ROBUST_CAUCHY, 1.0)
    b.set_factor_robustifier(3, abi.ROBUST_NONE, 0.0)
    sa, sb = a.solve(), b.solve()
    assert sa == sb and np.array_equal(a.poses(), b.poses())


@pytest.mark.parametrize("iterations", [1, 3, 10])
@pytest.mark.parametrize("rk", [abi.ROBUST_CLAMP, abi.ROBUST_SATURATED, abi.ROBUST_CAUCHY])
@pytest.mark.parametrize("kind", KINDS)
def test_reweighted_gn_matches_the_restatement(oracle, product, kind, rk, iterations):
    g, gw = R.outlier_case(kind)
    E = gw["ij"].shape[0]
    om = R.information(kind, E)
    kinds = np.full(E, rk, np.int32)
    thrs = np.full(E, 100.0, np.float32)
    P, chis, _, _ = R.reweighted_gn(oracle, kind, gw["poses_init"], gw["ij"], gw["Z"], om, kinds, thrs, iterations)
    pg = product.PoseGraph(kind)
    pg.set_graph(gw["poses_init"], gw["ij"], gw["Z"], omega=om)
    pg.set_robustifiers(kinds, thrs)
    st = pg.solve(_tight(iterations))
    assert len(st) == iterations and all(s["solver_status"] == 0 for s in st)
    assert np.max(np.abs(pg.poses() - P)) <= 1e-5
    for s, c in zip(st, chis):  # raw chi, not the weighted one
        assert abs(s["chi"] - c) <= 1e-5 * c, (s["chi"], c)


@pytest.mark.parametrize("kind", KINDS)
def test_outlier_story_on_the_gpu(product, kind):
    g, gw = R.outlier_case(kind)
    E0, E = g["ij"].shape[0], gw["ij"].shape[0]
    p = pgm.default_params()
    p.max_iterations = 15
    clean = product.PoseGraph(kind)
    clean.set_graph(g["poses_init"], g["ij"], g["Z"], omega=R.information(kind, E0))
    clean.solve(p)
    e_clean = R.max_position_error(kind, clean.poses(), g["poses_gt"])
    plain = product.PoseGraph(kind)
    plain.set_graph(gw["poses_init"], gw["ij"], gw["Z"], omega=R.information(kind, E))
    plain.solve(p)
    assert R.max_position_error(kind, plain.poses(), g["poses_gt"]) > 1.0
    for rk in (abi.ROBUST_CAUCHY, abi.ROBUST_SATURATED):
        pg = product.PoseGraph(kind)
        pg.set_graph(gw["poses_init"], gw["ij"], gw["Z"], omega=R.information(kind, E))
        pg.set_robustifiers(np.full(E, rk, np.int32), np.full(E, 100.0, np.float32))
        st = pg.solve(p)
        assert all(s["solver_status"] == 0 for s in st)
        assert R.max_position_error(kind, pg.poses(), g["poses_gt"]) <= 1.5 * e_clean
        chi, w = pg.evaluate_factors()
        assert np.array_equal(np.flatnonzero(w < 0.5), np.arange(E0, E)), np.flatnonzero(w < 0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_factors_enabled_disabled_removed(product, kind):
    """against e^T Omega e of the float64 restatement at the poses read back: the read-back forms its residual in double
    (edge_error_f64), where the oracle, like the solver, rounds three transforms to float32 -- 0.8 % of a chi on this SE(2)
    graph, whose coordinates reach hundreds of metres"""
    g = _graph(kind)
    E = g["ij"].shape[0]
    om = R.information(kind, E)
    en = np.ones(E, np.uint8)
    en[::5] = 0
    pg = product.PoseGraph(kind)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om, enabled=en)
    pg.solve(pgm.default_params())
    kinds = np.zeros(E, np.int32)
    thrs = np.zeros(E, np.float32)
    kinds[1::3], thrs[1::3] = abi.ROBUST_CAUCHY, 5.0
    kinds[2::3], thrs[2::3] = abi.ROBUST_CLAMP, 8.0
    pg.set_robustifiers(kinds, thrs)
    pg.set_factor_robustifier(4, abi.ROBUST_SATURATED, 3.0)
    kinds[4], thrs[4] = abi.ROBUST_SATURATED, 3.0
    removed = [10, 11, 500]
    for e in removed:
        pg.remove_factor(e)
    P0 = pg.poses().copy()
    chi, w = pg.evaluate_factors()
    assert np.array_equal(pg.poses(), P0)  # changes nothing
    r, _, _, Om, _, _ = PR.linearise(kind, P0, g["ij"], g["Z"], om)
    chi_ref = np.einsum("ea,eab,eb->e", r, Om, r)
    kinds[removed] = abi.ROBUST_NONE
    w_ref = R.weights(kinds, thrs, chi_ref)
    live = np.setdiff1d(np.arange(E), removed)
    assert np.all(np.abs(chi[live] - chi_ref[live]) <= 1e-6 * chi_ref[live] + 1e-12)
    assert np.allclose(w[live], w_ref[live], rtol=1e-6, atol=0)
    assert np.isnan(chi[removed]).all() and np.array_equal(w[removed], np.zeros(len(removed), np.float32))
    assert (en[live] == 0).any() and np.isfinite(chi[live][en[live] == 0]).all()  # disabled (pending) factors are evaluated
    assert (w[live] < 1).any() and (w[live] == 0).any()
    assert pg.size()[1] == E - len(removed)


def _hom(T):
    return T if T.shape[0] == T.shape[1] else np.vstack([T, [0, 0, 0, 1]])


def _leaf_run(product, kind, keep_structure, g, om, n_leaves, rk):
    pg = product.PoseGraph(kind)
    pg.set_tuning(keep_structure=keep_structure)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om)
    p = _tight(3)
    pg.solve(p)
    rng = np.random.default_rng(11)
    V = g["poses_init"].shape[0]
    for k in range(n_leaves):
        parent = V - 1 + k if k % 2 == 0 else int(rng.integers(0, V))
        P = pg.poses()
        Z = syn.se2(0.5, 0.1, 0.05) if kind == abi.SE2_RIGHT else syn.se3([0.5, 0.1, 0.0], [0.0, 0.0, 0.05])
        guess = (_hom(P[parent]) @ _hom(Z))[:3]
        guess[0, -1] += 0.3  # a leaf factor with a large chi at the first linearisation: its weight is far from 1
        vid = pg.add_variable(guess.astype(np.float32))
        pg.add_factor(parent, vid, Z.astype(np.float32), om[0], robustifier=(rk, 100.0))
    st = pg.solve(p)
    return pg, st


@pytest.mark.parametrize("kind", KINDS)
def test_robustified_leaves_are_eliminated_and_match_a_rebuild(product, kind):
    g = _graph(kind)
    om = R.information(kind, g["ij"].shape[0])
    for rk in (abi.ROBUST_CAUCHY, abi.ROBUST_SATURATED):
        a, sa = _leaf_run(product, kind, 1, g, om, 6, rk)
        b, sb = _leaf_run(product, kind, 0, g, om, 6, rk)
        assert a.structure_info()[1] == 6 and b.structure_info()[1] == 0
        assert all(s["solver_status"] == 0 for s in sa + sb)
        assert np.max(np.abs(a.poses() - b.poses())) <= 1e-5
        chi, w = a.evaluate_factors()
        assert np.isfinite(chi).all()


@pytest.mark.parametrize("kind", KINDS)
def test_changing_robustifiers_keeps_the_hierarchy(product, kind):
    g = _graph(kind)
    E = g["ij"].shape[0]
    pg = product.PoseGraph(kind)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"], omega=R.information(kind, E))
    pg.solve(_tight(2))
    builds = pg.structure_info()[0]
    pg.set_factor_robustifier(E - 1, abi.ROBUST_CAUCHY, 100.0)
    pg.solve(_tight(2))
    pg.set_robustifiers(np.full(E, abi.ROBUST_SATURATED, np.int32), np.full(E, 50.0, np.float32))
    st = pg.solve(_tight(2))
    pg.set_robustifiers(None)
    st += pg.solve(_tight(2))
    assert pg.structure_info()[0] == builds
    assert all(s["solver_status"] == 0 and s["pcg_residual"] <= 1.01e-10 for s in st)


@pytest.mark.parametrize("kind", KINDS)
def test_lifecycle_with_closure_robustifier_survives_wrong_closures(product, kind):
    g, gw = R.outlier_case(kind)
    V = g["poses_gt"].shape[0]
    E0, E = g["ij"].shape[0], gw["ij"].shape[0]
    info = R.information(kind, 1)[0]
    closures = [(int(gw["ij"][e, 0]), int(gw["ij"][e, 1]), gw["Z"][e], info) for e in range(V - 1, E)]
    p = pgm.default_params()
    p.max_iterations = 15

    def run(batch, robustifier):
        life = GraphSLAMLifecycle(product.PoseGraph(kind), default_information=info, closure_robustifier=robustifier)
        life.make_new_map(g["poses_init"][0], syn.identity(2 if kind == abi.SE2_RIGHT else 3))
        for v in range(1, V):
            life.make_new_map(g["poses_init"][v], g["Z"][v - 1])
        accepted = life.loop_validate(batch)
        st = life.optimize(p)
        return life, accepted, st

    clean, _, _ = run(closures[:E0 - (V - 1)], None)
    e_clean = R.max_position_error(kind, clean.graph.poses(), g["poses_gt"])
    life, accepted, st = run(closures, (abi.ROBUST_CAUCHY, 100.0))
    assert len(accepted) == E - (V - 1) and all(s["solver_status"] == 0 for s in st)
    assert R.max_position_error(kind, life.graph.poses(), g["poses_gt"]) <= 1.5 * e_clean
    cw = life.closure_weights()
    assert sorted(cw) == accepted
    low = sorted(fid for fid, (chi, w) in cw.items() if w < 0.5)
    assert low == list(range(E0, E))  # the wrong closures, by factor id


@pytest.mark.parametrize("kind", KINDS)
def test_singular_clamp_and_misuse(oracle, product, kind):
    lib = _raw(product)
    g = _graph(kind)
    E = g["ij"].shape[0]
    V = g["poses_init"].shape[0]
    om = R.information(kind, E)
    # CLAMP weights every factor of a free variable 0: its block is singular -> solver_status 1, poses untouched and finite
    pg = product.PoseGraph(kind)
    P = g["poses_init"].copy()
    v = V // 2
    P[v, 0, -1] += 5.0
    pg.set_graph(P, g["ij"], g["Z"], omega=om)
    incident = np.flatnonzero((g["ij"][:, 0] == v) | (g["ij"][:, 1] == v))
    for e in incident:
        pg.set_factor_robustifier(int(e), abi.ROBUST_CLAMP, 1.0)
    st = pg.solve(_tight(3))
    assert st[0]["solver_status"] == 1 and len(st) == 1
    assert np.isfinite(pg.poses()).all() and np.array_equal(pg.poses(), P)
    _, w = pg.evaluate_factors()
    assert np.array_equal(np.flatnonzero(w == 0), incident)
    # misuse: SRRG2_E_INVALID, the handle unchanged
    pg2 = product.PoseGraph(kind)
    pg2.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om)
    pg2.remove_factor(7)
    h = pg2._h
    fn = lib.srrg2_posegraph_set_factor_robustifier
    for fid, k, thr in ((-1, abi.ROBUST_CAUCHY, 1.0), (E, abi.ROBUST_CAUCHY, 1.0), (7, abi.ROBUST_CAUCHY, 1.0),
                        (0, 4, 1.0), (0, -1, 1.0), (0, abi.ROBUST_CAUCHY, 0.0), (0, abi.ROBUST_CLAMP, -1.0),
                        (0, abi.ROBUST_SATURATED, float("inf")), (0, abi.ROBUST_CAUCHY, float("nan"))):
        assert fn(h, C.c_int(fid), C.c_int(k), C.c_float(thr)) == E_INVALID, (fid, k, thr)
    kinds = np.full(E, abi.ROBUST_CAUCHY, np.int32)
    thrs = np.full(E, 1e-6, np.float32)
    thrs[E - 1] = 0.0
    assert lib.srrg2_posegraph_set_robustifiers(h, kinds.ctypes.data_as(C.POINTER(C.c_int32)),
                                                thrs.ctypes.data_as(C.POINTER(C.c_float))) == E_INVALID
    assert lib.srrg2_posegraph_set_robustifiers(h, kinds.ctypes.data_as(C.POINTER(C.c_int32)), None) == E_INVALID
    assert lib.srrg2_posegraph_evaluate_factors(h, None, None) == E_INVALID
    with pytest.raises(RuntimeError):
        pg2.set_factor_robustifier(E + 3, abi.ROBUST_CAUCHY, 1.0)
    _, w = pg2.evaluate_factors()
    assert np.all(w[np.arange(E) != 7] == 1.0)  # nothing was applied
    en = np.ones(E, np.uint8)
    en[7] = 0
    ref = oracle.OraclePoseGraph(kind)
    ref.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om, enabled=en)
    sr, sg = ref.solve(_tight()), pg2.solve(_tight())
    assert all(s["solver_status"] == 0 for s in sg)
    assert np.max(np.abs(ref.poses() - pg2.poses())) <= 1e-5


def _corrupted_c5(fraction=0.005, seed=7):
    V = 50_000
    g = syn.pose_graph_3d(V=V, E=200_000, seed=5000)
    Et = g["ij"].shape[0]
    loop = np.arange(V - 1, Et)
    rng = np.random.default_rng(seed)
    bad = np.sort(rng.choice(loop, size=int(round(fraction * loop.size)), replace=False))
    Z = g["Z"].copy()
    for e in bad:
        off = syn.se3(rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.2)
        Z[e] = (off @ np.vstack([Z[e], [0, 0, 0, 1]]))[:3].astype(np.float32)
    return g, Z, loop, bad


def test_c5_full_size_cauchy_on_corrupted_closures(product):
    """C5 (50 000 SE(3) poses, 200 000 factors, Omega = I) with 0.5 % of its loop closures corrupted (0.5 m, 0.2 rad):
    CAUCHY (thr 0.01: ~30 x a correct closure's mean chi) on every loop closure keeps the map within 1.5 x the error of the
    plain solve of the clean graph; every linear solve reaches its tolerance.  The first iteration linearises at the drifted
    odometry guess, where nearly every closure is down-weighted: its CG needs more than the default 600 iterations
    ("Robust kernels"), so the cap is raised."""
    g, Z, loop, bad = _corrupted_c5()
    Et = g["ij"].shape[0]
    p = pgm.default_params()
    clean = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    clean.set_graph(g["poses_init"], g["ij"], g["Z"])
    clean.solve(p)
    e_clean = R.max_position_error(abi.SE3_QUAT_RIGHT, clean.poses(), g["poses_gt"])
    kinds = np.zeros(Et, np.int32)
    kinds[loop] = abi.ROBUST_CAUCHY
    p.pcg_max_iterations = 5000
    pg = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    pg.set_graph(g["poses_init"], g["ij"], Z)
    pg.set_robustifiers(kinds, np.full(Et, 0.01, np.float32))
    st = pg.solve(p)
    assert len(st) == p.max_iterations and all(s["solver_status"] == 0 for s in st)
    assert all(s["pcg_iterations"] < p.pcg_max_iterations and s["pcg_residual"] <= 1.01e-6 for s in st), st
    err = R.max_position_error(abi.SE3_QUAT_RIGHT, pg.poses(), g["poses_gt"])
    assert err <= 1.5 * e_clean, (err, e_clean)
    _, w = pg.evaluate_factors()
    assert (w[bad] < 0.5).all()
