"""-m gpu: the HIP pose-graph solve (block-sparse GN + multigrid-preconditioned CG, through the C ABI) against the CPU oracle
and against the SciPy golden fixture.  Dot-product order differs between the two PCGs, so this is a tolerance
test: poses within 1e-5 (BASELINE.json north_star: increments within 1e-5)."""
import os

import numpy as np
import pytest

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import posegraph as pgm
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _tight():
    p = pgm.default_params()
    p.pcg_tolerance = 1e-10
    p.pcg_max_iterations = 3000
    return p


@pytest.mark.parametrize("kind", [abi.SE3_QUAT_RIGHT, abi.SE2_RIGHT])
def test_matches_oracle(oracle, product, kind):
    g = syn.pose_graph_3d(V=300, E=1000, seed=21) if kind == abi.SE3_QUAT_RIGHT else syn.pose_graph_2d(V=400, E=900)
    ref = oracle.OraclePoseGraph(kind)
    gpu = product.PoseGraph(kind)
    for pg in (ref, gpu):
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
    sr, sg = ref.solve(_tight()), gpu.solve(_tight())
    assert len(sr) == len(sg) == 10
    for a, b in zip(sr, sg):
        assert a["num_factors"] == b["num_factors"] and a["solver_status"] == b["solver_status"] == 0
        assert abs(a["chi"] - b["chi"]) <= 1e-5 * max(a["chi"], 1e-12) + 1e-9
    assert np.max(np.abs(ref.poses() - gpu.poses())) <= 1e-5
    assert np.array_equal(gpu.poses()[0], g["poses_init"][0])  # Fixed variable untouched
    assert sg[-1]["chi"] < 0.2 * sg[0]["chi"]


@pytest.mark.parametrize("two_phase", [1, 0])
def test_se2_matches_oracle_on_a_four_level_hierarchy(oracle, product, two_phase):
    """3 000 SE(2) poses: 3 000 -> ~375 -> ~47 -> ~6 nodes, so the 3 x 3-block instances of the two-phase cycle kernels
    (k_mg_down2 / k_mg_up2 / k_mg_down2_coarsest: whole blocks per lane) all run; poses within 1e-5 of the oracle's
    block-Jacobi PCG.  two_phase = 0: the six-phase cycle with the unfused CG steps, the solver's only other cycle"""
    g = syn.pose_graph_2d(V=3000, E=9000)
    ref, gpu = oracle.OraclePoseGraph(abi.SE2_RIGHT), product.PoseGraph(abi.SE2_RIGHT)
    gpu.set_tuning(two_phase=two_phase)
    for pg in (ref, gpu):
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
    sr, sg = ref.solve(_tight()), gpu.solve(_tight())
    assert len(sr) == len(sg)
    assert all(s["solver_status"] == 0 for s in sg)
    assert np.max(np.abs(ref.poses() - gpu.poses())) <= 1e-5


def test_information_matrices_disabled_factors_fixed_mask(oracle, product):
    kind = abi.SE3_QUAT_RIGHT
    g = syn.pose_graph_3d(V=150, E=500, seed=22)
    E = g["ij"].shape[0]
    om = np.tile(np.eye(6, dtype=np.float32), (E, 1, 1))
    om[:149] *= 0.1  # Omega = I * info_scale (0.1 when lost, multi_graph_slam_impl.cpp:188)
    om[149:, 3:, 3:] *= 1e-3 * 1e3  # full 6x6 blocks go through
    om[200, 0, 1] = om[200, 1, 0] = 0.2
    en = np.ones(E, np.uint8)
    en[::7] = 0
    fm = np.zeros(150, np.uint8)
    fm[[0, 75]] = 1
    ref, gpu = oracle.OraclePoseGraph(kind), product.PoseGraph(kind)
    for pg in (ref, gpu):
        pg.set_graph(g["poses_init"], g["ij"], g["Z"], omega=om, fixed_mask=fm, enabled=en)
    sr, sg = ref.solve(_tight()), gpu.solve(_tight())
    assert sr[0]["num_factors"] == sg[0]["num_factors"] == int(en.sum())
    assert np.max(np.abs(ref.poses() - gpu.poses())) <= 1e-5
    assert np.array_equal(gpu.poses()[75], g["poses_init"][75])
    en2 = np.ones(E, np.uint8)
    for pg in (ref, gpu):
        pg.set_enabled(en2)
    sr, sg = ref.solve(_tight()), gpu.solve(_tight())
    assert sg[0]["num_factors"] == E and np.max(np.abs(ref.poses() - gpu.poses())) <= 1e-5


def test_matches_scipy_golden(product):
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_golden.npz"))
    g = syn.pose_graph_3d(V=100, E=300, seed=11)
    pg = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"])
    p = _tight()
    p.max_iterations = 1
    st = pg.solve(p)
    assert abs(st[0]["chi"] - float(G["chi0"])) / float(G["chi0"]) < 1e-4
    assert np.max(np.abs(pg.poses() - G["poses_after_1"])) < 1e-5


def test_matches_scipy_direct_solve_2k(oracle, product):
    """2 048 poses / 8 192 factors (a hierarchy of several levels): one Gauss-Newton step against the committed result
    of SciPy's sparse DIRECT solver on an independently assembled system (tests/golden/make_posegraph_golden.py);
    the oracle's block-Jacobi PCG is held to the same fixture."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_golden_2k.npz"))
    g = syn.pose_graph_3d(V=2048, E=8192, seed=12)
    p = _tight()
    p.max_iterations = 1
    p.pcg_max_iterations = 20000
    for pg in (product.PoseGraph(abi.SE3_QUAT_RIGHT), oracle.OraclePoseGraph(abi.SE3_QUAT_RIGHT)):
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
        st = pg.solve(p)
        assert st[0]["solver_status"] == 0 and st[0]["pcg_iterations"] < p.pcg_max_iterations
        assert abs(st[0]["chi"] - float(G["chi0"])) / float(G["chi0"]) < 1e-4
        # |dx| reaches 0.3: relative agreement 1e-4 (float32 poses, numerical Jacobians on the golden side)
        assert np.max(np.abs(pg.poses() - G["poses_after_1"])) < 1e-4 * max(1.0, float(G["max_abs_dx"])) + 2e-5


def test_se2_matches_scipy_direct_solve(product):
    """SE(2) -- what srrg2_laser_slam_2d optimises (S/mapping/local_map.h:64) -- 1 500 poses / ~4 500 factors, a hierarchy of
    several levels: two Gauss-Newton steps against the committed result of SciPy's sparse DIRECT solver on an independently
    assembled system (tests/golden/make_posegraph_golden_se2.py).  VERDICT r3 #6: SE(2) had the oracle as its only anchor."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_golden_se2.npz"))
    g = syn.pose_graph_2d(V=1500, E=4500, seed=5300)
    p = _tight()
    p.pcg_max_iterations = 20000
    for its, key, chi_key in ((1, "poses_after_1", "chi0"), (2, "poses_after_2", "chi1")):
        pg = product.PoseGraph(abi.SE2_RIGHT)
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
        p.max_iterations = its
        st = pg.solve(p)
        assert all(s["solver_status"] == 0 and s["pcg_iterations"] < p.pcg_max_iterations for s in st)
        assert abs(st[-1]["chi"] - float(G[chi_key])) / float(G[chi_key]) < 1e-4
        # |dx| reaches 0.97 on the first step: float32 poses, numerical Jacobians on the golden side
        assert np.max(np.abs(pg.poses() - G[key])) < 2e-5 * max(1.0, float(G["max_abs_dx"][0]))


def test_larger_graph_properties(product):
    """size-independent properties at a size the oracle would need seconds for: chi decreases monotonically to the
    noise floor, PCG converges within its budget, the optimum is near the ground truth."""
    g = syn.pose_graph_3d(V=5000, E=20000, seed=23)
    pg = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"])
    st = pg.solve()
    chis = [s["chi"] for s in st]
    assert all(s["solver_status"] == 0 and s["pcg_iterations"] < 200 and s["pcg_residual"] <= 1.01e-6 for s in st)
    assert chis[1] < chis[0] and chis[-1] <= chis[1] * 1.001
    # layers of the lawn-mower trajectory are only weakly tied together, so the optimum keeps part of the drift
    assert np.max(np.abs(pg.poses()[:, :, 3] - g["poses_gt"][:, :, 3])) < 0.6 * np.max(
        np.abs(g["poses_init"][:, :, 3] - g["poses_gt"][:, :, 3]))


def test_larger_se2_graph_properties(product):
    """the same size-independent properties for SE(2): 20 000 poses / 60 000 factors, every linear solve on tolerance
    within a few dozen multigrid-preconditioned CG iterations, chi monotone down to the noise floor"""
    g = syn.pose_graph_2d(V=20000, E=60000)
    pg = product.PoseGraph(abi.SE2_RIGHT)
    pg.set_graph(g["poses_init"], g["ij"], g["Z"])
    st = pg.solve()
    chis = [s["chi"] for s in st]
    assert all(s["solver_status"] == 0 and s["pcg_iterations"] < 150 and s["pcg_residual"] <= 1.01e-6 for s in st)
    assert all(b <= a * 1.0001 for a, b in zip(chis, chis[1:])) and chis[-1] < 0.02 * chis[0]


def test_hub_vertex_fill_guard(oracle, product, capfd, monkeypatch):
    """a pose with factors to every other pose (a place revisited all the time): the smoothed interpolation of that
    level would fill the Galerkin product quadratically in the hub's degree -- the hierarchy falls back to the tentative
    interpolation there (posegraph.hip: fill guard) and the solve still agrees with the oracle"""
    V = 3000
    g = syn.pose_graph_3d(V=V, E=V + 500, seed=29)
    gt = g["poses_gt"].astype(np.float64)
    hub_i = np.zeros(V - 2, dtype=np.int32)
    hub_j = np.arange(2, V, dtype=np.int32)
    Zh = np.stack([syn.se3_mul(syn.se3_inv(gt[0]), gt[j]) for j in hub_j]).astype(np.float32)
    ij = np.concatenate([g["ij"], np.stack([hub_i, hub_j], 1)]).astype(np.int32)
    Z = np.concatenate([g["Z"], Zh]).astype(np.float32)
    monkeypatch.setenv("SRRG2_AMD_PG_DEBUG", "1")
    ref = oracle.OraclePoseGraph(abi.SE3_QUAT_RIGHT)
    gpu = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    for pg in (ref, gpu):
        pg.set_graph(g["poses_init"], ij, Z, fixed_mask=(np.arange(V) == 1).astype(np.uint8))  # (the hub itself is free)
    p = _tight()
    sr, sg = ref.solve(p), gpu.solve(p)
    assert "tentative" in capfd.readouterr().err  # the guard fired on some level
    assert all(s["solver_status"] == 0 and s["pcg_residual"] <= 1.01e-10 for s in sg)
    assert abs(sr[-1]["chi"] - sg[-1]["chi"]) <= 1e-5 * max(sr[-1]["chi"], 1e-12) + 1e-9
    assert np.max(np.abs(ref.poses() - gpu.poses())) <= 1e-5


def test_pose_graph_misuse(product):
    with pytest.raises(RuntimeError):
        product.PoseGraph(abi.SE3_EULER_RIGHT)
    pg = product.PoseGraph(abi.SE2_RIGHT)
    with pytest.raises(RuntimeError):
        pg.set_graph(np.tile(np.eye(3, dtype=np.float32), (3, 1, 1)), np.array([[0, 5]], np.int32),
                     np.eye(3, dtype=np.float32)[None])


def test_tuning_struct_round_trip_and_kept_structure(product, monkeypatch):
    """srrg2_posegraph_tuning (ABI v4; the knobs were environment-only): defaults, round trip, the environment read once at
    create -- and a set() with the same topology keeps the hierarchy's structure: same poses, bit for bit, as a solve that
    rebuilds it, and as a fresh handle."""
    for name in ("SRRG2_AMD_PG_PASSES", "SRRG2_AMD_PG_OMEGA", "SRRG2_AMD_PG_OMEGA_P", "SRRG2_AMD_PG_LAG", "SRRG2_AMD_PG_GRAPH",
                 "SRRG2_AMD_PG_TWO_PHASE", "SRRG2_AMD_PG_KEEP_STRUCTURE", "SRRG2_AMD_PG_DEBUG"):
        monkeypatch.delenv(name, raising=False)
    kind = abi.SE3_QUAT_RIGHT
    pg = product.PoseGraph(kind)
    t = pg.tuning()
    assert (t.match_passes, t.two_phase, t.use_graph, t.debug, t.keep_structure) == (3, 1, 1, 0, 1)
    assert t.omega_p == pytest.approx(0.75) and t.omega == pytest.approx(0.8) and t.lag_below == pytest.approx(0.05)
    pg.set_tuning(match_passes=2, use_graph=0)
    t = pg.tuning()
    assert (t.match_passes, t.use_graph, t.two_phase) == (2, 0, 1)
    with pytest.raises(KeyError):
        pg.set_tuning(no_such_knob=1)
    with pytest.raises(Exception):
        pg.set_tuning(match_passes=0)
    monkeypatch.setenv("SRRG2_AMD_PG_PASSES", "4")
    assert pg.tuning().match_passes == 2  # (the environment is read once, at create)
    assert product.PoseGraph(kind).tuning().match_passes == 4
    monkeypatch.delenv("SRRG2_AMD_PG_PASSES")

    g = syn.pose_graph_3d(V=2000, E=7000, seed=23)

    def solved(pgx):
        pgx.set_graph(g["poses_init"], g["ij"], g["Z"])
        st = pgx.solve()
        assert all(s["solver_status"] == 0 for s in st)
        return pgx.poses().copy(), [s["pcg_iterations"] for s in st]

    fresh = solved(product.PoseGraph(kind))
    keep = product.PoseGraph(kind)
    first, second = solved(keep), solved(keep)  # the second solve reuses the structure the first one built
    keep.set_tuning(keep_structure=0)
    third = solved(keep)                        # ... the third rebuilds it
    for other in (first, second, third):
        assert other[1] == fresh[1]
        assert other[0].tobytes() == fresh[0].tobytes()
    # a different topology after a kept one: rebuilt, and right
    g2 = syn.pose_graph_3d(V=1500, E=5000, seed=24)
    keep.set_tuning(keep_structure=1)
    keep.set_graph(g2["poses_init"], g2["ij"], g2["Z"])
    keep.solve()
    ref2 = product.PoseGraph(kind)
    ref2.set_graph(g2["poses_init"], g2["ij"], g2["Z"])
    ref2.solve()
    assert keep.poses().tobytes() == ref2.poses().tobytes()


def _hub_graph(V=3000, seed=29):
    g = syn.pose_graph_3d(V=V, E=V + 500, seed=seed)
    gt = g["poses_gt"].astype(np.float64)
    hub_j = np.arange(2, V, dtype=np.int32)
    Zh = np.stack([syn.se3_mul(syn.se3_inv(gt[0]), gt[j]) for j in hub_j]).astype(np.float32)
    ij = np.concatenate([g["ij"], np.stack([np.zeros(V - 2, dtype=np.int32), hub_j], 1)]).astype(np.int32)
    return g["poses_init"], ij, np.concatenate([g["Z"], Zh]).astype(np.float32), (np.arange(V) == 1).astype(np.uint8)


@pytest.mark.parametrize("case", ["se3_four_levels", "se2", "hub_fill_guard", "plain_aggregation", "fixed_and_disabled"])
def test_device_built_structure_equals_the_host_built_one(product, case):
    """the hierarchy's sparsity patterns built on the device (sort + unique: `device_structure`, the default) are the arrays of
    the host build entry for entry, so the two solves agree BIT FOR BIT -- poses, chi, CG iteration counts -- on graphs with
    three coarse levels, in SE(2), with a hub that trips the fill guard, without smoothing, with Fixed variables and disabled
    factors"""
    kind, kw, tune = abi.SE3_QUAT_RIGHT, {}, {}
    if case == "se3_four_levels":
        g = syn.pose_graph_3d(V=6000, E=22000, seed=31)
        poses, ij, Z = g["poses_init"], g["ij"], g["Z"]
    elif case == "se2":
        kind = abi.SE2_RIGHT
        g = syn.pose_graph_2d(V=3000, E=8000, seed=32)
        poses, ij, Z = g["poses_init"], g["ij"], g["Z"]
    elif case == "hub_fill_guard":
        poses, ij, Z, fixed = _hub_graph()
        kw = {"fixed_mask": fixed}
    elif case == "plain_aggregation":
        g = syn.pose_graph_3d(V=2500, E=9000, seed=33)
        poses, ij, Z = g["poses_init"], g["ij"], g["Z"]
        tune = {"omega_p": 0.0}
    else:
        g = syn.pose_graph_3d(V=2500, E=9000, seed=34)
        poses, ij, Z = g["poses_init"], g["ij"], g["Z"]
        rng = np.random.default_rng(5)
        kw = {"fixed_mask": (rng.random(2500) < 0.02).astype(np.uint8) | (np.arange(2500) == 0).astype(np.uint8),
              "enabled": (rng.random(ij.shape[0]) < 0.9).astype(np.uint8)}
    out = []
    for device in (1, 0):
        pg = product.PoseGraph(kind)
        pg.set_tuning(device_structure=device, **tune)
        assert pg.tuning().device_structure == device
        pg.set_graph(poses, ij, Z, **kw)
        st = pg.solve()
        out.append((pg.poses().copy(), [s["pcg_iterations"] for s in st], [s["chi"] for s in st], [s["solver_status"] for s in st]))
    assert out[0][3] == out[1][3] and (case == "fixed_and_disabled" or all(c == 0 for c in out[0][3]))
    assert out[0][1] == out[1][1]
    assert out[0][2] == out[1][2]
    assert out[0][0].tobytes() == out[1][0].tobytes()


def test_device_structure_falls_back_to_the_host_build(product, monkeypatch, capfd):
    """a candidate list that would not fit 32-bit offsets sends the structure build back to the host (posegraph.hip:
    pg_device_patterns returns 2); forced here by lowering the limit (SRRG2_AMD_PG_OFFSET_LIMIT, read at create) below the
    size of level 1's lists: level 0's patterns come from the device, the rest from the host -- same arrays, same bits"""
    g = syn.pose_graph_3d(V=6000, E=22000, seed=31)
    ref = product.PoseGraph(abi.SE3_QUAT_RIGHT)
    ref.set_graph(g["poses_init"], g["ij"], g["Z"])
    sr = ref.solve()
    for limit in ("60000", "1000"):  # (level 0 has 50 000 slots: the first limit trips on its Q candidates, the second at once)
        monkeypatch.setenv("SRRG2_AMD_PG_OFFSET_LIMIT", limit)
        monkeypatch.setenv("SRRG2_AMD_PG_DEBUG", "1")
        pg = product.PoseGraph(abi.SE3_QUAT_RIGHT)
        monkeypatch.delenv("SRRG2_AMD_PG_OFFSET_LIMIT")
        monkeypatch.delenv("SRRG2_AMD_PG_DEBUG")
        assert pg.tuning().device_structure == 1
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
        st = pg.solve()
        assert "patterns on the host" in capfd.readouterr().err
        assert [s["pcg_iterations"] for s in st] == [s["pcg_iterations"] for s in sr]
        assert pg.poses().tobytes() == ref.poses().tobytes()
