"""-m gpu: the planned tiles of the list-search pass (search_plan.h; kernels.hip: cnl_pass_tiles) -- launches of up to four
alignments deal their points over tiles of four, two and one lane per point so that the launch fits the workgroups resident
together.  `search_team` = ceiling on the lanes | (assumed resident workgroups << 8): a small capacity forces all three tile
classes on a 1000-point cloud.  A team only splits which lane examines which candidate, so everything stays bit for bit the
oracle's: indices, X, statistics, H -- on the first compute() of a handle (prologue launch) and on the second (prologue in
the first pass, which then has one workgroup more and the plan one fewer)."""
import numpy as np
import pytest

from helpers import assert_same_run, cue_config, prior_config, setup_pair
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# lists from the first compute() on, fused control steps, no one-workgroup kernel for small clouds: every search pass is the
# list-search kernel
BASE = {"search_lists": 2, "fused_control": 1, "small_max_points": 0}
BIG = 1 << 20


def team(lanes, capacity=0):
    return lanes | (capacity << 8)


# (lanes, capacity): 1000 points on 6 workgroups = 2 + 1 + 3 tiles (the last one partial), on 7 = the same behind the prologue's
# workgroup; capacity 1 = the one-lane fallback; a large one = every tile at four lanes; uniform two lanes
PLANS = [team(4, 6), team(4, 7), team(4, 1), team(4, BIG), team(2, BIG), team(2, 6)]


def _cut(d, keep=0.6):
    """the fixed cloud cut to ~60 % of the scene: many moving points have nothing within the gate"""
    m = d["fixed"][:, 0] <= np.quantile(d["fixed"][:, 0], keep)
    out = dict(d)
    out["fixed"], out["fixed_normals"] = d["fixed"][m], d["fixed_normals"][m]
    return out


@pytest.fixture(scope="module")
def pair3d():
    return _cut(syn.cloud_pair_3d(n=1000, seed=6100, t=(0.03, -0.02, 0.01), rpy_deg=(0.5, -0.6, 0.8)))


@pytest.fixture(scope="module")
def pair2d():
    return _cut(syn.scan_pair_2d(beams=1000, sigma=0.005, seed=6200))


def _twice(al, ref):
    """two compute()s on one handle against one oracle run; the second one carries the prologue in its first pass"""
    for k in range(2):
        al.set_moving_in_fixed(syn.identity(al.dim))
        al.compute()
        assert_same_run(ref, al)
        assert al.information().tobytes() == ref.information().tobytes()
        path = al.last_compute_path()
        assert path & abi.PATH_FUSED_CONTROL, (k, path)
        assert bool(path & abi.PATH_PROLOGUE_IN_PASS) == (k > 0), (k, path)


def _reference(oracle, kind, d, cfg, iterations=8):
    ref = oracle.OracleAligner(kind)
    ref.set_params(max_iterations=iterations)
    setup_pair(ref, d, cfg)
    ref.compute()
    return ref


@pytest.fixture(scope="module")
def ref3d(oracle, pair3d):
    cfg = cue_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, 0.6, abi.ROBUST_CAUCHY, 0.05, 0.7)
    ref = _reference(oracle, abi.SE3_QUAT_RIGHT, pair3d, cfg)
    assert ref.status() == abi.SUCCESS
    assert 300 < ref.num_correspondences() < 800  # (partial overlap: many points without a match)
    return cfg, ref


@pytest.fixture(scope="module")
def ref2d(oracle, pair2d):
    cfg = cue_config(abi.SE2_RIGHT, abi.SLICE_P2P, 0.5, abi.ROBUST_CAUCHY, 0.01)
    ref = _reference(oracle, abi.SE2_RIGHT, pair2d, cfg)
    assert ref.status() == abi.SUCCESS
    assert 300 < ref.num_correspondences() < 900
    return cfg, ref


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("all_passes_search", [False, True])
def test_planned_tiles_3d_point_to_plane(product, pair3d, ref3d, plan, all_passes_search):
    cfg, ref = ref3d
    al = product.MultiAligner(abi.SE3_QUAT_RIGHT)
    # (fast_from_iteration beyond the run: every pass is a search pass on the planned kernel, control steps inside)
    al.set_tuning(search_team=plan, **(dict(BASE, fast_from_iteration=100) if all_passes_search else BASE))
    al.set_params(max_iterations=8)
    setup_pair(al, pair3d, cfg)
    _twice(al, ref)


@pytest.mark.parametrize("plan", PLANS)
def test_planned_tiles_2d_point_to_point(product, pair2d, ref2d, plan):
    cfg, ref = ref2d
    al = product.MultiAligner(abi.SE2_RIGHT)
    al.set_tuning(search_team=plan, **dict(BASE, fast_from_iteration=100))
    al.set_params(max_iterations=8)
    setup_pair(al, pair2d, cfg)
    _twice(al, ref)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_point_counts_at_the_tile_edges(oracle, product, pair3d, n):
    """one point; one full four-lane tile; one point more; one point more than a one-lane tile -- on 3 workgroups (257 points:
    2 + 0 + 1 tiles) and on the device's own capacity"""
    kind = abi.SE3_QUAT_RIGHT
    d = dict(pair3d)
    d["moving"], d["moving_normals"] = pair3d["moving"][:n], pair3d["moving_normals"][:n]
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.6, abi.ROBUST_CAUCHY, 0.05, 0.7)
    ref = oracle.OracleAligner(kind)
    ref.set_params(max_iterations=5, min_num_inliers=1)
    setup_pair(ref, d, cfg)
    ref.compute()
    for plan in (team(4, 3), team(4), team(2, 2), 0):
        al = product.MultiAligner(kind)
        al.set_tuning(search_team=plan, **dict(BASE, fast_from_iteration=100))
        al.set_params(max_iterations=5, min_num_inliers=1)
        setup_pair(al, d, cfg)
        _twice(al, ref)


@pytest.mark.parametrize("plan", [team(4, 6), team(2, 7)])
def test_termination_criterion_and_inlier_only_run(oracle, product, pair3d, plan):
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.6, abi.ROBUST_CAUCHY, 0.002)

    def build(al):
        al.set_params(max_iterations=12, min_num_inliers=10, enable_inlier_only_runs=True, keep_only_inlier_correspondences=True)
        al.set_termination_criteria(abi.default_termination_params())
        setup_pair(al, pair3d, cfg)

    ref = oracle.OracleAligner(kind)
    build(ref)
    ref.compute()
    assert ref.status() == abi.SUCCESS
    al = product.MultiAligner(kind)
    al.set_tuning(search_team=plan, **dict(BASE, fast_from_iteration=100))
    build(al)
    _twice(al, ref)


@pytest.mark.parametrize("plan", [team(4, 6), team(2, 6), team(4, BIG)])
def test_prior_slice_next_to_the_cue_slice(oracle, product, pair3d, plan):
    """the control wave linearises the prior (the passes' FUSED = 2 instantiation from the second pass on)"""
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.6, abi.ROBUST_CAUCHY, 0.05, 0.7)
    Z = syn.se3(np.array([0.03, -0.02, 0.01]), np.deg2rad([0.5, -0.6, 0.8])).astype(np.float32)

    def build(al):
        al.set_params(max_iterations=8)
        setup_pair(al, pair3d, cfg)
        pi = al.add_slice(prior_config(kind, info=[50, 50, 50, 500, 500, 500], sets_guess=0))
        al.set_prior_measurement(pi, Z)

    ref = oracle.OracleAligner(kind)
    build(ref)
    ref.compute()
    assert ref.status() == abi.SUCCESS
    al = product.MultiAligner(kind)
    al.set_tuning(search_team=plan, **dict(BASE, fast_from_iteration=100))
    build(al)
    for k in range(2):
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()
        assert_same_run(ref, al)
        assert al.information().tobytes() == ref.information().tobytes()
        assert al.last_compute_path() & abi.PATH_PRIORS_FUSED, al.last_compute_path()


@pytest.mark.parametrize("plan", [team(4, 18), team(4, 21), team(2, BIG), team(4, 3), 0])
def test_batch_of_three_unequal_clouds_one_empty(oracle, product, pair3d, plan):
    """three alignments per launch share the plan of the largest cloud: 6 tiles each on 18 workgroups"""
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.6, abi.ROBUST_CAUCHY, 0.05, 0.7)
    movs = [pair3d["moving"], pair3d["moving"][:0], pair3d["moving"][:700]]
    nrms = [pair3d["moving_normals"], pair3d["moving_normals"][:0], pair3d["moving_normals"][:700]]

    def run(al, times):
        al.set_params(max_iterations=6)
        al.add_slice(cfg)
        al.set_fixed(0, pair3d["fixed"], pair3d["fixed_normals"])
        return [al.compute_batch(movs, [syn.identity(3)] * 3, nrms) for _ in range(times)]

    want = run(oracle.OracleAligner(kind), 1)[0]
    assert [r["status"] for r in want] == [abi.SUCCESS, abi.FAIL, abi.SUCCESS]
    al = product.MultiAligner(kind)
    al.set_tuning(search_team=plan, **dict(BASE, fast_from_iteration=100))
    for got in run(al, 2):
        for r, g in zip(want, got):
            assert r["status"] == g["status"] and r["num_iterations"] == g["num_iterations"]
            assert r["moving_in_fixed"].tobytes() == g["moving_in_fixed"].tobytes()
            assert r["last"] == g["last"] and r["num_correspondences"] == g["num_correspondences"]
            assert np.asarray(r["information"]).tobytes() == np.asarray(g["information"]).tobytes()


def test_negative_search_team_is_refused(product):
    al = product.MultiAligner(abi.SE3_QUAT_RIGHT)
    with pytest.raises(Exception):
        al.set_tuning(search_team=-1)
    assert al.tuning().search_team == 0
