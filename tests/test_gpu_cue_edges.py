"""GPU: the gated nearest-neighbour and given-correspondence slices on the cases of tests/test_oracle_cue_edges.py -- the
range cases, the ties, the sizes and half of the random configurations.  Every case runs once through compute() and once as
a batch of one (which hands out H); the run is the oracle's bit for bit and the first iteration is the float64 restatement's
(tests/cue_restatement.py) at the CPU module's tolerances.  One batch of three checks that every alignment of a batch keeps
its own fixed-point exponent."""
import numpy as np
import pytest

import cue_restatement as cr
from helpers import assert_same_run
from srrg2_slam_interfaces_amd import _abi as abi
from test_oracle_cue_edges import CASES, configure, refuse_degenerate_gate, restated, step_is_checked

pytestmark = pytest.mark.gpu


def _batch_of_one(al, case):
    """the same alignment as a batch of one: srrg2_batch_result::information is H of the last iteration"""
    normals = None if case["moving_normals"] is None else [case["moving_normals"]]
    if case["finder"] == cr.PAIRS:
        return al.compute_batch_correspondences([case["moving"]], [case["corr"]], [case["X"]], normals)
    return al.compute_batch([case["moving"]], [case["X"]], normals)


def check_device(oracle, product, name):
    case, fi, mi, resp, lin = restated(name)
    ref = configure(oracle.OracleAligner(case["kind"]), case)
    got = configure(product.MultiAligner(case["kind"]), case)
    ref.compute()
    got.compute()
    assert_same_run(ref, got)
    assert lin["max_scaled_term"] < 2.0 ** 51 and lin["max_scaled_sum"] < 2.0 ** 62
    c = got.correspondences(0)
    assert np.array_equal(c["fixed_idx"], fi) and np.array_equal(c["moving_idx"], mi)
    assert c["response"].tobytes() == resp.tobytes()
    st = got.iteration_stats()
    if len(fi) == 0:
        assert got.status() in (abi.NOT_ENOUGH_CORRESPONDENCES, abi.FAIL) and len(st) == 0
        return lin
    assert np.array_equal(got.factor_status(0), lin["status"])
    assert len(st) == 1
    s0 = st[0]
    for key in ("num_inliers", "num_outliers", "num_suppressed", "num_correspondences"):
        assert s0[key] == lin[key], (key, s0[key], lin[key])
    for key, n in (("chi_inliers", lin["num_inliers"]), ("chi_outliers", lin["num_outliers"])):
        assert abs(s0[key] - lin[key]) <= n * 2.0 ** (-lin["k"] - 1) + 1e-6 * lin[key], (key, s0[key], lin[key])
    X_run = got.moving_in_fixed()
    res = _batch_of_one(got, case)
    assert res[0]["status"] == got.status() and res[0]["moving_in_fixed"].tobytes() == X_run.tobytes()
    H = res[0]["information"]
    assert H.tobytes() == ref.information().tobytes()
    H64 = lin["H"]
    assert np.abs(H.astype(np.float64) - H64).max() <= 1e-6 * np.abs(H64).max() + 1e-300
    if s0["solver_status"] == 0 and step_is_checked(lin):
        X1 = cr.gauss_newton_step(case["kind"], case["X"], H64, lin["b"])
        assert np.abs(X_run.astype(np.float64) - X1).max() <= 1e-5
    return lin


@pytest.mark.parametrize("name", sorted(cr.RANGE_CASES))
def test_fixed_point_range(oracle, product, name):
    check_device(oracle, product, name)


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.split("_")[0] in ("lattice", "gate", "duplicate")))
def test_ties_and_the_gate(oracle, product, name):
    check_device(oracle, product, name)


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("size_")))
def test_sizes(oracle, product, name):
    check_device(oracle, product, name)


@pytest.mark.parametrize("seed", range(0, 24, 2))
def test_random_configurations(oracle, product, seed):
    check_device(oracle, product, "random_%d" % seed)


def test_batch_of_three_keeps_each_exponent(oracle, product):
    """one given-pair slice behind a sensor offset, three alignments: a far cloud, an ordinary one, an empty one"""
    kind = cr.QUAT
    base = cr.sensor_offset_case(kind, cr.P2P, 10.0)
    far = dict(base, moving=base["moving"] + np.float32(500.0))
    empty = dict(base, moving=np.zeros((0, 3), np.float32), corr=base["corr"][:0])
    items = [far, base, empty]
    lins = [cr.expected(c)[3] for c in items]
    assert lins[0]["k"] + 10 < lins[1]["k"]  # (with the ordinary cloud's exponent the far cloud's terms would leave the range)
    res = []
    for al in (oracle.OracleAligner(kind), product.MultiAligner(kind)):
        al.set_params(max_iterations=1, min_num_inliers=0)
        c = abi.default_slice_config(kind)
        c.kind, c.finder = cr.P2P, cr.PAIRS
        si = al.add_slice(c)
        al.set_sensor_in_robot(si, base["S"])
        al.set_fixed(si, base["fixed"], None)
        res.append(al.compute_batch_correspondences([c["moving"] for c in items], [c["corr"] for c in items],
                                                    [c["X"] for c in items]))
    r_ref, r_got = res
    assert np.array_equal(r_ref.status, r_got.status) and np.array_equal(r_ref.num_iterations, r_got.num_iterations)
    assert np.array_equal(r_ref.num_correspondences, r_got.num_correspondences)
    assert r_ref.moving_in_fixed.tobytes() == r_got.moving_in_fixed.tobytes()
    assert r_ref.information.tobytes() == r_got.information.tobytes()
    assert list(r_got.num_iterations) == [1, 1, 0] and r_got.status[2] in (abi.NOT_ENOUGH_CORRESPONDENCES, abi.FAIL)
    for k in (0, 1):
        lin = lins[k]
        assert lin["max_scaled_term"] < 2.0 ** 51 and lin["max_scaled_sum"] < 2.0 ** 62
        H = r_got[k]["information"].astype(np.float64)
        assert np.abs(H - lin["H"]).max() <= 1e-6 * np.abs(lin["H"]).max()
        last = r_got[k]["last"]
        assert last["num_inliers"] == lin["num_inliers"] == 200
        assert abs(last["chi_inliers"] - lin["chi_inliers"]) <= 200 * 2.0 ** (-lin["k"] - 1) + 1e-6 * lin["chi_inliers"]


@pytest.mark.parametrize("gate", [-0.25, float("inf"), float("nan")])
@pytest.mark.parametrize("finder", ["nn", "projective"])
def test_degenerate_gates_are_refused(product, gate, finder):
    """refused at add_slice, before any device work: nothing is launched here"""
    refuse_degenerate_gate(product.MultiAligner(cr.QUAT), gate, finder)
