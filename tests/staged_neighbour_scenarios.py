"""Scenarios for the staged neighbours of the converged passes (csrc/kernels.hip, icp_step_fast_body: the lanes whose exclusion
margin is nearly used up gather the ball of their previous neighbour while the record is waited for, and choose among the kept
candidates once the new transform is there).  Shared by tests/test_gpu_staged_neighbours.py (product library) and
tests/helpers_scripts/staged_neighbours_check.py (the -DSRRG2_FUSED_STALL build, whose counters prove which way a point went).

Clouds of 3 000 points: above the one-workgroup kernel's 1 024, 12 workgroups of 256, the last one not full."""
import numpy as np

from helpers import assert_same_run, cue_config, setup_pair
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

N = 3000
FUSED = {"search_lists": 2, "fused_control": 1}    # lists (hence the fused launches) from the first compute() on
UNFUSED = {"search_lists": 2, "fused_control": 0}


def _tangent(normals):
    """a unit vector orthogonal to every normal (any dimension >= 2)"""
    n = np.asarray(normals, np.float64)
    if n.shape[1] == 2:
        return np.stack([-n[:, 1], n[:, 0]], axis=1)
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t = np.cross(n, a)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def _apply(X, P):
    dim = P.shape[1]
    X = np.asarray(X, np.float64)
    return P.astype(np.float64) @ X[:dim, :dim].T + X[:dim, dim]


def _two_nearest(Q, F):
    d = np.sqrt(((Q[:, None, :] - F[None, :, :].astype(np.float64)) ** 2).sum(-1))
    idx = np.argsort(d, axis=1)[:, :2]
    two = np.take_along_axis(d, idx, axis=1)
    return idx[:, 0], two[:, 0], two[:, 1]


def pair(dim):
    if dim == 2:
        d = syn.scan_pair_2d(beams=N, sigma=0.0, seed=1234)
        d = {k: np.array(v, np.float32) for k, v in d.items()}
        for which in ("fixed", "moving"):  # (the scans' own normals, from neighbouring beams)
            p = d[which]
            t = np.roll(p, -1, axis=0) - np.roll(p, 1, axis=0)
            n = np.stack([-t[:, 1], t[:, 0]], axis=1)
            d[which + "_normals"] = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)).astype(np.float32)
        return d
    return {k: v.copy() for k, v in syn.cloud_pair_3d(n=N, seed=2600).items()}


def with_twins(d, count=64, exact=16):
    """`count` fixed points -- nearest neighbours of moving points at the ground truth -- get a twin at f + delta t along a surface
    tangent: delta = 0 for `exact` of them (equal distance bits: the index decides), 1e-7 .. 1e-4 m for the rest (the nearer twin
    can change between passes: the runner-up becomes the neighbour).  Returns the data and how many moving points have
    (d2 - d1) / d1 < 3e-5 at the ground truth."""
    d = dict(d)
    Q = _apply(d["X_gt"], d["moving"])
    nn, _, _ = _two_nearest(Q, d["fixed"])
    who, users = np.unique(nn, return_counts=True)
    sel = who[np.argsort(-users, kind="stable")][:count]  # (the fixed points most moving points look at first: they get delta = 0)
    assert len(sel) == count
    delta = np.concatenate([np.zeros(exact), np.logspace(-7, -4, count - exact)])
    tw = d["fixed"][sel].astype(np.float64) + delta[:, None] * _tangent(d["fixed_normals"][sel])
    d["fixed"] = np.ascontiguousarray(np.concatenate([d["fixed"], tw.astype(np.float32)]))
    d["fixed_normals"] = np.ascontiguousarray(np.concatenate([d["fixed_normals"], d["fixed_normals"][sel]]))
    _, d1, d2 = _two_nearest(Q, d["fixed"])
    return d, int(np.sum((d2 - d1) < 3e-5 * d1))


def with_clumps(d, clumps=8, size=80):
    """`size` fixed points within 1e-3 m of each other at the neighbour of a moving point: a ball that holds more candidates than a
    team keeps (STAGE_CAP = 64).  (Within 1e-5 m in fact, a few float32 steps of the coordinates: the nearest two of a clump stay
    closer than the certificate's safety factors resolve, so the point's certificate fails in every pass, converged or not.)"""
    d = dict(d)
    Q = _apply(d["X_gt"], d["moving"])
    nn, _, _ = _two_nearest(Q, d["fixed"])
    sel = np.unique(nn)[:: max(1, len(np.unique(nn)) // clumps)][:clumps]
    dim = d["fixed"].shape[1]
    off = np.stack([syn.uniform(77 + a, len(sel) * (size - 1), -2e-6, 2e-6) for a in range(dim)], axis=1)
    extra = np.repeat(d["fixed"][sel].astype(np.float64), size - 1, axis=0) + off
    assert np.max(np.abs(off)) * 2 * np.sqrt(dim) < 1e-3
    d["fixed"] = np.ascontiguousarray(np.concatenate([d["fixed"], extra.astype(np.float32)]))
    d["fixed_normals"] = np.ascontiguousarray(np.concatenate([d["fixed_normals"], np.repeat(d["fixed_normals"][sel], size - 1, axis=0)]))
    return d


def cropped():
    """the cropped-cloud setting of test_partial_overlap_through_the_one_linearisation_flow, at 3 000 points"""
    d = syn.cloud_pair_3d(n=N, seed=2601, t=(0.08, -0.05, 0.03), rpy_deg=(1.5, -2.0, 2.5))
    d = {k: v.copy() for k, v in d.items()}
    keep = d["fixed"][:, 0] <= np.quantile(d["fixed"][:, 0], 0.6)
    d["fixed"], d["fixed_normals"] = d["fixed"][keep], d["fixed_normals"][keep]
    return d


def with_edges(d):
    """moving points with NaN coordinates, with no neighbour inside the gate, and outside the grid"""
    d = dict(d)
    m = d["moving"].copy()
    m[5::397, 0] = np.nan
    m[7::401, 2] += 1.5     # (above the scene: nothing within the gate)
    m[11::409] += 500.0     # (far outside the fixed cloud's grid)
    d["moving"] = m
    return d


def gate_of(dim):
    return 0.5 if dim == 2 else 0.4


def run_all(oracle, product, kind, slice_kind, d, knobs_list, max_iterations=12, criterion=False, inlier_only=False):
    """oracle + one product run per knob set, two compute() calls each (the second finds the lists of the fixed cloud in place);
    every product run must be the oracle's, bit for bit, and must have taken the fused path iff asked to"""
    dim = 2 if kind == abi.SE2_RIGHT else 3
    cfg = cue_config(kind, slice_kind, gate_of(dim), abi.ROBUST_CAUCHY, 0.05)
    runs = []
    for make, knobs in [(lambda: oracle.OracleAligner(kind), None)] + [(lambda: product.MultiAligner(kind), k) for k in knobs_list]:
        al = make()
        if knobs:
            al.set_tuning(**knobs)
        al.set_params(max_iterations=max_iterations, min_num_inliers=10, enable_inlier_only_runs=inlier_only)
        if criterion:
            al.set_termination_criteria(abi.default_termination_params())
        setup_pair(al, d, cfg)
        al.compute()
        al.set_moving_in_fixed(syn.identity(al.dim))
        al.compute()
        if knobs:
            path = al.last_compute_path()
            assert bool(path & abi.PATH_FUSED_CONTROL) == bool(knobs.get("fused_control")), (knobs, path)
            assert not path & abi.PATH_ONE_WORKGROUP, path
        runs.append(al)
    ref = runs[0]
    assert ref.status() == abi.SUCCESS, ref.status()
    for got in runs[1:]:
        assert_same_run(ref, got)
        assert got.information().tobytes() == ref.information().tobytes()
    return runs
