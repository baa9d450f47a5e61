"""One more scenario for the staged neighbours of the converged passes (tests/staged_neighbour_scenarios.py has the others): fixed
points with TWO twins.  A staged winner that is not the neighbour the point had brings its position and its coordinates from the
staged set, and its normal from a load requested while the record was waited for -- if it is the runner-up of the kept neighbour at
the previous query (csrc/kernels.hip, icp_step_fast_body).  With three candidates inside the certificate's safety factors the third
one can win: that winner is fetched as before.  Shared by tests/test_gpu_staged_winners.py (product library) and
tests/helpers_scripts/staged_winners_check.py (the -DSRRG2_FUSED_STALL build, whose counters tell the two apart)."""
import numpy as np

import staged_neighbour_scenarios as sc


def _three_nearest(Q, F):
    d = np.sqrt(((Q[:, None, :] - F[None, :, :].astype(np.float64)) ** 2).sum(-1))
    return np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1).T


def with_triplets(d, count=32, exact=8):
    """`count` fixed points -- the ones most moving points look at first at the ground truth -- get two twins each, at f + delta t and
    f - delta t along a surface tangent, with the normal of the original: delta = 0 for the first `exact` of them (three equal
    distances: the index decides), 1e-7 .. 1e-5 m for the rest (any of the three can be the nearest in a pass).  Returns the data and
    how many moving points have (d3 - d1) / d1 < 3e-5 at the ground truth."""
    d = dict(d)
    Q = sc._apply(d["X_gt"], d["moving"])
    nn, _, _ = sc._two_nearest(Q, d["fixed"])
    who, users = np.unique(nn, return_counts=True)
    sel = who[np.argsort(-users, kind="stable")][:count]
    assert len(sel) == count
    delta = np.concatenate([np.zeros(exact), np.logspace(-7, -5, count - exact)])
    f, t = d["fixed"][sel].astype(np.float64), sc._tangent(d["fixed_normals"][sel])
    twins = [(f + delta[:, None] * t).astype(np.float32), (f - delta[:, None] * t).astype(np.float32)]
    d["fixed"] = np.ascontiguousarray(np.concatenate([d["fixed"]] + twins))
    d["fixed_normals"] = np.ascontiguousarray(np.concatenate([d["fixed_normals"]] + [d["fixed_normals"][sel]] * 2))
    d1, _, d3 = _three_nearest(Q, d["fixed"])
    return d, int(np.sum((d3 - d1) < 3e-5 * d1))
