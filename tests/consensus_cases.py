"""Seeded cases of the consensus pose (DESIGN.md section 4 "Consensus pose"): a case is a dict
{dim, fixed, movings, corrs, params} -- one query cloud, K candidate clouds with their match records."""
import numpy as np

from srrg2_slam_interfaces_amd import synthetic as syn

CORR = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])

# the sizes the kernels of csrc/consensus.hip (and the shared scan of kernels_prep.hip) change their path at
WAVE = 64            # ballot / shuffle width
BLOCK = 256          # k_cns_gather, k_cns_flags, k_cns_scatter, k_cns_hyp (HYP_THREADS): threads per workgroup
SCORE_TILE = 1024    # k_cns_score: SCORE_THREADS (256) x SCORE_PPT (4) pairs per workgroup
SCORE_CHUNK = 16     # k_cns_score: survivors per workgroup
SCAN_TILE = 2048     # launch_exclusive_scan: SCAN_THREADS (256) x SCAN_ITEMS (8)
PAIR_EDGES = sorted({v + d for v in (WAVE, BLOCK, SCORE_TILE, SCAN_TILE) for d in (-1, 0, 1)})
HYPOTHESIS_EDGES = sorted({1, 1000} | {v + d for v in (SCORE_CHUNK, WAVE, BLOCK) for d in (-1, 0, 1)})


def planted(seed, dim=3, n=200, wrong=0.4, yaw_deg=180.0, noise=0.002, extent=5.0, n_moving=None):
    """fixed = landmarks seen from the query; moving = the same landmarks in the candidate's frame (+ noise); records: the true
    pairs shuffled, a share of them made wrong.  Returns fixed, moving, corr, X (moving in fixed, float64), wrong mask."""
    rng = np.random.default_rng(seed)
    if dim == 3:
        X = syn.se3(rng.uniform(-1, 1, 3), np.deg2rad([rng.uniform(-10, 10), rng.uniform(-10, 10), yaw_deg]))
        P = rng.uniform(-extent, extent, (n, 3))
        Xi = syn.se3_inv(X)
        M = P @ Xi[:, :3].T + Xi[:, 3]
    else:
        X = syn.se2(*rng.uniform(-1, 1, 2), np.deg2rad(yaw_deg))
        P = rng.uniform(-extent, extent, (n, 2))
        Xi = np.linalg.inv(X)
        M = P @ Xi[:2, :2].T + Xi[:2, 2]
    M = M + rng.normal(scale=noise, size=M.shape)
    perm = rng.permutation(n)
    corr = np.zeros(n, CORR)
    corr["fixed_idx"] = perm
    corr["moving_idx"] = perm
    bad = rng.random(n) < wrong
    corr["moving_idx"][bad] = rng.integers(0, n, int(bad.sum()))
    bad &= corr["moving_idx"] != corr["fixed_idx"]
    corr["response"] = rng.uniform(0, 25, n).astype(np.float32)
    return P.astype(np.float32), M.astype(np.float32), corr, X, bad


def case(dim, fixed, movings, corrs, **params):
    return dict(dim=dim, fixed=fixed, movings=list(movings), corrs=list(corrs), params=params)


def basic(dim, seed=1, n=120, H=64, wrong=0.4, **params):
    f, m, c, X, bad = planted(seed, dim, n, wrong)
    out = case(dim, f, [m], [c], num_hypotheses=H, seed=seed, **params)
    out["X"], out["wrong"] = X, bad
    return out


def degenerate_and_rejected(dim=3, seed=3, H=96):
    """a few points repeated (too-close samples), a share of wrong matches (length check), some invalid records"""
    f, m, c, X, bad = planted(seed, dim, 60, 0.5)
    m[5:12] = m[4]  # coincident points in the candidate: samples among them are closer than min_sample_distance
    f[5:12] = f[4]
    c["moving_idx"][3] = 10_000  # out of range
    c["fixed_idx"][7] = -1
    m[20, 0] = np.nan
    return case(dim, f, [m], [c], num_hypotheses=H, seed=seed)


def collinear_close(seed=4, H=96):
    """dim 3: most points on one line (collinear triples: |n|^2 < msd^2 |a|^2), two pairs of near-coincident points"""
    rng = np.random.default_rng(seed)
    n = 40
    s = rng.uniform(-4, 4, n)
    P = np.stack([s, 0.5 * s + 1, -0.25 * s], 1)
    P[:8] = rng.uniform(-4, 4, (8, 3))  # the few points off the line
    P[9] = P[8] + 0.01
    P[11] = P[10] + 0.02
    X = syn.se3([0.3, -0.2, 0.1], np.deg2rad([5, -3, 170]))
    Xi = syn.se3_inv(X)
    M = P @ Xi[:, :3].T + Xi[:, 3]
    c = np.zeros(n, CORR)
    c["fixed_idx"] = c["moving_idx"] = np.arange(n)
    return case(3, P.astype(np.float32), [M.astype(np.float32)], [c], num_hypotheses=H, seed=seed)


def tiny(dim, n, seed=5, H=64):
    """n pairs, all true (n below, at and above the sample size)"""
    f, m, c, _, _ = planted(seed, dim, max(n, 1), 0.0)
    return case(dim, f, [m], [c[:n]], num_hypotheses=H, seed=seed)


def duplicates(dim=3, seed=6, H=256):
    """four points (three for dim 2), every record three times: many hypotheses are the same sample, so the lowest h wins"""
    f, m, c, _, _ = planted(seed, dim, 4 if dim == 3 else 3, 0.0, noise=0.0)
    return case(dim, f, [m], [np.concatenate([c, c, c])], num_hypotheses=H, seed=seed)


TAU_EXACT_ON, TAU_EXACT_OFF = 0, 1  # the records whose e is tau^2 exactly, and just beyond it


def tau_exact(dim=3, seed=7, H=64):
    """integer coordinates and the identity pose: record TAU_EXACT_ON is off by (3, 4[, 0]) -- e = 25 = tau^2 exactly, an inlier --
    record TAU_EXACT_OFF, the same place, by -(3, 4, 1) or -(3, 5): e = 26 or 34"""
    rng = np.random.default_rng(seed)
    n = 60
    P = rng.integers(-10, 11, (n, dim)).astype(np.float32)
    P[TAU_EXACT_OFF] = P[TAU_EXACT_ON]  # one place, moved opposite ways by more than 2 tau in all: no pose takes both in
    M = P.copy()
    M[TAU_EXACT_ON, :2] += (3, 4)
    M[TAU_EXACT_OFF, :2] -= (3, 4)
    M[TAU_EXACT_OFF, dim - 1] -= 1
    c = np.zeros(n, CORR)
    c["fixed_idx"] = c["moving_idx"] = np.arange(n)
    return case(dim, P, [M], [c], num_hypotheses=H, seed=seed, inlier_distance=5.0, min_sample_distance=1.0)


def batch5(dim=3, seed=8, H=64, n=90):
    """K = 5: a normal candidate, an EMPTY one, a normal one, an ALL-INVALID one (every moving index out of range), a normal one
    of another size"""
    movings, corrs = [], []
    f = None
    for k, nk in enumerate((n, 0, n, n, n // 2)):
        fk, m, c, _, _ = planted(seed, dim, n, 0.4 if k else 0.2)  # (the same landmarks: one query cloud)
        f = fk
        if k == 3:
            c["moving_idx"] += 100_000
        movings.append(m[: max(nk, 1)] if nk != n else m)
        if nk == 0:
            movings[-1] = np.zeros((0, dim), np.float32)
        c = c[:nk]
        if nk == n // 2:
            c = c[c["moving_idx"] < len(movings[-1])]
        corrs.append(c)
    return case(dim, f, movings, corrs, num_hypotheses=H, seed=seed)


def small_cases():
    """name -> case: small enough for the plain per-hypothesis, per-pair loop of tests/test_consensus_restatement.py"""
    return {
        "dim3_basic": basic(3),
        "dim2_basic": basic(2, seed=2),
        "dim3_no_length_check": basic(3, length_check=0),
        "dim2_no_length_check": basic(2, seed=2, length_check=0),
        "dim3_degenerate_and_rejected": degenerate_and_rejected(3),
        "dim2_degenerate_and_rejected": degenerate_and_rejected(2),
        "collinear_close": collinear_close(),
        "dim3_n_below_s": tiny(3, 2),
        "dim3_n_equals_s": tiny(3, 3),
        "dim2_n_equals_s": tiny(2, 2, seed=6),
        "dim3_n_one": tiny(3, 1),
        "dim2_n_one": tiny(2, 1),
        "dim3_duplicates": duplicates(3),
        "dim2_duplicates": duplicates(2),
        "dim3_tau_exact": tau_exact(3),
        "dim2_tau_exact": tau_exact(2),
        "dim3_min_inliers_high": basic(3, min_inliers=1000),
        "dim3_batch5": batch5(3),
        "dim2_batch5": batch5(2),
    }


def cpp_cases():
    """the three cases whose per-hypothesis bit patterns the g++ build of csrc/consensus_math.h must reproduce"""
    return {"dim3": basic(3), "dim2": basic(2, seed=2), "degenerate": degenerate_and_rejected(3)}
