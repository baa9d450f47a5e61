"""Independent numpy restatement of the feature tracker's contract (DESIGN.md section 4 "Feature tracking"): the projection in
float32 in the projective clipper's operation order, then every (landmark, keypoint) pair by brute force -- no row table, no
windows over sorted ranges.  It knows nothing of the library: the GPU tests compare srrg2_scene_track_features against it bit
for bit.  ``track_per_pair`` says the same in scalar Python, one pair at a time; tests/test_tracking_restatement.py holds the
two to each other."""
import numpy as np

F = np.float32
CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)
COUNTERS = ("num_moving", "num_fixed", "num_in_view", "num_with_candidate", "num_accepted", "num_mutual", "num_correspondences")


def hamming(A, B):
    """(len(A), len(B)) Hamming distances of (n, 32) uint8 rows"""
    A, B = np.asarray(A, np.uint8).reshape(-1, 32), np.asarray(B, np.uint8).reshape(-1, 32)
    out = np.zeros((len(A), len(B)), np.int64)
    for lo in range(0, len(A), 512):  # (chunks keep the xor table small)
        out[lo:lo + 512] = _POP[A[lo:lo + 512, None, :] ^ B[None, :, :]].sum(axis=2)
    return out


def project(points, moving_in_sensor, K, rows, cols, depth_min, depth_max):
    """-> (in_view, rv, cu) per landmark: srrg2_scene_clip_projective's steps with ONE transform, float32 throughout"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    M = np.asarray(moving_in_sensor, F).reshape(3, 4)
    K = np.asarray(K, F).reshape(3, 3)
    with np.errstate(all="ignore"):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        c = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]
        ok = np.isfinite(P).all(axis=1) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])
        ok &= (c[2] >= F(depth_min)) & (c[2] <= F(depth_max))
        u = (K[0, 0] * c[0]) / c[2] + K[0, 2]
        v = (K[1, 1] * c[1]) / c[2] + K[1, 2]
        uf, vf = u + F(0.5), v + F(0.5)
        in_view = ok & (uf >= F(0)) & (uf < F(cols)) & (vf >= F(0)) & (vf < F(rows))
        rv = np.where(in_view, np.floor(np.where(in_view, vf, 0)), -1).astype(np.int64)
        cu = np.where(in_view, np.floor(np.where(in_view, uf, 0)), -1).astype(np.int64)
    return in_view, rv, cu


def track(points, moving_desc, fixed_pixels, fixed_desc, moving_in_sensor, K, rows, cols, depth_min=0.4, depth_max=8.0,
          search_radius=16, max_distance=48, min_margin=0, cross_check=True):
    """-> dict: correspondences (CORR_DTYPE, ascending moving_idx), the counters of srrg2_track_result, and details (per landmark
    in_view, rv, cu, num_candidates, best, distance, second, accepted, mutual; the number of evaluated pairs)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    nm, pix = len(P), np.asarray(fixed_pixels, np.int64).reshape(-1)
    nf, R = len(pix), int(search_radius)
    in_view, rv, cu = project(P, moving_in_sensor, K, rows, cols, depth_min, depth_max)
    fr, fc = pix // cols, pix % cols
    cand = in_view[:, None] & (np.abs(fr[None, :] - rv[:, None]) <= R) & (np.abs(fc[None, :] - cu[:, None]) <= R)  # (nm, nf)
    H = hamming(moving_desc, fixed_desc) if nm and nf else np.zeros((nm, nf), np.int64)
    BIG = 1 << 20
    Hc = np.where(cand, H, BIG)
    ncand = cand.sum(axis=1)
    has = ncand > 0
    best = np.where(has, np.argmin(Hc, axis=1) if nf else 0, -1)  # (argmin: the first of equal distances = the smallest j)
    idx = np.arange(nm)
    h = np.where(has, Hc[idx, np.maximum(best, 0)] if nf else 0, -1)
    Hs = Hc.copy()
    if nf:
        Hs[idx, np.maximum(best, 0)] = BIG
    second = np.where(ncand > 1, Hs.min(axis=1) if nf else 0, -1)
    accepted = has & (h <= int(max_distance))
    if int(min_margin) > 0:
        accepted &= (ncand == 1) | (second - h >= int(min_margin))
    mutual = accepted.copy()
    if cross_check and nf:
        # per keypoint: the landmark of smallest (h, i) among those that have it as a candidate (argmin over axis 0: smallest i)
        back = np.where(cand.any(axis=0), np.argmin(Hc, axis=0), -1)
        mutual &= back[np.maximum(best, 0)] == idx
    keep = np.flatnonzero(mutual)
    corr = np.zeros(len(keep), CORR_DTYPE)
    corr["fixed_idx"], corr["moving_idx"], corr["response"] = best[keep], keep, h[keep].astype(F)
    return dict(correspondences=corr, num_moving=nm, num_fixed=nf, num_in_view=int(in_view.sum()), num_with_candidate=int(has.sum()),
                num_accepted=int(accepted.sum()), num_mutual=int(mutual.sum()), num_correspondences=int(mutual.sum()),
                details=dict(in_view=in_view, rv=rv, cu=cu, num_candidates=ncand, best=best, distance=h, second=second,
                             accepted=accepted, mutual=mutual, num_pairs=int(cand.sum())))


def _popcount_rows(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


def track_per_pair(points, moving_desc, fixed_pixels, fixed_desc, moving_in_sensor, K, rows, cols, depth_min=0.4, depth_max=8.0,
                   search_radius=16, max_distance=48, min_margin=0, cross_check=True):
    """the same contract, one landmark and one pair at a time in plain Python (float32 scalars for the projection): slow, for
    small cases only.  -> (correspondences, counters dict)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    M, Kf = np.asarray(moving_in_sensor, F).reshape(3, 4), np.asarray(K, F).reshape(3, 3)
    D, E = np.asarray(moving_desc, np.uint8).reshape(-1, 32), np.asarray(fixed_desc, np.uint8).reshape(-1, 32)
    pix = [int(p) for p in np.asarray(fixed_pixels).reshape(-1)]
    R = int(search_radius)
    fwd, back = {}, {}  # landmark -> (h, j, second or None); keypoint -> (h, i)
    n_view = n_cand = n_acc = 0
    with np.errstate(all="ignore"):
        for i, (x, y, z) in enumerate(P):
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            c = [F(F(F(M[r, 0] * x) + F(M[r, 1] * y)) + F(M[r, 2] * z)) + M[r, 3] for r in range(3)]
            if not all(np.isfinite(v) for v in c) or not (c[2] >= F(depth_min)) or not (c[2] <= F(depth_max)):
                continue
            uf = F(F(F(Kf[0, 0] * c[0]) / c[2]) + Kf[0, 2]) + F(0.5)
            vf = F(F(F(Kf[1, 1] * c[1]) / c[2]) + Kf[1, 2]) + F(0.5)
            if not (uf >= 0 and uf < F(cols) and vf >= 0 and vf < F(rows)):
                continue
            n_view += 1
            rv, cu = int(np.floor(vf)), int(np.floor(uf))
            seen = []
            for j, p in enumerate(pix):
                if abs(p // cols - rv) <= R and abs(p % cols - cu) <= R:
                    hh = _popcount_rows(D[i], E[j])
                    seen.append((hh, j))
                    if j not in back or (hh, i) < back[j]:
                        back[j] = (hh, i)
            if seen:
                n_cand += 1
                seen.sort()
                fwd[i] = (seen[0][0], seen[0][1], seen[1][0] if len(seen) > 1 else None)
    pairs = []
    for i in sorted(fwd):
        hh, j, second = fwd[i]
        if hh > int(max_distance) or (int(min_margin) > 0 and second is not None and second - hh < int(min_margin)):
            continue
        n_acc += 1
        if cross_check and back[j][1] != i:
            continue
        pairs.append((j, i, float(hh)))
    corr = np.array(pairs, CORR_DTYPE) if pairs else np.zeros(0, CORR_DTYPE)
    return corr, dict(num_moving=len(P), num_fixed=len(pix), num_in_view=n_view, num_with_candidate=n_cand, num_accepted=n_acc,
                      num_mutual=len(pairs), num_correspondences=len(pairs))


def to_merger(corr, moving_global_indices):
    """the pairs as the merger reads them: fixed_idx = map point, moving_idx = measurement point"""
    g = np.asarray(moving_global_indices, np.int64).reshape(-1)
    out = np.zeros(len(corr), CORR_DTYPE)
    out["fixed_idx"], out["moving_idx"], out["response"] = g[corr["moving_idx"]], corr["fixed_idx"], corr["response"]
    return out
