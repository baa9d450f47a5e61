"""Independent numpy restatement of the stereo-feature adaptor (DESIGN.md section 4 "Stereo features").

A rectified pair of U8 images -> the left image's keypoints that found their partner in the right image, triangulated.  Each image
goes through features_restatement.extract on its own; matching (row band, disparity gate, smallest (Hamming distance, pixel
index), distance gate, cross check) and the sub-pixel costs are integer arithmetic, the depth is z = (fx * baseline) / disparity
in float32, so the library must give the same bits.  Nothing here knows the library.
"""
import numpy as np

import features_restatement as fr

F = np.float32
MATCH_DTYPE = np.dtype([("left_pixel", np.int32), ("right_pixel", np.int32), ("distance", np.int32), ("disparity", np.float32)])
DEFAULTS = dict(min_disparity=1, max_disparity=128, row_tolerance=1, max_distance=48, cross_check=True, subpixel=True)
COUNTERS = ("status", "num_pixels", "num_left", "num_right", "num_matched", "num_mutual", "num_in_range", "scene_size")
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def hamming(a, b):
    """(len(a), len(b)) int64: bit differences between every row of a and every row of b ((n, 32) uint8 each)"""
    return _POPCOUNT[a[:, None, :] ^ b[None, :, :]].sum(-1)


def best_candidates(h, allowed):
    """per row of h (distances, candidates along the columns in ascending pixel order) the column of the smallest
    (distance, column) among the allowed ones, -1 without one; and whether another allowed column has the same distance"""
    n, m = h.shape
    best, tied = np.full(n, -1, np.int64), np.zeros(n, bool)
    if m == 0:
        return best, tied
    key = np.where(allowed, h * m + np.arange(m)[None, :], np.iinfo(np.int64).max)
    j = key.argmin(1)
    has = allowed.any(1)
    best[has] = j[has]
    hmin = np.where(allowed, h, np.iinfo(np.int64).max).min(1)
    tied = has & ((allowed & (h == hmin[:, None])).sum(1) > 1)
    return best, tied


def costs(L, R, r, cl, rr, cr):
    """cost(-1), cost(0), cost(1): the sum over the 7x7 window of |L(r+dy, cl+dx) - R(rr+dy, cr+k+dx)|"""
    a = L[r - 3:r + 4, cl - 3:cl + 4].astype(np.int64)
    return tuple(int(np.abs(a - R[rr - 3:rr + 4, cr + k - 3:cr + k + 4].astype(np.int64)).sum()) for k in (-1, 0, 1))


def offset(cm, c0, cp):
    """(off float32, D): the parabola's minimum through the three costs, 0 unless cost(0) is the smallest and D > 0"""
    D = cm - 2 * c0 + cp
    if c0 <= cm and c0 <= cp and D > 0:
        return F(cm - cp) / F(2 * D), D
    return F(0.0), D


def match(left, right, K, baseline, fast_threshold=20, max_features=1000, oriented=True, depth_min=0.4, depth_max=8.0,
          min_disparity=1, max_disparity=128, row_tolerance=1, max_distance=48, cross_check=True, subpixel=True, extracted=None):
    """dict(points (n, 3) f32, intensity (n,) f32, descriptors (n, 32) u8, global_indices (n,) i32, keypoints (n, 3) i32 of
    left pixel / score / angle_bin, matches (n,) MATCH_DTYPE, the counters of srrg2_stereo_result, and `details`: per left
    keypoint what became of it -- for the tests that pin the cases)"""
    L, R = np.asarray(left), np.asarray(right)
    if L.shape != R.shape:
        raise ValueError("left and right: one shape")
    rows, cols = L.shape
    if extracted is None:
        extracted = tuple(fr.extract(I, K=K, fast_threshold=fast_threshold, max_features=max_features, oriented=oriented)
                          for I in (L, R))
    eL, eR = extracted
    pl, pr = eL["global_indices"].astype(np.int64), eR["global_indices"].astype(np.int64)
    nl, nr = len(pl), len(pr)
    c = max(cols, 1)
    rl, cl, rr, cr = pl // c, pl % c, pr // c, pr % c
    h = hamming(eL["descriptors"], eR["descriptors"])
    band = np.abs(rr[None, :] - rl[:, None]) <= row_tolerance
    d = cl[:, None] - cr[None, :]
    allowed = band & (d >= min_disparity) & (d <= max_disparity)
    best_l, tied = best_candidates(h, allowed)
    best_r, _ = best_candidates(h.T, allowed.T)
    idx = np.arange(nl)
    has = best_l >= 0
    hbest = np.where(has, h[idx, np.maximum(best_l, 0)] if nr else 0, -1)
    matched = has & (hbest <= max_distance)
    mutual = matched.copy()
    if cross_check:
        mutual &= best_r[np.maximum(best_l, 0)] == idx if nr else False
    fb = F(np.asarray(K, F).reshape(9)[0]) * F(baseline)
    disparity, z = np.zeros(nl, F), np.zeros(nl, F)
    cost3, curv = np.zeros((nl, 3), np.int64), np.zeros(nl, np.int64)
    for i in np.flatnonzero(mutual):
        j = best_l[i]
        off = F(0.0)
        if subpixel:
            cost3[i] = costs(L, R, int(rl[i]), int(cl[i]), int(rr[j]), int(cr[j]))
            off, curv[i] = offset(*(int(v) for v in cost3[i]))
        disparity[i] = F(cl[i] - cr[j]) - off
        z[i] = fb / disparity[i]
    depth = np.zeros((rows, cols), F)
    depth.reshape(-1)[pl[mutual]] = z[mutual]
    pts, in_range = fr.keypoint_points(pl, cols, K, depth, depth_min=depth_min, depth_max=depth_max)
    keep = mutual & in_range
    ms = np.zeros(int(keep.sum()), MATCH_DTYPE)
    ms["left_pixel"], ms["right_pixel"] = pl[keep], pr[best_l[keep]]
    ms["distance"], ms["disparity"] = hbest[keep], disparity[keep]
    details = dict(band_size=band.sum(1), num_candidates=allowed.sum(1), best=best_l, distance=hbest, tied=tied, matched=matched,
                   mutual=mutual, kept=keep, costs=cost3, curvature=curv, disparity=disparity, z=z, left_pixel=pl, right_pixel=pr)
    return dict(points=pts[keep].reshape(-1, 3), intensity=eL["intensity"][keep], descriptors=eL["descriptors"][keep].reshape(-1, 32),
                global_indices=eL["global_indices"][keep], keypoints=eL["keypoints"][keep].reshape(-1, 3), matches=ms,
                status=1 if rows * cols == 0 else 0, num_pixels=rows * cols, num_left=nl, num_right=nr,
                num_matched=int(matched.sum()), num_mutual=int(mutual.sum()), num_in_range=int(keep.sum()), scene_size=int(keep.sum()),
                details=details, left=eL, right=eR)


def depth_image_of(matches, rows, cols, K, baseline):
    """the F32 depth image that (6) of the contract speaks of: z at the matched left pixels, 0 elsewhere"""
    fb = F(np.asarray(K, F).reshape(9)[0]) * F(baseline)
    depth = np.zeros((rows, cols), F)
    depth.reshape(-1)[matches["left_pixel"]] = fb / matches["disparity"].astype(F)
    return depth
