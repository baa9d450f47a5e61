"""Independent numpy restatement of the dense stereo adaptor (DESIGN.md section 4 "Dense stereo").

A rectified pair of U8 images -> census (9 x 7, 62 bits) -> Hamming cost over the disparity range -> semi-global aggregation along
the four axis directions -> best disparity, uniqueness, left-right check along the volume's diagonal, sub-pixel parabola -> depth
-> adaptor_restatement.adapt_depth_image's scene.  Everything up to the float disparity is integer arithmetic, the rest is
float32 in the documented order, so the library must give the same bits.  Nothing here knows the library.
"""
import numpy as np

import adaptor_restatement as ar

F = np.float32
DEFAULTS = dict(min_disparity=1, max_disparity=64, paths=4, p1=8, p2=48, uniqueness_ratio=10, lr_check=True, lr_tolerance=1,
                subpixel=True)
COUNTERS = ("status", "num_pixels", "num_evaluated", "num_unique", "num_consistent", "num_in_range", "num_valid", "scene_size")
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)
_BIG = 1 << 20  # above every aggregated cost: stands for a term the contract omits


def rectangle(rows, cols, max_disparity):
    """(first row, one past the last row, first column, one past the last column) of the processed rectangle; empty: None"""
    r0, r1, c0, c1 = 3, rows - 3, 4 + max_disparity, cols - 4
    return None if r1 <= r0 or c1 <= c0 else (r0, r1, c0, c1)


def census(I):
    """(rows, cols) uint64: bit per (dy, dx) in [-3, 3] x [-4, 4] except (0, 0), set iff I(r+dy, c+dx) < I(r, c); 0 where undefined"""
    I = np.asarray(I).astype(np.int64)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.uint64)
    if rows < 7 or cols < 9:
        return out
    ctr = I[3:rows - 3, 4:cols - 4]
    acc = np.zeros(ctr.shape, np.uint64)
    bit = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            acc |= (I[3 + dy:rows - 3 + dy, 4 + dx:cols - 4 + dx] < ctr).astype(np.uint64) << np.uint64(bit)
            bit += 1
    out[3:rows - 3, 4:cols - 4] = acc
    return out


def popcount64(x):
    return _POPCOUNT[np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def cost_volume(L, R, min_disparity, max_disparity):
    """(H, W, ND) int64 over the processed rectangle, None when it is empty"""
    rows, cols = L.shape
    rect = rectangle(rows, cols, max_disparity)
    if rect is None:
        return None
    r0, r1, c0, c1 = rect
    cl, cr = census(L), census(R)
    nd = max_disparity - min_disparity + 1
    C = np.zeros((r1 - r0, c1 - c0, nd), np.int64)
    for k in range(nd):
        d = min_disparity + k
        C[:, :, k] = popcount64(cl[r0:r1, c0:c1] ^ cr[r0:r1, c0 - d:c1 - d])
    return C


def _path(C, p1, p2, axis, reverse):
    """L_e over the whole volume for one direction: lines along `axis` (0: rows, 1: columns), walked backwards when `reverse`"""
    V = np.moveaxis(C, axis, 0)
    if reverse:
        V = V[::-1]
    out = np.empty_like(V)
    out[0] = V[0]
    for i in range(1, V.shape[0]):
        prev = out[i - 1]
        M = prev.min(-1, keepdims=True)
        lo = np.full_like(prev, _BIG)
        hi = np.full_like(prev, _BIG)
        lo[..., 1:] = prev[..., :-1] + p1
        hi[..., :-1] = prev[..., 1:] + p1
        out[i] = V[i] + np.minimum(np.minimum(prev, lo), np.minimum(hi, M + p2)) - M
    if reverse:
        out = out[::-1]
    return np.moveaxis(out, 0, axis)


def aggregate(C, paths, p1, p2):
    if paths == 0:
        return C.copy()
    return _path(C, p1, p2, 1, False) + _path(C, p1, p2, 1, True) + _path(C, p1, p2, 0, False) + _path(C, p1, p2, 0, True)


def disparity(left, right, min_disparity=1, max_disparity=64, paths=4, p1=8, p2=48, uniqueness_ratio=10, lr_check=True,
              lr_tolerance=1, subpixel=True):
    """dict(disparity (rows, cols) f32 with 0 where there is none, evaluated / unique / consistent (rows, cols) masks, best
    (rows, cols) int with -1 outside the rectangle, S (H, W, ND) or None)"""
    L, R = np.asarray(left), np.asarray(right)
    if L.shape != R.shape:
        raise ValueError("left and right: one shape")
    rows, cols = L.shape
    disp = np.zeros((rows, cols), F)
    ev, un, co = (np.zeros((rows, cols), bool) for _ in range(3))
    best = np.full((rows, cols), -1, np.int64)
    C = cost_volume(L, R, min_disparity, max_disparity) if rows * cols else None
    if C is None:
        return dict(disparity=disp, evaluated=ev, unique=un, consistent=co, best=best, S=None)
    r0, r1, c0, c1 = rectangle(rows, cols, max_disparity)
    H, W, nd = C.shape
    S = aggregate(C, paths, p1, p2)
    k = S.argmin(-1)  # (the first of equal minima: the smallest d)
    sb = np.take_along_axis(S, k[..., None], -1)[..., 0]
    ks = np.arange(nd)[None, None, :]
    far = np.abs(ks - k[..., None]) > 1
    s2 = np.where(far, S, _BIG * 8).min(-1)
    unique = np.ones((H, W), bool)
    if uniqueness_ratio > 0:
        unique = ~far.any(-1) | (s2 * (100 - uniqueness_ratio) > 100 * sb)
    consistent = unique.copy()
    if lr_check:
        # dR over the right image's columns: the left volume read along its diagonal, ascending d, strict <: the smallest d on ties
        sr = np.full((H, cols), _BIG * 8, np.int64)
        dr = np.full((H, cols), -(1 << 30), np.int64)
        for kk in range(nd):
            d = min_disparity + kk
            cand = S[:, :, kk]
            view_s, view_d = sr[:, c0 - d:c1 - d], dr[:, c0 - d:c1 - d]
            better = cand < view_s
            view_s[better] = cand[better]
            view_d[better] = d
        dstar = k + min_disparity
        x = np.arange(c0, c1)[None, :] - dstar
        got = np.take_along_axis(dr, x, 1)
        consistent &= np.abs(got - dstar) <= lr_tolerance
    val = (k + min_disparity).astype(F)
    if subpixel:
        inner = (k > 0) & (k < nd - 1)
        a = np.take_along_axis(S, np.maximum(k - 1, 0)[..., None], -1)[..., 0]
        cc = np.take_along_axis(S, np.minimum(k + 1, nd - 1)[..., None], -1)[..., 0]
        D = a - 2 * sb + cc
        ok = inner & (D > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = (a - cc).astype(F) / (2 * D).astype(F)
        val = np.where(ok, val + off.astype(F), val).astype(F)
    ev[r0:r1, c0:c1] = True
    un[r0:r1, c0:c1] = unique
    co[r0:r1, c0:c1] = consistent
    best[r0:r1, c0:c1] = k + min_disparity
    disp[r0:r1, c0:c1] = np.where(consistent, val, F(0.0))
    return dict(disparity=disp, evaluated=ev, unique=un, consistent=co, best=best, S=S)


def depth_of(disp, K, baseline):
    """Z = (fx * baseline) / disparity in float32, the product first; NaN where there is no disparity"""
    fb = F(np.asarray(K, F).reshape(9)[0]) * F(baseline)
    disp = np.asarray(disp, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (fb / disp).astype(F)
    return np.where(disp != 0, z, F(np.nan)).astype(F)


def adapt(left, right, K, baseline, depth_min=0.4, depth_max=8.0, col_gap=1, row_gap=1, max_distance_squared=0.0625,
          drop_points_without_normal=True, compact=False, **stereo):
    """the scene of adaptor_restatement.adapt_depth_image on Z with the left image as the intensity, plus `disparity`, the masks
    and the counters of srrg2_dense_stereo_result"""
    d = disparity(left, right, **stereo)
    z = depth_of(d["disparity"], K, baseline)
    out = ar.adapt_depth_image(z, K, depth_min=depth_min, depth_max=depth_max, col_gap=col_gap, row_gap=row_gap,
                               max_distance_squared=max_distance_squared, drop_points_without_normal=drop_points_without_normal,
                               compact=compact, intensity=np.asarray(left))
    n = int(np.asarray(left).size)
    out.update(disparity=d["disparity"], depth=z, evaluated=d["evaluated"], unique=d["unique"], consistent=d["consistent"],
               best=d["best"], status=1 if n == 0 else 0, num_pixels=n, num_evaluated=int(d["evaluated"].sum()),
               num_unique=int(d["unique"].sum()), num_consistent=int(d["consistent"].sum()), scene_size=len(out["points"]))
    return out
