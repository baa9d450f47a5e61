"""Independent numpy restatement of the scale-pyramid feature adaptor (DESIGN.md section 4 "Image features: scale pyramid").

Built on features_restatement.py: level sizes, the integer bilinear resampler, the per-level quotas and extract_pyramid, which runs
the single-scale restatement's stages on every level and places the keypoints at their level-0 positions.  All image arithmetic is
integer, so the library must give the same bits.  Nothing here knows the library.
"""
import numpy as np

import features_restatement as fr

F = np.float32
MAX_LEVELS = 8


def level_sizes(rows, cols, num_levels=4, num=6, den=5):
    """[(rows_l, cols_l)] of the levels that are built: floor(previous * den / num), ending before the first side <= 32"""
    out = []
    for _ in range(num_levels):
        if rows <= 2 * fr.MARGIN or cols <= 2 * fr.MARGIN:
            break
        out.append((rows, cols))
        rows, cols = rows * den // num, cols * den // num
    return out


def _taps(n_dst, n_src, num, den):
    """(i0, i1, f) int64 per destination index: X = ((2c+1) num 256) // (2 den) - 128"""
    c = np.arange(n_dst, dtype=np.int64)
    X = ((2 * c + 1) * num * 256) // (2 * den) - 128
    assert n_dst == 0 or X.min() >= 0
    return np.minimum(X >> 8, n_src - 1), np.minimum((X >> 8) + 1, n_src - 1), X & 255


def resample(img, num=6, den=5):
    """uint8 (rows * den // num, cols * den // num): bilinear with 8 fractional bits, sampled at pixel centres"""
    I = np.asarray(img).astype(np.int64)
    rows, cols = I.shape
    y0, y1, fy = _taps(rows * den // num, rows, num, den)
    x0, x1, fx = _taps(cols * den // num, cols, num, den)
    fy, gy, gx = fy[:, None], 256 - fy[:, None], 256 - fx[None, :]
    fx = fx[None, :]
    v = I[y0][:, x0] * gx * gy + I[y0][:, x1] * fx * gy + I[y1][:, x0] * gx * fy + I[y1][:, x1] * fx * fy + 32768
    return (v >> 16).astype(np.uint8)


def resample_loop(img, num=6, den=5):
    """resample(), one pixel at a time in plain Python integers"""
    rows, cols = img.shape
    out = np.zeros((rows * den // num, cols * den // num), np.uint8)
    for r in range(out.shape[0]):
        Y = ((2 * r + 1) * num * 256) // (2 * den) - 128
        y0, y1, fy = min(Y >> 8, rows - 1), min((Y >> 8) + 1, rows - 1), Y & 255
        for c in range(out.shape[1]):
            X = ((2 * c + 1) * num * 256) // (2 * den) - 128
            x0, x1, fx = min(X >> 8, cols - 1), min((X >> 8) + 1, cols - 1), X & 255
            v = (int(img[y0, x0]) * (256 - fx) * (256 - fy) + int(img[y0, x1]) * fx * (256 - fy) +
                 int(img[y1, x0]) * (256 - fx) * fy + int(img[y1, x1]) * fx * fy + 32768)
            out[r, c] = v >> 16
    return out


def build(img, num_levels=4, num=6, den=5):
    """the level images: level 0 is img itself, each further one resampled from the one before"""
    img = np.asarray(img)
    out = []
    for _ in level_sizes(img.shape[0], img.shape[1], num_levels, num, den):
        out.append(img)
        img = resample(img, num, den)
    return out


def quotas(sizes, max_features):
    """per built level floor(max_features * A_l / sum A), level 0 also the remainder; all 0 without a cap"""
    if max_features <= 0 or not sizes:
        return [0] * len(sizes)
    areas = [r * c for r, c in sizes]
    q = [max_features * a // sum(areas) for a in areas]
    q[0] += max_features - sum(q)
    return q


def position_q8(i, level, num=6, den=5):
    """level-0 position, 1/256 pixel, of the centre of level index i (int64 array): ((2i+1) num^l 128) // den^l - 128"""
    return ((2 * np.asarray(i, np.int64) + 1) * (num ** level) * 128) // (den ** level) - 128


def extract_pyramid(img, K=None, fast_threshold=20, max_features=1000, oriented=True, depth=None, depth_scale=0.001, depth_min=0.4,
                    depth_max=8.0, num_levels=4, num=6, den=5):
    """dict(points (n, 3) f32, intensity (n,) f32, descriptors (n, 32) u8, global_indices (n,) i32, keypoints (n, 8) i32 of
    pixel / score / angle_bin / level / level_pixel / u_q8 / v_q8 / 0, and the fields of srrg2_pyramid_result, per-level ones as
    lists over the built levels)"""
    I0 = np.asarray(img)
    if I0.dtype != np.uint8 or I0.ndim != 2:
        raise ValueError("intensity image: 2-D uint8")
    rows0, cols0 = I0.shape
    K = np.asarray(np.eye(3, dtype=F) if K is None else K, F).reshape(3, 3)
    levels = build(I0, num_levels, num, den)
    sizes = [im.shape for im in levels]
    quota = quotas(sizes, max_features)
    out = {"status": 1 if rows0 * cols0 == 0 else 0, "num_levels_built": len(levels), "rows": [s[0] for s in sizes],
           "cols": [s[1] for s in sizes], "quota": quota, "num_candidates": [], "num_maxima": [], "num_selected": [],
           "num_with_depth": []}
    parts = {k: [] for k in ("points", "intensity", "descriptors", "keypoints")}
    ifx, ify = F(1.0) / K[0, 0], F(1.0) / K[1, 1]
    for l, I in enumerate(levels):
        rows, cols = I.shape
        score = fr.fast_score(I)
        cand, kp = fr.maxima(score, fast_threshold)
        pix = np.flatnonzero(kp.reshape(-1))
        sc = score.reshape(-1)[pix]
        if max_features > 0 and quota[l] == 0:
            sel = np.zeros(0, np.int64)
        else:
            sel = fr.cap(pix, sc, quota[l])
        pix, sc = pix[sel], sc[sel]
        r, c = pix // cols, pix % cols
        u, v = position_q8(c, l, num, den), position_q8(r, l, num, den)
        c0, r0 = np.minimum((u + 128) >> 8, cols0 - 1), np.minimum((v + 128) >> 8, rows0 - 1)
        pixel0 = r0 * cols0 + c0
        # the depth gate at (r0, c0) by the single-scale rule; the point at the sub-pixel level-0 position
        gate_pts, kept = fr.keypoint_points(pixel0, cols0, K, depth, depth_scale, depth_min, depth_max)
        z = gate_pts[:, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            x = ((u.astype(F) * F(1.0 / 256.0) - K[0, 2]) * ifx) * z
            y = ((v.astype(F) * F(1.0 / 256.0) - K[1, 2]) * ify) * z
        pts = np.stack([x, y, z], -1).astype(F)
        out["num_candidates"].append(int(cand.sum()))
        out["num_maxima"].append(int(kp.sum()))
        out["num_selected"].append(len(pix))
        out["num_with_depth"].append(int(kept.sum()))
        pix, sc, r, c, u, v, pixel0, pts = (a[kept] for a in (pix, sc, r, c, u, v, pixel0, pts))
        B = fr.box_sums(I)
        pats, bins, desc = {}, [], []
        for rr, cc in zip(r, c):
            k = fr.orientation_bin(I, int(rr), int(cc), oriented)
            if k not in pats:
                pats[k] = fr.rotated_pattern(k)
            bins.append(k)
            desc.append(fr.describe(B, int(rr), int(cc), pats[k]))
        n = len(pix)
        parts["points"].append(pts.reshape(-1, 3))
        parts["intensity"].append(I.reshape(-1)[pix].astype(F))
        parts["descriptors"].append(np.array(desc, np.uint8).reshape(-1, 32))
        parts["keypoints"].append(np.stack([pixel0, sc, np.array(bins, np.int64), np.full(n, l, np.int64), pix, u, v,
                                            np.zeros(n, np.int64)], -1).astype(np.int32).reshape(-1, 8))
    empty = {"points": np.zeros((0, 3), F), "intensity": np.zeros(0, F), "descriptors": np.zeros((0, 32), np.uint8),
             "keypoints": np.zeros((0, 8), np.int32)}
    for k, v in parts.items():
        out[k] = np.concatenate(v) if v else empty[k]
    out["global_indices"] = out["keypoints"][:, 0].copy()
    out["scene_size"] = len(out["keypoints"])
    return out


def mutual_matches(da, db, max_distance=64):
    """(ia, ib): mutual nearest neighbours by Hamming distance (lowest index of equals) within max_distance"""
    if len(da) == 0 or len(db) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    bits_a, bits_b = np.unpackbits(da, axis=1).astype(np.int32), np.unpackbits(db, axis=1).astype(np.int32)
    dist = bits_a.sum(1)[:, None] + bits_b.sum(1)[None, :] - 2 * bits_a @ bits_b.T
    best_b, best_a = dist.argmin(1), dist.argmin(0)
    ia = np.flatnonzero((best_a[best_b] == np.arange(len(da))) & (dist[np.arange(len(da)), best_b] <= max_distance))
    return ia, best_b[ia]


def correct_matches(uv_a, uv_b, ia, ib, num, den, tol_pixels=3.0):
    """how many matches (ia, ib) are correct when B is A resampled by num/den: A's level-0 position (1/256 pixel, (n, 2)) within
    tol_pixels * num/den of where B's keypoint comes from in A, (2 c_B + 1) num / (2 den) - 1/2"""
    if len(ia) == 0:
        return 0
    src = ((2.0 * (uv_b[ib] / 256.0) + 1.0) * num / (2.0 * den)) - 0.5
    d = np.abs(uv_a[ia] / 256.0 - src).max(1)
    return int((d <= tol_pixels * num / den).sum())
