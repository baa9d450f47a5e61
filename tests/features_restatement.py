"""Independent numpy restatement of the image-feature adaptor (DESIGN.md section 4 "Image features").

U8 intensity image (+ optional depth image) -> keypoints: FAST-9/16 score, raster-order maxima, histogram cap, intensity-centroid
orientation in 32 bins, a 256-bit rotated-pair descriptor over 5x5 box sums, and the 3-D point of the depth adaptor.  All image
arithmetic is integer, so the library must give the same bits.  Nothing here knows the library.
"""
import numpy as np

F = np.float32
MARGIN = 16
# the 16-pixel Bresenham circle of radius 3, (dx, dy) with y pointing down, p0 .. p15
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))
_MAGNITUDES = (0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384)


def cos_sin_table():
    """(32, 2) int64: C_k, S_k = round(16384 cos / sin (2 pi k / 32)), from the nine magnitudes and the quadrant symmetries"""
    t = np.zeros((32, 2), np.int64)
    for k in range(32):
        q, j = divmod(k, 8)
        c, s = _MAGNITUDES[8 - j], _MAGNITUDES[j]  # the angle j * pi/16 in the first quadrant
        t[k] = ((c, s), (-s, c), (-c, -s), (s, -c))[q]
    return t


def base_pattern(return_draws=False):
    """(256, 4) int64 pairs (ax, ay, bx, by) from the 64-bit LCG; optionally the number of candidates drawn"""
    mask = (1 << 64) - 1
    state = [0x5352524732]

    def nxt():
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & mask
        return (state[0] >> 33) % 7

    def coord():
        return nxt() + nxt() + nxt() + nxt() - 12

    pairs, draws = [], 0
    while len(pairs) < 256:
        ax, ay, bx, by = coord(), coord(), coord(), coord()
        draws += 1
        if ax * ax + ay * ay > 169 or bx * bx + by * by > 169 or (ax, ay) == (bx, by):
            continue
        pairs.append((ax, ay, bx, by))
    p = np.array(pairs, np.int64)
    return (p, draws) if return_draws else p


def rotated_pattern(k):
    """(256, 4) int64: the pattern of bin k; x' = (x C - y S + 8192) >> 14, y' = (x S + y C + 8192) >> 14"""
    c, s = (int(v) for v in cos_sin_table()[k])
    p = base_pattern()
    out = np.empty_like(p)
    for o in (0, 2):
        x, y = p[:, o], p[:, o + 1]
        out[:, o] = (x * c - y * s + 8192) >> 14
        out[:, o + 1] = (x * s + y * c + 8192) >> 14
    return out


def disc_offsets():
    """(709, 2) int64 (dx, dy) with dx^2 + dy^2 <= 225"""
    d = np.arange(-15, 16)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    keep = dx * dx + dy * dy <= 225
    return np.stack([dx[keep], dy[keep]], -1).astype(np.int64)


def fast_score(img):
    """(rows, cols) int32 in 0 .. 255: the largest threshold below which the 9-of-16 segment test passes; 0 within 3 of a border"""
    I = np.asarray(img).astype(np.int32)
    rows, cols = I.shape
    score = np.zeros((rows, cols), np.int32)
    if rows < 7 or cols < 7:
        return score
    ctr = I[3:rows - 3, 3:cols - 3]
    d = np.stack([I[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] - ctr for dx, dy in CIRCLE], 0)
    best = np.zeros(ctr.shape, np.int32)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    score[3:rows - 3, 3:cols - 3] = best
    return score


def maxima(score, threshold):
    """(candidates, keypoints): bool images.  candidate: score > threshold inside the margin of 16; keypoint: a candidate
    strictly above its 4 raster-order predecessors among the 8 neighbours and not below its 4 successors"""
    rows, cols = score.shape
    cand = np.zeros((rows, cols), bool)
    if rows <= 2 * MARGIN or cols <= 2 * MARGIN:
        return cand, cand.copy()
    inner = (slice(MARGIN, rows - MARGIN), slice(MARGIN, cols - MARGIN))
    s = score[inner]
    cand[inner] = s > threshold
    keep = cand[inner].copy()
    for dr, dc in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):
        keep &= s > score[MARGIN + dr:rows - MARGIN + dr, MARGIN + dc:cols - MARGIN + dc]
    for dr, dc in ((0, 1), (1, -1), (1, 0), (1, 1)):
        keep &= s >= score[MARGIN + dr:rows - MARGIN + dr, MARGIN + dc:cols - MARGIN + dc]
    kp = np.zeros((rows, cols), bool)
    kp[inner] = keep
    return cand, kp


def cap(pixels, scores, max_features):
    """indices into `pixels` (ascending pixel order) that the cap keeps, through the 256-bin histogram"""
    n = len(pixels)
    if max_features <= 0 or n <= max_features:
        return np.arange(n)
    hist = np.bincount(scores, minlength=256)
    above = 0  # keypoints with a score > s
    for s in range(255, -1, -1):
        if above + hist[s] >= max_features:
            break
        above += hist[s]
    quota = max_features - above
    ties = np.flatnonzero(scores == s)[:quota]
    return np.sort(np.concatenate([np.flatnonzero(scores > s), ties]))


def box_sums(img):
    """(rows, cols) int32: the 5x5 sum centred on each pixel; 0 where the window leaves the image"""
    I = np.asarray(img).astype(np.int32)
    rows, cols = I.shape
    B = np.zeros((rows, cols), np.int32)
    if rows < 5 or cols < 5:
        return B
    acc = np.zeros((rows - 4, cols - 4), np.int32)
    for dr in range(5):
        for dc in range(5):
            acc += I[dr:rows - 4 + dr, dc:cols - 4 + dc]
    B[2:rows - 2, 2:cols - 2] = acc
    return B


def orientation_bin(img, r, c, oriented=True):
    if not oriented:
        return 0
    I = np.asarray(img)
    d = disc_offsets()
    v = I[r + d[:, 1], c + d[:, 0]].astype(np.int64)
    m10, m01 = int((d[:, 0] * v).sum()), int((d[:, 1] * v).sum())
    t = cos_sin_table()
    proj = m10 * t[:, 0] + m01 * t[:, 1]
    return int(np.argmax(proj))  # (the first of equal maxima)


def describe(B, r, c, k):
    """32 bytes: bit i = B(a_i) < B(b_i), least significant bit first"""
    p = rotated_pattern(k) if not isinstance(k, np.ndarray) else k
    bits = B[r + p[:, 1], c + p[:, 0]] < B[r + p[:, 3], c + p[:, 2]]
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def keypoint_points(pixels, cols, K, depth=None, depth_scale=0.001, depth_min=0.4, depth_max=8.0):
    """(points (n, 3) float32, kept (n,) bool): the depth adaptor's arithmetic at the keypoints' own pixels; z = 1 without depth"""
    pixels = np.asarray(pixels, np.int64)
    K = np.asarray(K, F).reshape(3, 3)
    r, c = pixels // max(cols, 1), pixels % max(cols, 1)
    if depth is None:
        z, kept = np.ones(len(pixels), F), np.ones(len(pixels), bool)
    else:
        depth = np.asarray(depth)
        raw = depth[r, c]
        if depth.dtype == np.uint16:
            z, kept = raw.astype(F) * F(depth_scale), raw != 0
        elif depth.dtype == np.float32:
            z, kept = raw.astype(F), np.ones(len(pixels), bool)
        else:
            raise ValueError("depth image: uint16 or float32, got %s" % depth.dtype)
        with np.errstate(invalid="ignore"):
            kept = kept & np.isfinite(z) & (F(depth_min) <= z) & (z <= F(depth_max))
    ifx, ify = F(1.0) / K[0, 0], F(1.0) / K[1, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((c.astype(F) - K[0, 2]) * ifx) * z
        y = ((r.astype(F) - K[1, 2]) * ify) * z
    return np.stack([x, y, z], -1).astype(F), kept


def extract(img, K=None, fast_threshold=20, max_features=1000, oriented=True, depth=None, depth_scale=0.001, depth_min=0.4,
            depth_max=8.0):
    """dict(points (n, 3) f32, intensity (n,) f32, descriptors (n, 32) u8, global_indices (n,) i32, keypoints (n, 3) i32 of
    pixel / score / angle_bin, and the counters of srrg2_feature_result)"""
    I = np.asarray(img)
    if I.dtype != np.uint8 or I.ndim != 2:
        raise ValueError("intensity image: 2-D uint8")
    rows, cols = I.shape
    K = np.eye(3, dtype=F) if K is None else K
    score = fast_score(I)
    cand, kp = maxima(score, fast_threshold)
    pix = np.flatnonzero(kp.reshape(-1))
    sc = score.reshape(-1)[pix]
    sel = cap(pix, sc, max_features)
    pix, sc = pix[sel], sc[sel]
    pts, kept = keypoint_points(pix, cols, K, depth, depth_scale, depth_min, depth_max)
    out = {"num_pixels": rows * cols, "num_candidates": int(cand.sum()), "num_maxima": int(kp.sum()), "num_selected": len(pix),
           "num_with_depth": int(kept.sum()), "scene_size": int(kept.sum()), "status": 1 if rows * cols == 0 else 0}
    pix, sc, pts = pix[kept], sc[kept], pts[kept]
    B = box_sums(I)
    pats = {}
    bins, desc = [], []
    for p in pix:
        r, c = divmod(int(p), cols)
        k = orientation_bin(I, r, c, oriented)
        if k not in pats:
            pats[k] = rotated_pattern(k)
        bins.append(k)
        desc.append(describe(B, r, c, pats[k]))
    out.update(points=pts.reshape(-1, 3), intensity=I.reshape(-1)[pix].astype(F), global_indices=pix.astype(np.int32),
               descriptors=np.array(desc, np.uint8).reshape(-1, 32),
               keypoints=np.stack([pix, sc, np.array(bins, np.int64)], -1).astype(np.int32).reshape(-1, 3))
    return out
