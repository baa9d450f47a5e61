"""Images at camera resolutions, past the launch caps of the image-feature and stereo kernels, and what the device has to make of
them.  numpy only: the builders and references here know nothing of the library (tests/test_image_large_cases.py checks them on
the CPU, tests/test_gpu_image_large.py runs the device on them).

FEAT_CAP: `blocks_of()` (csrc/features.hip) launches k_feat_tie, k_feat_select and k_feat_scatter with at most 1024 workgroups of
256 threads; an image of more pixels sends every thread round its grid-stride loop again ("trip" t covers the pixels
t * FEAT_CAP .. (t + 1) * FEAT_CAP - 1).  Crossing the cap is not enough: keypoints have to lie in the later trips, and the margin
of 16 pixels keeps them out of the last 16 rows.

STEREO_COUNT_CAP: srrg2_adapt_stereo_features (csrc/stereo.hip) launches k_stereo_count with at most 64 workgroups of 256 threads;
more left keypoints than that send it round its loop again.

Not built here: k_stereo_scatter goes through `blocks_for()` (csrc/scene_device.h), whose cap of 2048 * 256 = 524 288 threads
would need that many keypoints in one image (the row table and the band search, csrc/desc_band.hip, have one thread or wave per
element and no capped launch: there is no loop to reach); and the exclusive scan's second level needs more than 4 194 304
pixels (tests/test_gpu_scene_large.py drives the same launch_exclusive_scan there).
"""
import numpy as np

import features_cases as fc
import features_restatement as fr
import stereo_cases as sc
import stereo_restatement as sr

F = np.float32
FEAT_CAP = 1024 * 256  # features.hip blocks_of(): b > 1024 ? 1024 : b workgroups, launched with dim3(256) threads
STEREO_COUNT_CAP = 64 * 256  # stereo.hip, the k_stereo_count launch: dim3(count_blocks < 64 ? count_blocks : 64), dim3(256)
TILE_W, TILE_H = 64, 16  # features.hip: the tile of k_feat_score_box; the score and box images have a pitch of whole tiles
CAMERA, BASELINE = sc.CAMERA, sc.BASELINE

# name -> (rows, cols, seed) of features_cases.rectangles
#   vga  cols a multiple of the tile width: pitch == cols; two trips
#   odd  neither side a multiple of a tile, pitch 512 != 509; two trips; at threshold 0 more keypoints than STEREO_COUNT_CAP
#   hd   four trips, a partial tile on both edges
RECTANGLES = {"vga": (480, 640, 480640), "odd": (563, 509, 563509), "hd": (723, 1283, 7231283)}
TILED_REPEATS = (24, 21)  # of the 24 x 24 block of features_cases.tiled_image(): 576 x 504
FEATURE_NAMES = ("vga", "odd", "hd", "tiled_large")
DEPTH_NAMES = ("vga", "odd")
STEREO_NAMES = ("vga", "odd", "hd")
# (pair, parameters) the device is held to; max_features 0 unless it says otherwise, as in stereo_cases.want
DENSE = dict(fast_threshold=0, row_tolerance=2)
STEREO_CASES = (("vga", dict()), ("odd", DENSE), ("odd", dict(cross_check=False, **DENSE)), ("hd", dict(max_features=1000)))

_IMAGES, _DEPTHS, _EXTRACTED, _WANT, _CAPS = {}, {}, {}, {}, {}


def image(name, side="left"):
    """the case image of a name (treat it as read-only); side 'right': stereo_cases.shifted of it, bands of 40 rows"""
    key = (name, side)
    if key not in _IMAGES:
        if side == "right":
            left = image(name)
            _IMAGES[key] = sc.shifted(left, 77 * left.shape[0] + left.shape[1])
        elif name == "tiled_large":
            _IMAGES[key] = np.tile(fc.tiled_image()[:24, :24], TILED_REPEATS)
        else:
            _IMAGES[key] = fc.rectangles(*RECTANGLES[name])
    return _IMAGES[key]


def depth(name, kind):
    """features_cases.depth_for under the case image; kind 'u16' or 'f32'"""
    if (name, kind) not in _DEPTHS:
        _DEPTHS[(name, kind)] = fc.depth_for(image(name), kind)
    return _DEPTHS[(name, kind)]


def trip_of(pixels):
    """the trip of k_feat_tie / k_feat_select / k_feat_scatter's grid-stride loop that takes each pixel index"""
    return np.asarray(pixels, np.int64) // FEAT_CAP


def pitch_of(cols):
    """features.hip feat_queue_select: the row pitch of the score and box-sum images"""
    return -(-cols // TILE_W) * TILE_W


def want_features(name, threshold=20, max_features=0, depth_kind=None, side="left"):
    """features_restatement.extract of a case image, computed once per parameter set and shared (treat it as read-only)"""
    key = (name, side, threshold, max_features, depth_kind)
    if key not in _EXTRACTED:
        d = None if depth_kind is None else depth(name, depth_kind)
        _EXTRACTED[key] = fr.extract(image(name, side), K=CAMERA, fast_threshold=threshold, max_features=max_features, depth=d)
    return _EXTRACTED[key]


def tiled_caps():
    """dict of max_features values for `tiled_large` at threshold 20, derived from the restatement:
    boundary  as features_cases.tie_caps has it: everything down to and including the largest score class -- the quota is the
              whole class, whose members lie on both sides of pixel FEAT_CAP
    past      the quota ends halfway through the members of that class that lie at or past pixel FEAT_CAP
    and cut (the class's score), below / past_members (its members before / from pixel FEAT_CAP on), above (keypoints of higher
    scores).  From the shared uncapped extraction; tests/test_image_large_cases.py holds `boundary` to features_cases.tie_caps."""
    if not _CAPS:
        full = want_features("tiled_large")
        pix, score = full["keypoints"][:, 0].astype(np.int64), full["keypoints"][:, 1]
        classes, counts = np.unique(score, return_counts=True)
        cut = int(classes[np.argmax(counts)])  # (the first of equal counts, classes ascending: tie_caps' choice)
        members = pix[score == cut]  # ascending: the order of the quota
        above, below = int((score > cut).sum()), int((members < FEAT_CAP).sum())
        past = len(members) - below
        _CAPS.update(boundary=above + len(members), past=above + below + past // 2, cut=cut, above=above, below=below, past_members=past)
    return _CAPS


# ---- the row-banded stereo restatement --------------------------------------------------------------------------------------
def _best_in_bands(q_desc, q_row, q_col, c_desc, c_row, c_col, tolerance, dmin, dmax, sign):
    """per query keypoint, among the candidates in the rows q_row +- tolerance: what stereo_restatement.match reads off its
    all-pairs table -- best (candidate index of the smallest (distance, index) inside the disparity gate, -1 without one), its
    distance (-1), tied, the band's size and the number of candidates inside the gate.  Both sets are in raster order, so a band
    is one contiguous range of candidates and the order inside it is the order of the whole.
    sign +1: the queries are left keypoints, d = q_col - c_col; -1: right ones, d = c_col - q_col."""
    nq = len(q_row)
    best, dist = np.full(nq, -1, np.int64), np.full(nq, -1, np.int64)
    tied, band, gated = np.zeros(nq, bool), np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    if nq == 0 or len(c_row) == 0:
        return best, dist, tied, band, gated
    rows, first = np.unique(q_row, return_index=True)
    last = np.r_[first[1:], nq]
    begin, end = np.searchsorted(c_row, rows - tolerance, "left"), np.searchsorted(c_row, rows + tolerance, "right")
    for q0, q1, b, e in zip(first, last, begin, end):
        band[q0:q1] = e - b
        if e == b:
            continue
        h = sr.hamming(q_desc[q0:q1], c_desc[b:e])
        d = sign * (q_col[q0:q1, None] - c_col[None, b:e])
        allowed = (d >= dmin) & (d <= dmax)
        j, t = sr.best_candidates(h, allowed)  # (the tie rule itself: smallest distance, then smallest candidate index)
        has = j >= 0
        gated[q0:q1], tied[q0:q1] = allowed.sum(1), t
        best[q0:q1] = np.where(has, j + b, -1)
        dist[q0:q1] = np.where(has, h[np.arange(q1 - q0), np.maximum(j, 0)], -1)
    return best, dist, tied, band, gated


def match_banded(left, right, K, baseline, fast_threshold=20, max_features=1000, oriented=True, depth_min=0.4, depth_max=8.0,
                 min_disparity=1, max_disparity=128, row_tolerance=1, max_distance=48, cross_check=True, subpixel=True, extracted=None):
    """stereo_restatement.match -- the same contract, the same dict -- without its (num_left, num_right) tables: per image row
    only the other image's keypoints in the rows r +- row_tolerance are looked at, the cross check the same way round.
    tests/test_image_large_cases.py holds it to stereo_restatement.match on every case of stereo_cases.all_cases()."""
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
    best_l, hbest, tied, band, gated = _best_in_bands(eL["descriptors"], rl, cl, eR["descriptors"], rr, cr, row_tolerance,
                                                      min_disparity, max_disparity, 1)
    idx = np.arange(nl)
    matched = (best_l >= 0) & (hbest <= max_distance)
    mutual = matched.copy()
    if cross_check:
        best_r = _best_in_bands(eR["descriptors"], rr, cr, eL["descriptors"], rl, cl, row_tolerance, min_disparity, max_disparity, -1)[0]
        mutual &= best_r[np.maximum(best_l, 0)] == idx if nr else False
    fb = F(np.asarray(K, F).reshape(9)[0]) * F(baseline)
    disparity, z = np.zeros(nl, F), np.zeros(nl, F)
    cost3, curv = np.zeros((nl, 3), np.int64), np.zeros(nl, np.int64)
    for i in np.flatnonzero(mutual):
        j = best_l[i]
        off = F(0.0)
        if subpixel:
            cost3[i] = sr.costs(L, R, int(rl[i]), int(cl[i]), int(rr[j]), int(cr[j]))
            off, curv[i] = sr.offset(*(int(v) for v in cost3[i]))
        disparity[i] = F(cl[i] - cr[j]) - off
        z[i] = fb / disparity[i]
    depth_img = np.zeros((rows, cols), F)
    depth_img.reshape(-1)[pl[mutual]] = z[mutual]
    pts, in_range = fr.keypoint_points(pl, cols, K, depth_img, depth_min=depth_min, depth_max=depth_max)
    keep = mutual & in_range
    ms = np.zeros(int(keep.sum()), sr.MATCH_DTYPE)
    ms["left_pixel"], ms["right_pixel"] = pl[keep], pr[best_l[keep]]
    ms["distance"], ms["disparity"] = hbest[keep], disparity[keep]
    details = dict(band_size=band, num_candidates=gated, best=best_l, distance=hbest, tied=tied, matched=matched, mutual=mutual,
                   kept=keep, costs=cost3, curvature=curv, disparity=disparity, z=z, left_pixel=pl, right_pixel=pr)
    return dict(points=pts[keep].reshape(-1, 3), intensity=eL["intensity"][keep], descriptors=eL["descriptors"][keep].reshape(-1, 32),
                global_indices=eL["global_indices"][keep], keypoints=eL["keypoints"][keep].reshape(-1, 3), matches=ms,
                status=1 if rows * cols == 0 else 0, num_pixels=rows * cols, num_left=nl, num_right=nr,
                num_matched=int(matched.sum()), num_mutual=int(mutual.sum()), num_in_range=int(keep.sum()), scene_size=int(keep.sum()),
                details=details, left=eL, right=eR)


def want_stereo(name, **kw):
    """match_banded of a case pair, computed once per parameter set and shared (treat it as read-only); the two extractions are
    want_features' own, shared with the feature tests and between the calls that differ in the stereo parameters only"""
    kw.setdefault("max_features", 0)
    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        t, m = kw.get("fast_threshold", 20), kw["max_features"]
        extracted = (want_features(name, t, m), want_features(name, t, m, side="right"))
        _WANT[key] = match_banded(image(name), image(name, "right"), CAMERA, BASELINE, extracted=extracted, **kw)
    return _WANT[key]
