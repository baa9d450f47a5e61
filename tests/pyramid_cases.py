"""Shared cases of the scale-pyramid tests (tests/test_pyramid_restatement.py, tests/test_gpu_pyramid.py): images, ratios and caps.

The images are those of features_cases.py.  Nothing here knows the library.
"""
import functools

import numpy as np

import features_cases as fc
import pyramid_restatement as pr

RATIOS = ((6, 5), (3, 2), (2, 1))
CAMERA = fc.CAMERA


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "quadrant":
        return fc.quadrant_image()
    if name == "tiled":
        return fc.tiled_image()
    if name == "frame":  # one camera frame: 8 levels at 6/5
        return fc.rectangles(480, 640, 4806)
    rows, cols = (int(v) for v in name.split("x"))
    return fc.image(rows, cols)


# (image, levels asked for, num, den): what each exercises stands in the GPU test's docstrings
CASES = (("48x64", 4, 6, 5), ("67x101", 4, 6, 5), ("67x101", 4, 2, 1), ("96x128", 4, 6, 5), ("96x128", 4, 3, 2), ("96x128", 3, 2, 1),
         ("tiled", 4, 6, 5), ("tiled", 3, 3, 2), ("tiled", 2, 2, 1), ("quadrant", 2, 6, 5), ("120x160", 8, 6, 5))


@functools.lru_cache(maxsize=None)
def reference(name, num_levels, num, den, max_features=0, oriented=True, depth=None, fast_threshold=20):
    """the restatement's result of a case, computed once (treat it as read-only); depth: None, 'u16' or 'f32'"""
    img = image(name)
    d = None if depth is None else depth_for(name, depth)
    return pr.extract_pyramid(img, K=CAMERA, fast_threshold=fast_threshold, max_features=max_features, oriented=oriented, depth=d,
                              num_levels=num_levels, num=num, den=den)


@functools.lru_cache(maxsize=None)
def depth_for(name, kind):
    return fc.depth_for(image(name), kind)


def upper_levels_depth(name, kind, num_levels=4, num=6, den=5):
    """a depth image, valid everywhere, with holes punched exactly at the level-0 pixels of the keypoints of levels >= 1 that no
    level-0 keypoint shares: it gates out keypoints of the upper levels only.  Returns (depth, pixels punched)"""
    img = image(name)
    ref = pr.extract_pyramid(img, K=CAMERA, max_features=0, num_levels=num_levels, num=num, den=den)
    kp = ref["keypoints"]
    mine = np.setdiff1d(kp[kp[:, 3] >= 1, 0], kp[kp[:, 3] == 0, 0])[::2]  # every other one, so that some stay
    d = np.full(img.shape, 2000, np.uint16) if kind == "u16" else np.full(img.shape, 2.0, np.float32)
    d.reshape(-1)[mine] = 0 if kind == "u16" else np.nan
    return d, mine


def cap_settings(name, num_levels=4, num=6, den=5):
    """max_features values of each kind for a case: one that gives the LAST level a quota of 0 while level 0 is cut, one that puts
    a tie at a level's cut (a level keeps fewer than its members of the cut score), one above every level's count"""
    full = reference(name, num_levels, num, den)
    sizes = list(zip(full["rows"], full["cols"]))
    area = sum(r * c for r, c in sizes)
    zero = (area - 1) // (sizes[-1][0] * sizes[-1][1])  # the largest cap with floor(cap * A_last / area) == 0
    out = {"zero_quota": zero, "above": 10 * max(full["num_maxima"]) * len(sizes) + 7}
    kp = full["keypoints"]
    for cap in range(len(sizes), max(full["num_maxima"]) * len(sizes)):
        for l, q in enumerate(pr.quotas(sizes, cap)):
            sc = np.sort(kp[kp[:, 3] == l, 1])[::-1]
            if 0 < q < len(sc) and sc[q - 1] == sc[q]:
                out["tie"] = cap
                return out
    raise AssertionError("no cap with a tie at a level's cut")


def scaled_pair(rows, cols, seed, num, den):
    """(A, B): an image and its resample by num/den (the scale property's pair)"""
    A = fc.rectangles(rows, cols, seed)
    return A, pr.resample(A, num, den)


def scale_counts(A, B, num, den, num_levels=4):
    """the restatement's correct-match counts of B's single-scale keypoints against A's single-scale and A's pyramid keypoints
    (mutual nearest neighbours, Hamming <= 64, within 3 * num/den pixels): (single, pyramid) and the pairs of the pyramid"""
    single = pr.extract_pyramid(A, max_features=0, num_levels=1)
    pyramid = pr.extract_pyramid(A, max_features=0, num_levels=num_levels)
    b = pr.extract_pyramid(B, max_features=0, num_levels=1)
    counts = []
    for a in (single, pyramid):
        ia, ib = pr.mutual_matches(a["descriptors"], b["descriptors"])
        counts.append(pr.correct_matches(a["keypoints"][:, 5:7].astype(np.float64), b["keypoints"][:, 5:7].astype(np.float64), ia, ib,
                                         num, den))
    return tuple(counts)
