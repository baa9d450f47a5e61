"""Seeded stereo pairs and case lists of the stereo-feature tests (tests/test_gpu_stereo.py, tests/test_stereo_restatement.py).

The left image is a features_cases image; the right image is the left one shifted by a disparity that is constant per horizontal
band (right(r, c) = left(r, c + d_band)), the columns the shift exposes filled with noise.  Bands are at least 40 rows tall, so a
keypoint whose 31 x 31 window lies inside one band has the same score, angle and descriptor in both images.  Nothing here knows
the library.
"""
import numpy as np

import features_cases as fc

SIZES = fc.SIZES
CAMERA = fc.CAMERA
BASELINE = 0.1  # with fx = 525: z = 52.5 / disparity, so a disparity of 5 lies beyond depth_max = 8 and one of 140 below depth_min
BAND_ROWS = 40
# disparity of band k (cycled): 5 is gated out by depth_max, the others are kept
DISPARITIES = (12, 5, 20)


def bands(rows):
    """[(first row, one past the last row, disparity)]: bands of BAND_ROWS rows, the last one takes the remainder"""
    count = max(rows // BAND_ROWS, 1)
    out = []
    for k in range(count):
        out.append((k * BAND_ROWS, rows if k == count - 1 else (k + 1) * BAND_ROWS, DISPARITIES[k % len(DISPARITIES)]))
    return out


def shifted(left, seed, band_list=None):
    """the right image of `left`: every band shifted by its disparity, the exposed columns filled with uniform noise"""
    rows, cols = left.shape
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    for r0, r1, d in (bands(rows) if band_list is None else band_list):
        right[r0:r1, :cols - d] = left[r0:r1, d:]
    return right


def pair(rows, cols, rotated=False):
    left = fc.image(rows, cols, rotated)
    return left, shifted(left, 77 * rows + cols + (1 if rotated else 0))


def pairs():
    """[(name, left, right)]: every size plain and rotated"""
    out = []
    for rows, cols in SIZES:
        for rot in (False, True):
            left, right = pair(rows, cols, rot)
            out.append(("%dx%d%s" % (rows, cols, "_rot" if rot else ""), left, right))
    return out


def band_of(rows, r):
    """(disparity, interior): the band of row r, and whether the 31 x 31 window around that row lies inside it"""
    for r0, r1, d in bands(rows):
        if r0 <= r < r1:
            return d, (r - 15 >= r0 and r + 15 < r1)
    raise ValueError(r)


def blank_like(img):
    return np.full(img.shape, 110, np.uint8)


# ---- the case lists -----------------------------------------------------------------------------------------------------
# every variant runs on every pair (max_features 0 unless it says otherwise): each switch both ways, the row tolerances, the
# two ends of the distance gate
VARIANTS = (dict(), dict(oriented=False), dict(cross_check=False), dict(subpixel=False), dict(row_tolerance=0), dict(row_tolerance=8),
            dict(max_distance=0), dict(max_distance=256, cross_check=False), dict(min_disparity=6, max_disparity=15))
# every admissible local maximum is a keypoint: row bands of more than 64 keypoints, ties of the Hamming distance
DENSE = (dict(fast_threshold=0, row_tolerance=2, max_distance=256, cross_check=False),
         dict(fast_threshold=0, row_tolerance=8, max_distance=256), dict(fast_threshold=0, row_tolerance=8, subpixel=False))
DENSE_PAIR = "120x160"
TILED_DISPARITY = 10
TILED = (dict(max_disparity=40, cross_check=False), dict(max_disparity=40), dict(max_disparity=20))

# a gate of ONE column (min_disparity == max_disparity), in both directions: left -> right it admits the column c - 12 only,
# right -> left the column c + 12 only.  The wide row band and the open distance gate give the right keypoints several left
# keypoints to choose from, so that the cross check has something to reject (tests/test_stereo_restatement.py pins it)
ONE_COLUMN_PAIR = "120x160"
ONE_COLUMN_DISPARITY = 12
ONE_COLUMN = tuple(dict(min_disparity=ONE_COLUMN_DISPARITY, max_disparity=ONE_COLUMN_DISPARITY, row_tolerance=8, max_distance=256,
                        cross_check=cross) for cross in (True, False))

_PAIRS = {}
_EXTRACTED = {}
_WANT = {}


def named(name):
    """(left, right) of a case name: a size (plain or _rot), 'tiled', 'blank' (96x128 against a flat right image)"""
    if not _PAIRS:
        for n, left, right in pairs():
            _PAIRS[n] = (left, right)
        left = fc.tiled_image()
        _PAIRS["tiled"] = (left, shifted(left, 4242, [(0, left.shape[0], TILED_DISPARITY)]))
        _PAIRS["blank"] = (_PAIRS["96x128"][0], blank_like(_PAIRS["96x128"][0]))
        _PAIRS["32x40"] = (fc.rectangles(32, 40, 1), fc.rectangles(32, 40, 2))
        _PAIRS["0x0"] = (np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8))
    return _PAIRS[name]


def want(name, **kw):
    """the restatement's result for a named pair, computed once and shared by the tests (treat it as read-only); the two
    extractions are shared between the calls that differ in the stereo parameters only"""
    import features_restatement as fr
    import stereo_restatement as sr

    kw.setdefault("max_features", 0)
    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        fkw = {k: kw[k] for k in ("fast_threshold", "max_features", "oriented") if k in kw}
        fkey = (name, tuple(sorted(fkw.items())))
        if fkey not in _EXTRACTED:
            _EXTRACTED[fkey] = tuple(fr.extract(I, K=CAMERA, **fkw) for I in named(name))
        _WANT[key] = sr.match(*named(name), CAMERA, BASELINE, extracted=_EXTRACTED[fkey], **kw)
    return _WANT[key]


def all_cases():
    """[(pair name, parameters)]: everything the GPU test compares bit for bit and the CPU test draws its pins from"""
    out = [(n, v) for n, _, _ in pairs() for v in VARIANTS]
    out += [(DENSE_PAIR, v) for v in DENSE] + [("tiled", v) for v in TILED] + [(ONE_COLUMN_PAIR, v) for v in ONE_COLUMN]
    return out
