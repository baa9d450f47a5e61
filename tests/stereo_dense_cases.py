"""Seeded pairs and case lists of the dense-stereo tests (tests/test_gpu_stereo_dense.py, tests/test_stereo_dense_restatement.py).

Pairs: the stereo_cases pairs (disparity constant per band of rows), the two-plane pair (a background at disparity 6 and a
foreground rectangle at 14 painted over it, with the occlusion that makes), a flat pair, the tiled pair (two disparities tie)
and small noise pairs.  Nothing here knows the library.
"""
import numpy as np

import features_cases as fc
import stereo_cases as sc

CAMERA = fc.CAMERA
BASELINE = 0.05  # with fx = 525: z = 26.25 / disparity, so disparities 3.3 .. 65 lie inside the depth gate 0.4 .. 8 m
TWO_PLANE_SIZES = fc.SIZES
BACKGROUND, FOREGROUND = 6, 14
TWO_PLANE_RANGE = dict(min_disparity=1, max_disparity=24)


def foreground(rows, cols):
    """(first row, one past the last row, first column, one past the last column): rows 24 .. 71 x cols 52 .. 94 at 96 x 128"""
    return rows // 4, 3 * rows // 4, 13 * cols // 32, 95 * cols // 128


def two_plane(rows, cols):
    """(left, right, truth, visible): the right image is uniform noise of seed 9 with the background painted at c - 6 and then
    the foreground over it at c - 14; visible: inside the processed rectangle of the range 1 .. 24 and not a background pixel
    whose right position the foreground covers"""
    left = fc.image(rows, cols)
    r0, r1, c0, c1 = foreground(rows, cols)
    truth = np.full((rows, cols), BACKGROUND, np.int64)
    truth[r0:r1, c0:c1] = FOREGROUND
    right = np.random.default_rng(9).integers(0, 256, (rows, cols)).astype(np.uint8)
    back = np.zeros((rows, cols), bool)  # in the right image: where a background pixel lands
    back[:, :cols - BACKGROUND] = truth[:, BACKGROUND:] == BACKGROUND
    right[back] = np.roll(left, -BACKGROUND, 1)[back]
    right[r0:r1, c0 - FOREGROUND:c1 - FOREGROUND] = left[r0:r1, c0:c1]
    covered = np.zeros((rows, cols), bool)  # in the right image
    covered[r0:r1, c0 - FOREGROUND:c1 - FOREGROUND] = True
    occluded = np.zeros((rows, cols), bool)
    occluded[:, BACKGROUND:] = covered[:, :cols - BACKGROUND]
    occluded &= truth == BACKGROUND
    rect = np.zeros((rows, cols), bool)
    rect[3:rows - 3, 4 + TWO_PLANE_RANGE["max_disparity"]:cols - 4] = True
    return left, right, truth, rect & ~occluded


def noise_pair(rows, cols, seed, shift):
    """a noise image and itself moved left by `shift`, fresh noise in the exposed columns"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    right = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    right[:, :cols - shift] = left[:, shift:]
    return left, right


_PAIRS = {}


def named(name):
    """(left, right) of a case name: a stereo_cases name, 'two_plane_RxC', 'flat' (48 x 64 of one grey level), 'tiled',
    'noise_RxC' (shift 3) or 'noise_RxC_sN' (shift N), 'rand_RxC' (unrelated noise), '0x0'"""
    if name not in _PAIRS:
        if name.startswith("two_plane_"):
            rows, cols = (int(v) for v in name[len("two_plane_"):].split("x"))
            _PAIRS[name] = two_plane(rows, cols)[:2]
        elif name.startswith("noise_"):
            size, _, shift = name[len("noise_"):].partition("_s")
            rows, cols = (int(v) for v in size.split("x"))
            _PAIRS[name] = noise_pair(rows, cols, 31 * rows + cols, int(shift) if shift else 3)
        elif name.startswith("rand_"):  # two unrelated noise images: nothing to find, every test has something to reject
            rows, cols = (int(v) for v in name[len("rand_"):].split("x"))
            rng = np.random.default_rng(17 * rows + cols)
            _PAIRS[name] = tuple(rng.integers(0, 256, (rows, cols)).astype(np.uint8) for _ in range(2))
        elif name == "flat":
            _PAIRS[name] = (np.full((48, 64), 110, np.uint8), np.full((48, 64), 110, np.uint8))
        else:
            _PAIRS[name] = sc.named(name)
    return _PAIRS[name]


# every variant runs on every pair: the two path counts, the ends of the penalties, the ends of the uniqueness ratio, each
# switch both ways, the strictest left-right check
VARIANTS = (dict(), dict(paths=0), dict(p1=0, p2=0), dict(p1=255, p2=255), dict(uniqueness_ratio=0), dict(uniqueness_ratio=99),
            dict(lr_check=0), dict(lr_tolerance=0), dict(subpixel=0), dict(paths=0, subpixel=0, lr_tolerance=0))
PAIR_RANGE = dict(min_disparity=1, max_disparity=24)  # the band disparities 5, 12 and 20 lie inside
# disparity counts around the wave width on 120 x 160, from min_disparity 11 (the band at 12 is inside even the shortest range);
# 129 leaves a rectangle of 160 - 8 - 139 = 13 columns
ND_PAIR = "120x160"
ND_COUNTS = (1, 2, 3, 63, 64, 65, 128, 129)
ND_MIN = 11
# 256 disparities need 265 columns: a 20 x 300 strip of noise, shift 40
STRIP = ("noise_20x300_s40", dict(min_disparity=1, max_disparity=256))
# rectangle widths 1, 63, 64 and 65 with 8 disparities 3 .. 10 (cols = width + 18) on noise shifted by 5, one row high (rows = 7)
WIDTHS = (1, 63, 64, 65)
WIDTH_RANGE = dict(min_disparity=3, max_disparity=10)
WIDTH_NAME = "noise_%dx%d_s5"

_WANT = {}


def want(name, **kw):
    """the restatement's result for a named pair, computed once and shared by the tests (treat it as read-only)"""
    import stereo_dense_restatement as sd

    key = (name, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = sd.adapt(*named(name), CAMERA, BASELINE, **kw)
    return _WANT[key]
