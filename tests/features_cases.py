"""Seeded images and case lists of the image-feature tests (tests/test_gpu_features.py, tests/test_features_restatement.py).

Image content: random rectangles of random grey levels on a flat ground plus +-3 noise -- corners, T-junctions and plateaus of
equal scores -- every image also rotated by 90 degrees.  Nothing here knows the library.
"""
import numpy as np

import features_restatement as fr

# rows x cols: neither side of 67 x 101 is a multiple of a tile; 120 x 160 spans several tile rows; 33 x 33 holds one admissible
# pixel, 32 x 40 none
SIZES = ((48, 64), (67, 101), (96, 128), (120, 160))
THRESHOLDS = (0, 20, 254)


def rectangles(rows, cols, seed, noise=3):
    """uint8 (rows, cols): about one rectangle per 150 pixels, sides 4 .. 24, grey 20 .. 235, then integer noise in +-noise"""
    rng = np.random.default_rng(seed)
    I = np.full((rows, cols), 110, np.int32)
    for _ in range(max(rows * cols // 150, 1)):
        h, w = rng.integers(4, 25, 2)
        r, c = rng.integers(-4, rows), rng.integers(-4, cols)
        I[max(r, 0):r + h, max(c, 0):c + w] = rng.integers(20, 236)
    if noise:
        I += rng.integers(-noise, noise + 1, (rows, cols))
    return np.clip(I, 0, 255).astype(np.uint8)


def image(rows, cols, rotated=False):
    """the test image of a size; rotated: the image of the transposed size turned by 90 degrees"""
    if rotated:
        return np.ascontiguousarray(np.rot90(rectangles(cols, rows, 1000 * cols + rows)))
    return rectangles(rows, cols, 1000 * rows + cols)


def images():
    """[(name, image)]: every size plain and rotated"""
    out = []
    for rows, cols in SIZES:
        out.append(("%dx%d" % (rows, cols), image(rows, cols)))
        out.append(("%dx%d_rot" % (rows, cols), image(rows, cols, True)))
    return out


def quadrant_image(mirrored=False):
    """33 x 33, 100 everywhere and 200 in the lower-right quadrant from (16, 16): one keypoint, pixel 544, score 100, bin 4.
    mirrored (both axes): the surviving maximum of the corner's plateau falls outside the margin, no keypoint"""
    I = np.full((33, 33), 100, np.uint8)
    I[16:, 16:] = 200
    return np.ascontiguousarray(I[::-1, ::-1]) if mirrored else I


def tiled_image():
    """a 24 x 24 block tiled 4 x 5 to 96 x 120: every keypoint of the block's interior repeats with the same score, so the
    score classes hold many equal members and the cap's cut falls inside one (121 keypoints in 11 classes of 6 .. 24)"""
    block = rectangles(24, 24, 74, noise=0)
    rng = np.random.default_rng(75)
    block = np.clip(block.astype(np.int32) + rng.integers(-3, 4, block.shape), 0, 255).astype(np.uint8)
    return np.tile(block, (4, 5))


def tie_caps(img, threshold=20):
    """max_features values that put the cut inside a score class, at a class boundary, at 1 and above the count; with the
    uncapped result they come from"""
    full = fr.extract(img, fast_threshold=threshold, max_features=0)
    scores = full["keypoints"][:, 1]
    n = len(scores)
    classes, counts = np.unique(scores, return_counts=True)
    big = int(np.argmax(counts))  # the largest class, classes ascending
    above = int(counts[big + 1:].sum())
    inside = above + int(counts[big]) // 2
    boundary = above + int(counts[big])
    return full, {"inside": inside, "boundary": boundary, "one": 1, "above": n + 5}


def depth_for(img, kind, seed=5):
    """a depth image under `img` with holes (0 / NaN), values below depth_min and beyond depth_max; kind: 'u16' or 'f32'"""
    rows, cols = img.shape
    rng = np.random.default_rng(seed + rows * 7 + cols)
    r, c = np.mgrid[0:rows, 0:cols]
    z = 1.5 + 0.01 * r + 0.004 * c + 0.3 * np.sin(c / 9.0)
    pick = rng.integers(0, 10, (rows, cols))
    if kind == "u16":
        d = np.round(z * 1000.0).astype(np.uint16)
        d[pick == 0] = 0        # no reading
        d[pick == 1] = 200      # nearer than depth_min
        d[pick == 2] = 60000    # beyond depth_max
        return d
    d = z.astype(np.float32)
    d[pick == 0] = np.nan
    d[pick == 1] = np.float32(0.1)
    d[pick == 2] = np.inf
    d[pick == 3] = np.float32(-1.0)
    return d


CAMERA = (525.0, 0.0, 80.5, 0.0, 520.0, 61.25, 0.0, 0.0, 1.0)


def crops():
    """two 96 x 128 crops of one 120 x 160 image, shifted by (7, 11) whole pixels: ((r0, c0), crop) twice"""
    big = image(120, 160)
    return ((5, 9), np.ascontiguousarray(big[5:101, 9:137])), ((12, 20), np.ascontiguousarray(big[12:108, 20:148]))
