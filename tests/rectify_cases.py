"""Camera models, target shapes, seeded images and the warped stereo pair of the rectification tests
(tests/test_rectify_restatement.py, tests/test_gpu_rectify.py, tests/test_rectify_cpp.py).  Nothing here knows the library.
"""
import math

import numpy as np

import features_cases as fc
import stereo_dense_cases as dc

F64 = np.float64


def K3(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], F64)


def rotation(axis, angle):
    """rotation by `angle` about 'x' or 'y'"""
    c, s = math.cos(angle), math.sin(angle)
    if axis == "y":
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], F64)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], F64)


_VGA = dict(K=K3(500.0, 505.0, 318.3, 241.7), shape=(480, 640))
_SMALL = dict(K=K3(40.0, 41.0, 26.2, 18.4), shape=(37, 53))
# name -> K, source shape, distortion (k1, k2, p1, p2, k3, k4, k5, k6), rotation (None: the case's own)
MODELS = {
    "vga_barrel": dict(_VGA, distortion=(-0.28, 0.07, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)),
    "vga_rational": dict(_VGA, distortion=(0.1, -0.05, 2e-4, 3e-4, 0.01, 0.4, -0.1, 0.02)),
    "pincushion": dict(_VGA, distortion=(0.15, 0.02, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    "small": dict(_SMALL, distortion=(-0.2, 0.04, 2e-3, -1e-3, 0.0, 0.0, 0.0, 0.0)),
    "behind": dict(_SMALL, distortion=(-0.2, 0.04, 2e-3, -1e-3, 0.0, 0.0, 0.0, 0.0), rotation=rotation("y", math.radians(100.0))),
    "identity": dict(_SMALL, distortion=(0.0,) * 8),
}
DISTORTING = ("vga_barrel", "vga_rational", "pincushion", "small", "behind")
ROTATIONS = {"identity": None, "tilted": rotation("y", 0.03)}
# the tails and the tile edges: one pixel, one short row, a few rows, neither side a multiple of the 64 x 16 tile (53 and 101
# columns: cols % 4 = 1), and the one target above 101 columns
SHAPES = ((1, 1), (1, 7), (3, 5), (37, 53), (67, 101), (480, 640))
SMALL_SHAPES = SHAPES[:-1]
# `behind` on a target of its source's shape has no valid entry (W <= 0 left of column 33, the rest looks far past the source's
# edge); on this wider target with the same K the columns from 95 on see the source again: valid and invalid entries side by side
BEHIND_WIDE = (37, 140)


def model(name, rot="identity"):
    """(K, distortion, rotation, source shape); a model with a rotation of its own keeps it"""
    m = MODELS[name]
    R = m.get("rotation")
    if R is None:
        R = ROTATIONS[rot]
    return m["K"], np.array(m["distortion"], F64), (np.eye(3) if R is None else R), m["shape"]


def target_K(name, dst_shape):
    """the source's K scaled to the target's shape: the target sees what the source sees, at another resolution"""
    K, shape = MODELS[name]["K"], MODELS[name]["shape"]
    sy, sx = dst_shape[0] / shape[0], dst_shape[1] / shape[1]
    return K3(K[0, 0] * sx, K[1, 1] * sy, K[0, 2] * sx, K[1, 2] * sy)


_IMAGES = {}


def image(shape, kind="u8"):
    """the seeded image of a shape: 'u8' rectangles with noise, 'u16' / 'f32' a depth image with holes under it"""
    key = (tuple(shape), kind)
    if key not in _IMAGES:
        rows, cols = shape
        img = fc.rectangles(rows, cols, 77 * rows + cols)
        _IMAGES[key] = img if kind == "u8" else fc.depth_for(img, kind)
    return _IMAGES[key]


def nan_payload_image(shape):
    """float32 whose every pixel is a NaN with a payload of its own, signalling and quiet, both signs"""
    rows, cols = shape
    i = np.arange(rows * cols, dtype=np.uint32).reshape(rows, cols)
    bits = np.uint32(0x7f800001) + (i * np.uint32(2654435761) & np.uint32(0x007ffffe)) | ((i & np.uint32(1)) << np.uint32(31))
    return bits.astype(np.uint32).view(np.float32)


def undistort_normalised(xd, yd, distortion, steps=30):
    """the inverse of the distortion by fixed-point iteration: normalised distorted -> normalised ideal coordinates"""
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in distortion)
    x, y = np.array(xd, F64), np.array(yd, F64)
    for _ in range(steps):
        r2 = x * x + y * y
        rad = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x, y


def source_to_target(u, v, K, distortion, R, new_K):
    """where source pixel coordinates (u, v) fall in the target: the inverse of the map's model"""
    xd, yd = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    xn, yn = undistort_normalised(xd, yd, distortion)
    X = R[0, 0] * xn + R[0, 1] * yn + R[0, 2]
    Y = R[1, 0] * xn + R[1, 1] * yn + R[1, 2]
    Z = R[2, 0] * xn + R[2, 1] * yn + R[2, 2]
    return new_K[0, 0] * X / Z + new_K[0, 2], new_K[1, 1] * Y / Z + new_K[1, 2]


def warp_to_source(ideal, K, distortion, R, new_K, src_shape, seed):
    """the raw image a camera (K, distortion) turned by R against the ideal one would deliver: every source pixel sampled
    bilinearly from `ideal` (camera new_K) where it falls there, seeded noise where it falls outside"""
    rows, cols = src_shape
    v, u = np.mgrid[0:rows, 0:cols].astype(F64)
    c, r = source_to_target(u, v, K, distortion, R, new_K)
    out = np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)
    ok = (c >= 0) & (c <= ideal.shape[1] - 1) & (r >= 0) & (r <= ideal.shape[0] - 1)
    c0, r0 = np.floor(c[ok]).astype(np.int64), np.floor(r[ok]).astype(np.int64)
    c1, r1 = np.minimum(c0 + 1, ideal.shape[1] - 1), np.minimum(r0 + 1, ideal.shape[0] - 1)
    a, b = c[ok] - c0, r[ok] - r0
    I = ideal.astype(F64)
    val = I[r0, c0] * (1 - a) * (1 - b) + I[r0, c1] * a * (1 - b) + I[r1, c0] * (1 - a) * b + I[r1, c1] * a * b
    out[ok] = np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)
    return out


# the stereo rig of the front-end tests: two cameras of one K with `small`-like distortion, the right one turned by 0.02 rad
# about x (a vertical misalignment of 1.6 px at f = 80) and set 0.3 m to the right; the ideal pair is two_plane_67x101
RIG_NAME = "two_plane_67x101"
RIG_K = K3(80.0, 80.0, 50.0, 33.0)
RIG_DISTORTION = np.array((-0.2, 0.04, 2e-3, -1e-3, 0.0, 0.0, 0.0, 0.0), F64)
RIG_BASELINE = 0.3  # z = 24 / disparity: the two planes at disparity 6 and 14 lie at 4 m and 1.7 m
RIG_R = rotation("x", 0.02)
RIG_T = -RIG_R @ np.array([RIG_BASELINE, 0.0, 0.0], F64)
RIG_RANGE = dict(dc.TWO_PLANE_RANGE)
_RIG = {}


def rig():
    """dict: the ideal pair, the calibration's rotations and target camera (rectify_restatement.stereo_rectify), the raw pair
    the rig delivers, and per camera the arguments of build_map"""
    if not _RIG:
        import rectify_restatement as rr

        left, right = dc.named(RIG_NAME)
        R1, R2, Knew, baseline = rr.stereo_rectify(RIG_K, RIG_K, RIG_R, RIG_T)
        shape = left.shape
        raw_left = warp_to_source(left, RIG_K, RIG_DISTORTION, R1, Knew, shape, 401)
        raw_right = warp_to_source(right, RIG_K, RIG_DISTORTION, R2, Knew, shape, 402)
        _RIG.update(ideal=(left, right), R1=R1, R2=R2, Knew=Knew, baseline=baseline, raw=(raw_left, raw_right), shape=shape,
                    maps=tuple(rr.build_map(RIG_K, RIG_DISTORTION, R, Knew, shape, shape)[0] for R in (R1, R2)))
    return _RIG


def rig_rectified(border=0):
    """the restated rectified pair of the rig's raw pair"""
    import rectify_restatement as rr

    key = ("rectified", border)
    if key not in _RIG:
        g = rig()
        _RIG[key] = tuple(rr.remap(m, img, border) for m, img in zip(g["maps"], g["raw"]))
    return _RIG[key]
