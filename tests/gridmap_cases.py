"""The cases the occupancy-grid tests share (CPU: tests/test_gridmap_restatement.py, GPU: tests/test_gpu_gridmap.py): seeded
rectangular rooms, trajectories inside them, the scans a planar scanner takes there, and the list of shapes."""
import math

import numpy as np

import gridmap_restatement as gr

F = np.float32
PI = math.pi
GRIDS = ((1, 1), (1, 9), (7, 5), (64, 64), (129, 257))  # (rows, cols)
SCAN_COUNTS = (0, 1, 3, 65)
BEAM_COUNTS = (0, 1, 63, 64, 65, 361, 1081)
# (grid, K, num_beams): every grid, every K and every beam count at least once
SHAPES = (((1, 1), 1, 1), ((1, 9), 3, 63), ((7, 5), 3, 64), ((7, 5), 1, 65), ((64, 64), 65, 361), ((129, 257), 3, 1081),
          ((129, 257), 65, 65), ((64, 64), 0, 361), ((7, 5), 3, 0), ((1, 9), 0, 0))


def pose(x, y, theta):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s, x], [s, c, y], [0, 0, 1]], F)


def fan(num_beams, fov=1.5 * PI, clockwise=False):
    """(angle_min, angle_increment) of a scanner with num_beams over `fov` radians, centred on its x axis"""
    inc = fov / max(num_beams - 1, 1)
    return (0.5 * fov, -inc) if clockwise else (-0.5 * fov, inc)


def room_of(g, margin=0.12):
    """(xmin, xmax, ymin, ymax) of a room whose walls lie `margin` of the grid's extent inside it"""
    w, h = g["cols"] * float(g["res"]), g["rows"] * float(g["res"])
    return (float(g["ox"]) + margin * w, float(g["ox"]) + (1 - margin) * w, float(g["oy"]) + margin * h, float(g["oy"]) + (1 - margin) * h)


def trajectory(room, K, seed):
    """K seeded robot poses inside the middle of the room, (K, 3, 3) float32"""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = room
    xs = rng.uniform(x0 + 0.3 * (x1 - x0), x1 - 0.3 * (x1 - x0), K)
    ys = rng.uniform(y0 + 0.3 * (y1 - y0), y1 - 0.3 * (y1 - y0), K)
    th = rng.uniform(-PI, PI, K)
    return np.stack([pose(*v) for v in zip(xs, ys, th)]).reshape(K, 3, 3) if K else np.zeros((0, 3, 3), F)


def room_scans(room, poses, sc, sigma=0.0, seed=0):
    """(K, num_beams) float32 ranges from the SENSOR (pose * sensor_in_robot) to the walls of the room, float64 ray casting"""
    nb = sc["num_beams"]
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 3)
    K = poses.shape[0]
    if K * nb == 0:
        return np.zeros((K, nb), F)
    T = poses @ sc["sensor_in_robot"].astype(np.float64)
    th = np.arctan2(T[:, 1, 0], T[:, 0, 0])[:, None] + (sc["angle_min"] + np.arange(nb) * sc["angle_increment"])[None, :]
    dx, dy = np.cos(th), np.sin(th)
    ox, oy = T[:, 0, 2, None], T[:, 1, 2, None]
    x0, x1, y0, y1 = room
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(dx > 0, (x1 - ox) / dx, (x0 - ox) / dx)
        ty = np.where(dy > 0, (y1 - oy) / dy, (y0 - oy) / dy)
    tx = np.where(np.isfinite(tx) & (tx > 0), tx, np.inf)
    ty = np.where(np.isfinite(ty) & (ty > 0), ty, np.inf)
    r = np.minimum(tx, ty)
    if sigma > 0:
        r = r + np.random.default_rng(seed).normal(0.0, sigma, r.shape)
    return r.astype(F)


def mixed(ranges, seed):
    """a copy with one entry in five replaced: +inf, NaN, 0, below any minimum, -inf, far beyond any maximum, negative"""
    rng = np.random.default_rng(seed)
    r = np.array(ranges, F, copy=True)
    flat = r.reshape(-1)
    pick = rng.random(flat.size) < 0.2
    flat[pick] = rng.choice(np.array([np.inf, np.nan, 0.0, 1e-4, -np.inf, 1e4, -1.0], F), int(pick.sum()))
    return r


def shape_case(shape, seed=0, resolution=0.05, origin=(-1.0, 0.5), **scanner_kw):
    """grid, scanner, poses and ranges of one entry of SHAPES: a room inside the grid seen from a seeded trajectory"""
    (rows, cols), K, nb = shape
    g = gr.grid(rows, cols, resolution, origin)
    a0, inc = fan(nb)
    kw = dict(range_min=0.02, range_max=20.0)
    kw.update(scanner_kw)
    sc = gr.scanner(a0, inc, nb, **kw)
    room = room_of(g)
    poses = trajectory(room, K, seed)
    return g, sc, poses, room_scans(room, poses, sc, sigma=0.004, seed=seed + 1)
