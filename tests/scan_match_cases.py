"""The cases the scan-matching tests share (CPU: tests/test_scan_match_restatement.py, GPU: tests/test_gpu_scan_match.py): the
seeded room of tests/gridmap_cases.py with two boxes in it (they break the rectangle's symmetry), the map drawn from a trajectory
inside it, and the recovery setting -- a scan taken at a known pose, handed in with a guess that is off."""
import functools
import math

import numpy as np

import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_restatement as sm

F = np.float32


def boxes_of(room):
    """two axis-aligned boxes (xmin, xmax, ymin, ymax) near two opposite corners of the room, of different sizes"""
    x0, x1, y0, y1 = room
    w, h = x1 - x0, y1 - y0
    return ((x0 + 0.08 * w, x0 + 0.22 * w, y0 + 0.10 * h, y0 + 0.16 * h), (x0 + 0.70 * w, x0 + 0.80 * w, y0 + 0.78 * h, y0 + 0.92 * h))


def box_scans(room, boxes, poses, sc, sigma=0.0, seed=0):
    """(K, num_beams) float32 ranges from the sensor to the nearer of the room's walls and the boxes: slab ray casting, float64"""
    nb = sc["num_beams"]
    walls = gc.room_scans(room, poses, sc).astype(np.float64)
    K = walls.shape[0]
    if K * nb == 0:
        return walls.astype(F)
    T = np.asarray(poses, np.float64).reshape(-1, 3, 3) @ sc["sensor_in_robot"].astype(np.float64)
    th = np.arctan2(T[:, 1, 0], T[:, 0, 0])[:, None] + (sc["angle_min"] + np.arange(nb) * sc["angle_increment"])[None, :]
    dx, dy = np.cos(th), np.sin(th)
    ox, oy = T[:, 0, 2, None], T[:, 1, 2, None]
    r = walls
    for bx0, bx1, by0, by1 in boxes:
        with np.errstate(divide="ignore", invalid="ignore"):
            tx0, tx1 = (bx0 - ox) / dx, (bx1 - ox) / dx
            ty0, ty1 = (by0 - oy) / dy, (by1 - oy) / dy
        near = np.maximum(np.minimum(tx0, tx1), np.minimum(ty0, ty1))
        far = np.minimum(np.maximum(tx0, tx1), np.maximum(ty0, ty1))
        hit = np.isfinite(near) & (near <= far) & (near > 0)
        r = np.where(hit, np.minimum(r, near), r)
    if sigma > 0:
        r = r + np.random.default_rng(seed).normal(0.0, sigma, r.shape)
    return r.astype(F)


@functools.lru_cache(maxsize=None)
def recovery_map():
    """the setting of the recovery trials: 160 x 200 cells of 0.05 m at (-1.0, 0.5), drawn from 12 poses of trajectory(room, 12, 3)
    with 361 beams over 270 degrees and 4 mm range noise; the field of radius 4 with the default table.  Everything read-only."""
    g = gr.grid(160, 200, 0.05, (-1.0, 0.5))
    a0, inc = gc.fan(361)
    sc = gr.scanner(a0, inc, 361, range_min=0.05, range_max=20.0)
    room = gc.room_of(g)
    boxes = boxes_of(room)
    poses = gc.trajectory(room, 12, 3)
    ranges = box_scans(room, boxes, poses, sc, sigma=0.004, seed=4)
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    field = sm.likelihood(h, w, 1, 50, 4, sm.default_lut(4))
    for a in (poses, ranges, h, w, field):
        a.setflags(write=False)
    return {"g": g, "sc": sc, "room": room, "boxes": boxes, "poses": poses, "ranges": ranges, "hits": h, "misses": w, "field": field}


def recovery_trial(seed, max_offset=0.6, max_degrees=10.0):
    """(true pose, its scan (1, 361), the guess): the true pose inside the room, the guess up to max_offset per axis and
    max_degrees off, seeded"""
    m = recovery_map()
    rng = np.random.default_rng(1000 + seed)
    x0, x1, y0, y1 = m["room"]
    x = rng.uniform(x0 + 0.35 * (x1 - x0), x1 - 0.35 * (x1 - x0))
    y = rng.uniform(y0 + 0.35 * (y1 - y0), y1 - 0.35 * (y1 - y0))
    th = rng.uniform(-math.pi, math.pi)
    off = rng.uniform(-1.0, 1.0, 3) * np.array([max_offset, max_offset, math.radians(max_degrees)])
    truth = gc.pose(x, y, th)
    scan = box_scans(m["room"], m["boxes"], truth[None], m["sc"], sigma=0.004, seed=2000 + seed)
    return truth, scan, gc.pose(x + off[0], y + off[1], th + off[2])


def pose_error(P, truth):
    """(|x error|, |y error|, |heading error| in radians)"""
    P, truth = np.asarray(P, np.float64), np.asarray(truth, np.float64)
    d = math.atan2(P[1, 0], P[0, 0]) - math.atan2(truth[1, 0], truth[0, 0])
    d = (d + math.pi) % (2 * math.pi) - math.pi
    return abs(P[0, 2] - truth[0, 2]), abs(P[1, 2] - truth[1, 2]), abs(d)
