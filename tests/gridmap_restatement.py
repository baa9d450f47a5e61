"""Independent numpy restatement of the occupancy grid (DESIGN.md section 4 "Occupancy grid").

A beam's end point in float32 in the documented operation order (the bearing and its sine / cosine in float64: the ``sincos`` of
tests/adaptor_restatement.py, the scan adaptor's; the pose composed with the sensor's mount entry by entry in float64, rounded
once), the cell by a float32 divide and floor, and from there integers alone: the closed form of the ray's cells, the two count
planes, the rendered image and the exported scene.  The library must give the same bits.  Every function works on whole arrays;
nothing here knows the library.
"""
import numpy as np

from adaptor_restatement import sincos

F = np.float32
MAX_SIDE, MAX_RAY, MAX_STEPS, CELL_GUARD = 32768, 32767, 32000.0, 2.0 ** 30
UNKNOWN = 255


def grid(rows, cols, resolution=0.05, origin=(0.0, 0.0)):
    return {"rows": int(rows), "cols": int(cols), "res": F(resolution), "ox": F(origin[0]), "oy": F(origin[1])}


def scanner(angle_min, angle_increment, num_beams, range_min=0.05, range_max=30.0, sensor_in_robot=None, clear_beyond_max=True):
    S = np.eye(3, dtype=F) if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(3, 3)
    return {"angle_min": float(angle_min), "angle_increment": float(angle_increment), "num_beams": int(num_beams),
            "range_min": F(range_min), "range_max": F(range_max), "sensor_in_robot": S, "clear_beyond_max": bool(clear_beyond_max)}


def new_planes(g):
    return np.zeros((g["rows"], g["cols"]), np.int32), np.zeros((g["rows"], g["cols"]), np.int32)


def refuses(g, sc):
    """what set-up refuses of a grid and a scanner together: the step cap, in float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return not (F(sc["range_max"]) / g["res"] <= F(MAX_STEPS))


def compose(poses, S):
    """dm::se2_compose(pose, S) for K poses: every entry a float64 sum of products rounded once to float32 -> (K, 2, 3)"""
    a = np.asarray(poses, F).reshape(-1, 3, 3).astype(np.float64)
    b = np.asarray(S, F).reshape(3, 3).astype(np.float64)
    T = np.zeros((a.shape[0], 2, 3), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(2):
            for j in range(2):
                T[:, i, j] = (a[:, i, 0] * b[0, j] + a[:, i, 1] * b[1, j]).astype(F)
            T[:, i, 2] = ((a[:, i, 0] * b[0, 2] + a[:, i, 1] * b[1, 2]) + a[:, i, 2]).astype(F)
    return T


def classify(ranges, sc):
    """(is a return, is cleared only): the rest is skipped"""
    r = np.asarray(ranges, F)
    with np.errstate(invalid="ignore"):
        ret = np.isfinite(r) & (sc["range_min"] <= r) & (r <= sc["range_max"])
        clr = ~ret & (r > sc["range_max"]) & sc["clear_beyond_max"]
    return ret, clr


def _cell(x, o, res):
    """(cell as int64, representable): u = floor((x - o) / res) in float32, never converted outside [-2^30, 2^30)"""
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.floor((x - o) / res)
        ok = (u >= F(-CELL_GUARD)) & (u < F(CELL_GUARD))
    return np.where(ok, u, 0).astype(np.int64), ok


def beams(ranges, poses, sc, g):
    """per beam of the (K, num_beams) batch: is a return, is traced at all, start cell, end cell, n"""
    nb = sc["num_beams"]
    r = np.asarray(ranges, F).reshape(-1, nb)
    K = r.shape[0]
    ret, clr = classify(r, sc)
    T = compose(poses, sc["sensor_in_robot"])
    assert T.shape[0] == K
    bearing = np.float64(sc["angle_min"]) + np.arange(nb, dtype=np.float64) * np.float64(sc["angle_increment"])
    s, c = sincos(bearing)
    cf, sf = c.astype(F)[None, :], s.astype(F)[None, :]
    reach = np.where(ret, r, sc["range_max"]).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        bx, by = cf * reach, sf * reach
        ex = (T[:, 0, 0, None] * bx + T[:, 0, 1, None] * by) + T[:, 0, 2, None]
        ey = (T[:, 1, 0, None] * bx + T[:, 1, 1, None] * by) + T[:, 1, 2, None]
    x0, okx0 = _cell(np.broadcast_to(T[:, 0, 2, None], ex.shape), g["ox"], g["res"])
    y0, oky0 = _cell(np.broadcast_to(T[:, 1, 2, None], ey.shape), g["oy"], g["res"])
    x1, okx1 = _cell(ex, g["ox"], g["res"])
    y1, oky1 = _cell(ey, g["oy"], g["res"])
    n = np.maximum(np.abs(x1 - x0), np.abs(y1 - y0))
    traced = (ret | clr) & okx0 & oky0 & okx1 & oky1 & (n <= MAX_RAY)
    return {"ret": ret, "clr": clr, "traced": traced, "x0": x0, "y0": y0, "x1": x1, "y1": y1, "n": n}


def step_cells(x0, y0, x1, y1, i):
    """the cell of step i (0 <= i <= n) of the rays (x0, y0) -> (x1, y1): the closed form, integer division"""
    dx, dy = x1 - x0, y1 - y0
    ax, ay = np.abs(dx), np.abs(dy)
    n = np.maximum(ax, ay)
    d = np.maximum(2 * n, 1)  # (n = 0: the only step is 0, its offset 0)
    assert np.all(2 * i * np.maximum(ax, ay) + n < 2 ** 31)  # the 32-bit promise of the contract
    return x0 + np.sign(dx) * ((2 * i * ax + n) // d), y0 + np.sign(dy) * ((2 * i * ay + n) // d)


def integrate(hits, misses, ranges, poses, sc, g, weight=1):
    """adds the batch to the planes in place; returns the counters of srrg2_gridmap_result"""
    assert weight in (1, -1)
    nb = sc["num_beams"]
    K = int(np.asarray(poses, F).size // 9)
    out = {"num_beams_total": K * nb, "num_returns": 0, "num_cleared_only": 0, "num_skipped": 0, "num_hits_in_grid": 0,
           "num_miss_updates": 0}
    if K * nb == 0:
        return out
    b = beams(ranges, poses, sc, g)
    out["num_returns"], out["num_cleared_only"] = int(b["ret"].sum()), int(b["clr"].sum())
    out["num_skipped"] = K * nb - out["num_returns"] - out["num_cleared_only"]
    t = b["traced"].reshape(-1)
    x0, y0, x1, y1, n, ret = (b[k].reshape(-1)[t] for k in ("x0", "y0", "x1", "y1", "n", "ret"))
    rows, cols = g["rows"], g["cols"]
    hflat, mflat = hits.reshape(-1), misses.reshape(-1)
    for i in range(int(n.max()) + 1 if n.size else 0):
        live = n >= i
        cx, cy = step_cells(x0[live], y0[live], x1[live], y1[live], i)
        inside = (cx >= 0) & (cx < cols) & (cy >= 0) & (cy < rows)
        last = n[live] == i
        miss = inside & ~last
        hit = inside & last & ret[live]
        np.add.at(mflat, (cy * cols + cx)[miss], np.int32(weight))
        np.add.at(hflat, (cy * cols + cx)[hit], np.int32(weight))
        out["num_miss_updates"] += int(miss.sum())
        out["num_hits_in_grid"] += int(hit.sum())
    return out


def render(hits, misses, min_observations=1):
    """(rows, cols) uint8: (100 hits + n / 2) / n with n = hits + misses, 255 where n < max(min_observations, 1) or a count < 0"""
    h, m = hits.astype(np.int64), misses.astype(np.int64)
    n = h + m
    known = (h >= 0) & (m >= 0) & (n >= max(int(min_observations), 1))
    v = (100 * h + n // 2) // np.maximum(n, 1)
    return np.where(known, v, UNKNOWN).astype(np.uint8)


def to_scene(hits, misses, g, min_observations=1, occupied_percent=50):
    """(points (k, 2) float32, plane indices (k,) int32) of the cells that render into [occupied_percent, 100]"""
    v = render(hits, misses, min_observations).reshape(-1).astype(np.int64)
    idx = np.flatnonzero((v >= occupied_percent) & (v <= 100)).astype(np.int32)
    iy, ix = idx // max(g["cols"], 1), idx % max(g["cols"], 1)
    x = g["ox"] + (ix.astype(F) + F(0.5)) * g["res"]
    y = g["oy"] + (iy.astype(F) + F(0.5)) * g["res"]
    return np.stack([x, y], -1).astype(F).reshape(-1, 2), idx
