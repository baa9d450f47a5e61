"""Synthetic sweeps of a MOVING spinning lidar with per-ring elevation tables, in the room of ``lidar_cases``.  Every beam is cast
from the sensor's pose at its own firing time -- constant rotation rate about a fixed axis, translation linear in the normalised
time s -- in float64 and with NO range noise, so that a correct de-skew puts every point back on a surface up to float32
rounding.  Beams fire column by column; ``times`` is the firing fraction (column ordinal + azimuth jitter + 0.5) / cols, which
runs past 1 on the columns fired again behind the seam.  Pure numpy (np.sin / np.cos / arccos); nothing here knows the library
or the restatement's arithmetic."""
import functools

import numpy as np

import lidar_cases as lc
from lidar_restatement import Model

F = np.float32
DEG = np.pi / 180.0


# ---- ring tables ------------------------------------------------------------------------------------------------------------
def uniform_table(rows=16, first_deg=-15.0, last_deg=15.0):
    """exactly the elevations of Model.full_turn's rows"""
    m = Model.full_turn(rows, 8, first_deg * DEG, last_deg * DEG)
    return m.elevation_min + np.arange(rows, dtype=np.float64) * m.elevation_increment


def two_block_table(descending=False):
    """16 rings in two blocks of 8, the lower block 1.5 times as widely spaced as the upper one (an HDL-64 in small)"""
    lower = -15.0 + 2.4 * np.arange(8)
    upper = lower[-1] + 2.0 + 1.6 * np.arange(8)
    e = np.concatenate([lower, upper]) * DEG
    return e[::-1].copy() if descending else e


def hdl64_table():
    """64 rings: 32 at 1/3 degree from +2 downwards, 32 at 1/2 degree below them (descending, as the sensor numbers its lasers)"""
    upper = 2.0 - np.arange(32) / 3.0
    lower = upper[-1] - 0.5 * (1 + np.arange(32))
    return np.concatenate([upper, lower]) * DEG


def blocks_table(rows, descending=False, first_deg=-24.0):
    """`rows` rings in two halves, spacing 0.9 and 0.6 degrees"""
    h = rows // 2
    lower = first_deg + 0.9 * np.arange(h)
    upper = lower[-1] + 0.75 + 0.6 * np.arange(rows - h)
    e = np.concatenate([lower, upper]) * DEG
    return e[::-1].copy() if descending else e


SYMMETRIC4 = np.array([-0.3, -0.1, 0.1, 0.3])


# ---- motion -----------------------------------------------------------------------------------------------------------------
def motion(dx=0.35, dy=0.2, dz=0.06, yaw_deg=10.0, pitch_deg=1.0):
    """the sensor at the sweep's end in its frame at the sweep's start: about 0.41 m and 10 degrees; 3x4 float32"""
    return lc.pose(dx, dy, dz, yaw_deg=yaw_deg, pitch_deg=pitch_deg)


def axis_angle(motion_3x4):
    """plain numpy: rotation angle, unit axis and translation of a 3x4 float32 [R|t] (float64).  A float32 matrix is a rotation
    only up to 6e-8, so WHICH angle and axis it stands for is a matter of definition at that level -- metres times 6e-8 is a
    float32 ulp of a lidar point: the definition is the contract's, through the unit quaternion (its trace form, which holds
    for angles below 120 degrees), theta = 2 atan2(|v|, w), axis = v / |v|"""
    M = np.asarray(motion_3x4, F).astype(np.float64).reshape(3, 4)
    R = M[:, :3]
    assert np.trace(R) > 0.0
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    n = np.sqrt(w * w + v @ v)
    w, v = w / n, v / n
    if not v.any():
        return 0.0, np.array([0.0, 0.0, 1.0]), M[:, 3]
    return 2.0 * np.arctan2(np.linalg.norm(v), w), v / np.linalg.norm(v), M[:, 3]


def rotation(axis, angle):
    """matrix Rodrigues, angle scalar or (k,) -> (3, 3) or (k, 3, 3)"""
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    angle = np.asarray(angle, np.float64)
    s, c = np.sin(angle)[..., None, None], np.cos(angle)[..., None, None]
    return np.eye(3) + s * K + (1.0 - c) * (K @ K)


def pose_at(start_in_room, motion_3x4, s):
    """the sensor in the room at normalised time s (scalar) -> 3x4 float64"""
    theta, a, t = axis_angle(motion_3x4)
    T0 = np.asarray(start_in_room, np.float64)
    return np.concatenate([T0[:, :3] @ rotation(a, s * theta), (T0[:, :3] @ (s * t) + T0[:, 3])[:, None]], axis=1)


def deskew_float64(points, s, motion_3x4, reference):
    """the de-skew in plain float64 numpy (np.sin, np.cos, matrix Rodrigues), rounded to float32 once"""
    theta, a, t = axis_angle(motion_3x4)
    P = np.asarray(points, F).astype(np.float64)
    s = np.asarray(s, np.float64)
    q = np.einsum("kij,kj->ki", rotation(a, s * theta), P) + s[:, None] * t
    return ((q - reference * t) @ rotation(a, reference * theta)).astype(F)  # (R^T v)^T = v^T R


def moving_sweep(rows, cols, start_in_room, motion_3x4, seed, ring_elevations=None, overlap_cols=None, dropped=0.02,
                 elevation_deg=(-15.0, 15.0), jitter=0.45):
    """-> dict(points (n, 3) float32 RAW sensor-frame points in firing order, intensity, times (n,) float32, s (n,) float64 (the
    float32 times widened: what the library is told), model, start_in_room, motion, ring_elevations)"""
    rng = np.random.default_rng(seed)
    if ring_elevations is None:
        m = Model.full_turn(rows, cols, elevation_deg[0] * DEG, elevation_deg[1] * DEG)
        e = m.elevation_min + np.arange(rows) * m.elevation_increment
    else:
        e = np.asarray(ring_elevations, np.float64)
        m = Model.full_turn(rows, cols, e[0], e[-1])
    gap = np.abs(np.diff(e))
    room_for = np.minimum(np.concatenate([gap[:1], gap]), np.concatenate([gap, gap[-1:]]))  # per ring: the nearer neighbour
    overlap_cols = max(1, cols // 20) if overlap_cols is None else overlap_cols
    ordinal = np.arange(cols + overlap_cols)
    oo, rr = np.meshgrid(ordinal, np.arange(rows), indexing="ij")  # column by column, as the sensor fires
    oo, rr = oo.reshape(-1), rr.reshape(-1)
    k = oo.shape[0]
    ja = rng.uniform(-jitter, jitter, k)
    az = m.azimuth_min + ((oo % cols) + ja) * m.azimuth_increment
    el = e[rr] + rng.uniform(-jitter, jitter, k) * room_for[rr]
    times = ((oo + ja + 0.5) / cols).astype(F)
    s = times.astype(np.float64)
    d_s = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    theta, a, t = axis_angle(motion_3x4)
    T0 = np.asarray(start_in_room, np.float64)
    Rs = T0[:, :3] @ rotation(a, s * theta)  # (k, 3, 3)
    origin = (s[:, None] * t) @ T0[:, :3].T + T0[:, 3]
    d_w = np.einsum("kij,kj->ki", Rs, d_s)
    rng_m = _cast_each(origin, d_w)
    keep = rng.uniform(size=k) >= dropped
    pts = (d_s * rng_m[:, None])[keep].astype(F)
    inten = (0.2 + 0.6 * rng.uniform(size=k))[keep].astype(F)
    return {"points": pts, "intensity": inten, "times": times[keep], "s": s[keep], "model": m,
            "start_in_room": np.asarray(start_in_room, F), "motion": np.asarray(motion_3x4, F),
            "ring_elevations": None if ring_elevations is None else e}


def _cast_each(origins, dirs):
    """lidar_cases._cast with one origin per beam: ranges to the nearest of walls / floor / ceiling / pillar"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.full(dirs.shape[0], np.inf)
        for a in range(3):
            far = np.where(dirs[:, a] > 0, lc.ROOM[a], 0.0)
            ta = np.where(dirs[:, a] != 0, (far - origins[:, a]) / dirs[:, a], np.inf)
            t = np.minimum(t, np.where(ta > 0, ta, np.inf))
        lo, hi = np.full(dirs.shape[0], -np.inf), np.full(dirs.shape[0], np.inf)
        for a, (p0, p1) in enumerate(((lc.PILLAR[0], lc.PILLAR[1]), (lc.PILLAR[2], lc.PILLAR[3]))):
            t0, t1 = (p0 - origins[:, a]) / dirs[:, a], (p1 - origins[:, a]) / dirs[:, a]
            lo, hi = np.maximum(lo, np.minimum(t0, t1)), np.minimum(hi, np.maximum(t0, t1))
        hit = (lo <= hi) & (lo > 0) & (lo < t)
    return np.where(hit, lo, t)


def surface_distance(points_in_room):
    """per point the distance to the nearest surface of the room: six planes and the four faces of the pillar"""
    P = np.asarray(points_in_room, np.float64)
    d = np.full(P.shape[0], np.inf)
    for a in range(3):
        d = np.minimum(d, np.minimum(np.abs(P[:, a]), np.abs(P[:, a] - lc.ROOM[a])))
    x0, x1, y0, y1 = lc.PILLAR
    off_y = np.maximum(np.maximum(y0 - P[:, 1], P[:, 1] - y1), 0.0)
    off_x = np.maximum(np.maximum(x0 - P[:, 0], P[:, 0] - x1), 0.0)
    for x in (x0, x1):
        d = np.minimum(d, np.hypot(P[:, 0] - x, off_y))
    for y in (y0, y1):
        d = np.minimum(d, np.hypot(P[:, 1] - y, off_x))
    return d


def to_room(points, sensor_in_room):
    """float64, not rounded: the geometry checks measure micrometres"""
    T = np.asarray(sensor_in_room, np.float64)
    return np.asarray(points, np.float64) @ T[:, :3].T + T[:, 3]


START = lc.pose(3.2, 2.9, 1.1, yaw_deg=20.0, pitch_deg=1.5)


@functools.lru_cache(maxsize=None)
def moving_case(table="uniform", overlap=True):
    """16 x 360 from inside the room while the sensor moves 0.41 m and 10 degrees; `table`: uniform (None is passed on: the
    model's rows), two_block, two_block_desc"""
    e = {"uniform": None, "two_block": two_block_table(), "two_block_desc": two_block_table(True)}[table]
    return moving_sweep(16, 360, START, motion(), seed=21, ring_elevations=e, overlap_cols=None if overlap else 0)


@functools.lru_cache(maxsize=None)
def static_ring_case(table):
    """16 x 360, sensor at rest, rings from a table (two_block, two_block_desc, uniform_table)"""
    e = {"two_block": two_block_table(), "two_block_desc": two_block_table(True), "uniform_table": uniform_table()}[table]
    return moving_sweep(16, 360, START, np.eye(3, 4, dtype=F), seed=22, ring_elevations=e)


@functools.lru_cache(maxsize=None)
def large_case():
    """66 x 2048 with a 66-entry two-block table, moving: more than 512 x 256 points and pixels"""
    return moving_sweep(66, 2048, START, motion(), seed=23, ring_elevations=blocks_table(66), overlap_cols=80, dropped=0.0)


def boundary_points(descending=False):
    """points for the 4-row symmetric tables (+-0.1, +-0.3 rad: boundaries at -0.4, -0.2, 0, 0.2, 0.4): z = 0 lies exactly on
    b[2] = 0; the others sit inside rows and just inside / outside b[0] and b[rows]
    -> (table, points (n, 3) float32, the row every point must get (-1 = out of view))"""
    e = SYMMETRIC4[::-1].copy() if descending else SYMMETRIC4.copy()
    els = [0.0, -0.0, 0.05, -0.05, 0.25, -0.25, 0.399, -0.399, 0.401, -0.401, 0.2 + 1e-6, -0.2 - 1e-6]
    asc_rows = [2, 2, 2, 1, 3, 0, 3, 0, -1, -1, 3, 0]
    pts = [[2.0 * np.cos(el), 0.0, 2.0 * np.sin(el)] if el != 0 else [2.0, 0.0, el] for el in els]
    rows = list(asc_rows)
    if descending:  # row k of the reversed table is row 3 - k of the ascending one, but a boundary point goes to the higher INDEX
        rows = [-1 if r < 0 else 3 - r for r in asc_rows]
        rows[0] = rows[1] = 2
    return e, np.asarray(pts, F), np.asarray(rows)
