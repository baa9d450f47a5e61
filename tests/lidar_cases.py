"""Synthetic 3-D lidar sweeps for the lidar tests: a box room with a square pillar, ray-cast from a sensor pose.  Every beam is
fired at its pixel's centre plus an angular jitter below half a pixel (so it lands in its own pixel), about 2 % of the beams
give no return, and the sweep runs a little over one turn -- the first columns are fired twice, as a spinning sensor's packets
overlap at the seam -- so that some pixels get more than one candidate.  Pure numpy; nothing here knows the library."""
import functools

import numpy as np

from lidar_restatement import Model

F = np.float32
ROOM = (10.0, 8.0, 3.0)  # interior of the box [0, x] x [0, y] x [0, z]
PILLAR = (5.6, 6.4, 3.4, 4.2)  # x0, x1, y0, y1; floor to ceiling
DEG = np.pi / 180.0


def pose(x, y, z, yaw_deg=0.0, pitch_deg=0.0):
    """sensor (or robot) in the room: 3x4 float32 [R|t], R = Rz(yaw) Ry(pitch)"""
    cy, sy, cp, sp = np.cos(yaw_deg * DEG), np.sin(yaw_deg * DEG), np.cos(pitch_deg * DEG), np.sin(pitch_deg * DEG)
    R = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    return np.concatenate([R, np.array([[x], [y], [z]])], axis=1).astype(F)


def _cast(origin, dirs):
    """range along unit directions `dirs` (k, 3) from `origin` inside the room to the nearest of walls / floor / ceiling / pillar"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.full(dirs.shape[0], np.inf)
        for a in range(3):  # leaving the box: the first of the three far planes
            far = np.where(dirs[:, a] > 0, ROOM[a], 0.0)
            ta = np.where(dirs[:, a] != 0, (far - origin[a]) / dirs[:, a], np.inf)
            t = np.minimum(t, np.where(ta > 0, ta, np.inf))
        lo, hi = np.full(dirs.shape[0], -np.inf), np.full(dirs.shape[0], np.inf)
        for a, (p0, p1) in enumerate(((PILLAR[0], PILLAR[1]), (PILLAR[2], PILLAR[3]))):  # the pillar: slabs in x and y
            t0, t1 = (p0 - origin[a]) / dirs[:, a], (p1 - origin[a]) / dirs[:, a]
            lo, hi = np.maximum(lo, np.minimum(t0, t1)), np.minimum(hi, np.maximum(t0, t1))
        hit = (lo <= hi) & (lo > 0) & (lo < t)
    return np.where(hit, lo, t)


def room_sweep(rows, cols, sensor_in_room, seed, overlap_cols=None, dropped=0.02, elevation_deg=(-15.0, 15.0), jitter=0.45,
               clockwise=False, top_first=False):
    """-> dict(points (n, 3) float32 in the SENSOR frame, in firing order; intensity (n,); model; sensor_in_room; elevation:
    the first and the last row's, as the full-turn helper takes them)"""
    rng = np.random.default_rng(seed)
    e0, e1 = (elevation_deg[1], elevation_deg[0]) if top_first else elevation_deg
    m = Model.full_turn(rows, cols, e0 * DEG, e1 * DEG)
    if clockwise:
        m = Model(-m.azimuth_min, -m.azimuth_increment, m.elevation_min, m.elevation_increment, rows, cols)
    overlap_cols = max(1, cols // 20) if overlap_cols is None else overlap_cols
    c = np.arange(cols + overlap_cols) % cols  # a little more than one turn
    cc, rr = np.meshgrid(c, np.arange(rows), indexing="ij")  # column by column, as the sensor fires
    cc, rr = cc.reshape(-1), rr.reshape(-1)
    k = cc.shape[0]
    az = m.azimuth_min + (cc + rng.uniform(-jitter, jitter, k)) * m.azimuth_increment
    el = m.elevation_min + (rr + rng.uniform(-jitter, jitter, k)) * m.elevation_increment
    d_s = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    T = np.asarray(sensor_in_room, np.float64)
    rng_m = _cast(T[:, 3], d_s @ T[:, :3].T) + rng.normal(0.0, 0.002, k)
    keep = rng.uniform(size=k) >= dropped
    pts = (d_s * rng_m[:, None])[keep].astype(F)
    inten = (0.2 + 0.6 * rng.uniform(size=k))[keep].astype(F)
    return {"points": pts, "intensity": inten, "model": m, "sensor_in_room": np.asarray(sensor_in_room, F),
            "elevation": (e0 * DEG, e1 * DEG)}


def to_room(points, sensor_in_room):
    T = np.asarray(sensor_in_room, np.float64)
    return (np.asarray(points, np.float64) @ T[:, :3].T + T[:, 3]).astype(F)


def direction(az, el, rho=1.0):
    return [rho * np.cos(el) * np.cos(az), rho * np.cos(el) * np.sin(az), rho * np.sin(el)]


def full_image(m, rho=3.0):
    """one point at the centre of every pixel, row-major"""
    return np.asarray([direction(m.azimuth_min + c * m.azimuth_increment, m.elevation_min + r * m.elevation_increment, rho)
                       for r in range(m.rows) for c in range(m.cols)], F)


def collinear_sweep(nudge=0.0):
    """a 3 x 4 image whose centre pixel (1, 1) looks along +x: its left / right neighbours differ in y alone and so do its
    upper / lower ones, so both central differences are multiples of (0, 1, 0) and their cross product is exactly zero
    (`nudge` lifts the right neighbour's z: the normal exists again) -> (model, points, the centre's pixel index)"""
    m = Model(-np.pi / 2, np.pi / 2, 0.639, 0.073, 3, 4)  # row centres 0.639, 0.712, 0.785 rad
    z = np.sqrt(5.0) * np.tan(0.712)
    pts = [[2 * np.cos(0.712), 0, 2 * np.sin(0.712)],  # centre
           [1, -2, z], [1, 2, z + nudge],  # left, right: azimuth -+63 degrees, elevation 0.712
           [1, 0.9, 1], [1, 0, 1]]  # up (row 0, elevation 0.639), down (row 2, 0.785)
    return m, np.asarray(pts, F), 1 * 4 + 1


def edge_cases():
    """hand-made inputs on 2 x 4 to 4 x 8 images -> list of (name, model, points (n, 3) float32, adaptor keywords)"""
    PI = np.pi
    m = Model.full_turn(4, 8, -0.3, 0.3)
    a, b = direction(0.1, 0.05, 3.0), direction(0.12, 0.04, 2.0)
    img = full_image(m)
    wide = dict(max_distance_squared=100.0)
    axes = Model(-PI / 4, PI / 2, -PI / 4, PI / 2, 2, 4, range_min=1.0, range_max=2.0)  # pixel boundaries on the x axis
    gates = Model(0.0, 0.25, 0.0, 0.25, 4, 8, range_min=1.0, range_max=2.0)
    below, above = np.nextafter(F(1), F(0)), np.nextafter(F(2), F(3))
    sector = Model(PI - 0.3, 0.2, -0.3, 0.2, 4, 4)  # four columns across +-pi
    clockwise = Model(-m.azimuth_min, -m.azimuth_increment, 0.3, -0.2, 4, 8)
    pole = Model(0.0, PI / 2, -PI / 2, PI / 3, 4, 4)
    no_wrap = Model(m.azimuth_min, m.azimuth_increment, m.elevation_min, m.elevation_increment, 4, 7)
    cases = [
        ("tie goes to the lower index", m, [a, a, b, b], {}),
        ("nearer wins, far first", m, [a, b, a], {}),
        ("nearer wins, near first", m, [b, a, a], {}),
        ("pixel boundaries", axes, [[1, 0, 0], [1, -1e-6, 0], [1, 0, -1e-6], [1, -1e-6, -1e-6], [1.5, 0, 0]], {}),
        ("range gates", gates, [[1, 0, 0], [2, 0, 0], [below, 0, 0], [above, 0, 0]], {}),
        ("outside the image", gates, [direction(0.0, -0.2, 1.5), direction(1.9, 0.1, 1.5), direction(1.85, 0.1, 1.5)], {}),
        ("seam, wrapping", m, np.concatenate([img, [direction(PI - 0.01, 0.0, 2.0), direction(-PI + 0.01, 0.0, 2.0),
                                                    [-2, 1e-6, 0], [-2, -1e-6, 0], [-2, 0, 0]]]), wide),
        ("seam, sector across pi", sector, [direction(PI - 0.3 + 0.2 * c + j, -0.3 + 0.2 * r, 2.0 + 0.1 * c)
                                            for r in range(4) for c in range(-1, 5) for j in (-0.05, 0.05)], wide),
        ("clockwise, rows from the top", clockwise, img, wide),
        ("no wrap: border columns get no normal", no_wrap, img, wide),
        ("z axis", pole, [[0, 0, 2], [0, 0, -2], [0, 0, 1], [1e-3, 0, 2]], {}),
        ("gaps larger than the image", m, img, dict(col_gap=1, row_gap=2, **wide)),
        ("column gap beyond one turn", m, img, dict(col_gap=9, row_gap=1, **wide)),
        ("column gap of one turn", m, img, dict(col_gap=8, row_gap=1, **wide)),
        ("gate closes", m, img, dict(max_distance_squared=0.5)),
        ("gate on one difference", m, img * np.where(np.arange(32) % 8 == 3, F(1.4), F(1.0)).astype(F)[:, None],
         dict(max_distance_squared=20.0)),
        ("one missing neighbour", m, np.delete(img, 1 * 8 + 3, axis=0), wide),
        ("collinear neighbours", collinear_sweep()[0], collinear_sweep()[1], wide),
        ("nearly collinear neighbours", collinear_sweep()[0], collinear_sweep(0.05)[1], wide),
        ("NaN and inf", m, np.concatenate([img[:12], [[np.nan, 0, 0], [1, np.inf, 0], [1, 1, -np.inf], [np.nan] * 3], img[12:]]),
         wide),
        ("every point out of view", m, [[0.1, 0, 0], [200, 0, 0], [0, 0, 3], [1, 0, 2], [np.nan, 1, 1]], {}),
    ]
    return [(name, mod, np.asarray(pts, F).reshape(-1, 3), kw) for name, mod, pts, kw in cases]


def next_door(sensor_in_room, k, seed):
    """k points (and their normals) on the wall of the room next door, 0.6 m behind the x = 10 wall, in the SENSOR frame: a
    map holds them, the sensor cannot see them"""
    rng = np.random.default_rng(seed)
    w = np.stack([np.full(k, ROOM[0] + 0.6), rng.uniform(0.0, ROOM[1], k), rng.uniform(0.0, ROOM[2], k)], axis=1)
    T = np.asarray(sensor_in_room, np.float64)
    return ((w - T[:, 3]) @ T[:, :3]).astype(F), np.tile(-T[0, :3], (k, 1)).astype(F)


@functools.lru_cache(maxsize=None)
def main_case():
    """16 rows x 360 columns from inside the room, about 5.5 k points"""
    return room_sweep(16, 360, pose(3.2, 2.9, 1.1, yaw_deg=20.0, pitch_deg=1.5), seed=11)


@functools.lru_cache(maxsize=None)
def second_sweep():
    """the same sensor 5 cm and 1 degree further on"""
    return room_sweep(16, 360, pose(3.24, 2.93, 1.1, yaw_deg=21.0, pitch_deg=1.5), seed=12)


@functools.lru_cache(maxsize=None)
def occlusion_case():
    """a map of the room in room coordinates -- two sweeps from either side of the pillar and the wall of the room next door,
    0.6 m behind the x = 10 wall -- seen from the main case's pose: what lies behind the pillar and behind the wall is hidden.
    -> dict(points, normals, intensity, robot_in_local_map, sensor_in_robot, model, margin)"""
    a = main_case()
    b = room_sweep(16, 360, pose(8.4, 5.6, 1.3, yaw_deg=-140.0), seed=13)
    rng = np.random.default_rng(14)
    pts = np.concatenate([to_room(a["points"], a["sensor_in_room"]), to_room(b["points"], b["sensor_in_room"]),
                          to_room(next_door(a["sensor_in_room"], 1500, 15)[0], a["sensor_in_room"])])
    order = rng.permutation(pts.shape[0])  # a map has no firing order
    pts = pts[order]
    nrm = rng.normal(size=pts.shape)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    # the robot carries the sensor 0.3 m ahead and 0.4 m up, turned by 20 degrees
    sensor_in_robot = pose(0.3, 0.0, 0.4, yaw_deg=20.0)
    S, A = np.eye(4), np.eye(4)
    S[:3], A[:3] = sensor_in_robot, a["sensor_in_room"]
    robot_in_local_map = (A @ np.linalg.inv(S))[:3].astype(F)
    return {"points": pts, "normals": nrm, "intensity": rng.uniform(size=pts.shape[0]).astype(F),
            "robot_in_local_map": robot_in_local_map, "sensor_in_robot": sensor_in_robot, "model": a["model"], "margin": 0.1}


GATE = 0.3  # the finder's gate of the through-the-stack alignment: 5 cm and 1 degree move no point of the room further


@functools.lru_cache(maxsize=None)
def stack_case():
    """two sweeps 5 cm and 1 degree apart and what the frame makes of them, all by the restatement: both adapted (compact), a map
    in the first sensor's frame -- the first measurement and the wall next door -- clipped to what the lidar sees from there
    (margin 0.1 m).  -> dict(a, b (sweeps), meas_a, meas_b (restated adapts), map_points, map_normals, clipped (restated clip),
    true_b_from_a (3x4 float64))"""
    import lidar_restatement as lr

    a, b = main_case(), second_sweep()
    meas_a = lr.adapt_lidar_sweep(a["points"], a["model"], compact=True)
    meas_b = lr.adapt_lidar_sweep(b["points"], b["model"], compact=True)
    hidden, hidden_n = next_door(a["sensor_in_room"], 600, 16)
    map_points, map_normals = np.concatenate([meas_a["points"], hidden]), np.concatenate([meas_a["normals"], hidden_n])
    clipped = lr.clip_spherical(map_points, np.eye(3, 4, dtype=F), a["model"], None, 0.1, normals=map_normals)
    A, B = np.eye(4), np.eye(4)
    A[:3], B[:3] = a["sensor_in_room"], b["sensor_in_room"]
    return {"a": a, "b": b, "meas_a": meas_a, "meas_b": meas_b, "map_points": map_points, "map_normals": map_normals,
            "clipped": clipped, "true_b_from_a": (np.linalg.inv(B) @ A)[:3]}


def stack_oracle_run(oracle, fixed_points, fixed_normals, moving_points, moving_normals):
    """the oracle's point-to-plane alignment of the clipped map (moving) against the second measurement (fixed)"""
    from helpers import cue_config
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import synthetic as syn

    al = oracle.OracleAligner(abi.SE3_QUAT_RIGHT)
    si = al.add_slice(cue_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, GATE, robust=abi.ROBUST_CAUCHY))
    al.set_fixed(si, fixed_points, fixed_normals)
    al.set_moving(si, moving_points, moving_normals)
    al.set_moving_in_fixed(syn.identity(3))
    al.compute()
    return al
