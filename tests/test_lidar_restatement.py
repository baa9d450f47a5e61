"""CPU: the numpy restatement of DESIGN.md section 4 "Lidar sweeps" (tests/lidar_restatement.py) on hand-made inputs -- the
properties the contract spells out, checked on the executable contract itself -- and the synthetic sweeps of
tests/lidar_cases.py are not vacuous.  Needs no GPU and nothing of the library."""
import math

import numpy as np

import lidar_cases as lc
import lidar_restatement as lr

F = np.float32
PI = math.pi
I34 = np.eye(3, 4, dtype=F)


_dir = lc.direction


def _model(rows=4, cols=8, el=(-0.3, 0.3), **kw):
    return lr.Model.full_turn(rows, cols, el[0], el[1], **kw)


def _pix(m, pts):
    P = np.asarray(pts, F).reshape(-1, 3)
    return lr.project(P[:, 0], P[:, 1], P[:, 2], m)[0]


def test_full_turn_model_and_validation():
    m = _model(4, 8)
    assert m.valid() and m.columns_wrap()
    assert m.azimuth_increment == 2 * PI / 8 and m.azimuth_min == -PI + PI / 8
    assert m.elevation_min == -0.3 and m.elevation_increment == (0.3 - -0.3) / 3
    assert (m.range_min, m.range_max) == (F(0.5), F(120.0))
    bad = [dict(rows=0), dict(cols=0), dict(rows=70000, cols=70000), dict(azimuth_increment=0.0),
           dict(azimuth_increment=float("inf")), dict(elevation_increment=0.0), dict(elevation_increment=float("nan")),
           dict(azimuth_min=float("nan")), dict(azimuth_min=7.0), dict(azimuth_increment=2 * PI / 6.9),
           dict(elevation_min=float("inf")), dict(elevation_min=-1.7), dict(elevation_increment=0.7), dict(range_min=0.0),
           dict(range_min=float("nan")), dict(range_max=0.4)]
    for kw in bad:
        q = _model(4, 8)
        for k, v in kw.items():
            setattr(q, k, F(v) if k.startswith("range") else (v if k in ("rows", "cols") else np.float64(v)))
        assert not q.valid(), kw
    # 9 columns over 8 increments' turn close on themselves once: legal, and no longer a wrap
    q = lr.Model(m.azimuth_min, m.azimuth_increment, -0.3, 0.2, 4, 9)
    assert q.valid() and not q.columns_wrap()
    # an increment that went through float32 still wraps
    assert lr.Model(m.azimuth_min, F(2 * PI / 360), -0.3, 0.2, 4, 360).columns_wrap()
    # the poles are legal row centres
    assert lr.Model(m.azimuth_min, m.azimuth_increment, -PI / 2, PI / 3, 4, 8).valid()


def test_pixel_boundary_goes_to_the_upper_pixel_and_gates_are_inclusive():
    # boundaries on the x axis, where the restated atan2 is exact: alpha = 0 and eps = 0 give t = (pi/4) / (pi/2) = 0.5 exactly,
    # t + 0.5 = 1.0, and floor takes the UPPER pixel of the two that meet there: column 1, row 1
    q = lr.Model(-PI / 4, PI / 2, -PI / 4, PI / 2, 2, 4, range_min=1.0, range_max=2.0)
    assert q.valid() and q.columns_wrap()
    assert list(_pix(q, [[1, 0, 0], [1, -1e-6, 0], [1, 0, -1e-6], [1, -1e-6, -1e-6]])) == [1 * 4 + 1, 1 * 4 + 0, 0 * 4 + 1, 0]
    # range gates, both inclusive; rho is the float32 square root of the float32 sum
    m = lr.Model(0.0, 0.25, 0.0, 0.25, 4, 8, range_min=1.0, range_max=2.0)
    assert m.valid() and not m.columns_wrap()
    below, above = np.nextafter(F(1), F(0)), np.nextafter(F(2), F(3))
    assert list(_pix(m, [[1, 0, 0], [2, 0, 0], [below, 0, 0], [above, 0, 0]])) == [0, 0, -1, -1]
    # outside the image: below row 0, beyond the last column (no wrap into column 0: the sector is 2 rad wide)
    assert list(_pix(m, [_dir(0.0, -0.2, 1.5), _dir(0.25 * 7.6, 0.1, 1.5), _dir(0.25 * 7.4, 0.1, 1.5)])) == [-1, -1, 0 * 8 + 7]


def test_seam_wrap_clockwise_descending_and_the_z_axis():
    m = _model(4, 8)  # columns tile [-pi, pi): column 0 starts at -pi, column 7 ends at +pi
    pix = _pix(m, [_dir(PI - 0.01, 0.0, 2.0), _dir(-PI + 0.01, 0.0, 2.0), [-2, 1e-6, 0], [-2, -1e-6, 0]])
    assert list(pix % 8) == [7, 0, 7, 0] and len(set(pix // 8)) == 1  # either side of the seam, one row
    # a sector camera across +-pi: 4 columns centred on pi, one increment each side of the seam
    s = lr.Model(PI - 0.3, 0.2, -0.3, 0.2, 4, 4)
    assert s.valid() and not s.columns_wrap()
    assert list(_pix(s, [_dir(PI - 0.3, 0, 2), _dir(PI - 0.1, 0, 2), _dir(-PI + 0.1, 0, 2), _dir(-PI + 0.3, 0, 2)]) % 4) == [0, 1, 2, 3]
    assert list(_pix(s, [_dir(-PI + 0.45, 0, 2), _dir(PI - 0.45, 0, 2)])) == [-1, -1]
    # clockwise azimuth, rows from the top
    cw = lr.Model(-m.azimuth_min, -m.azimuth_increment, 0.3, -0.2, 4, 8)
    assert cw.valid() and cw.columns_wrap()
    pts = [_dir(m.azimuth_min + c * m.azimuth_increment, -0.3 + r * 0.2, 3.0) for r in range(4) for c in range(8)]
    assert list(_pix(m, pts)) == list(range(32))
    assert list(_pix(cw, pts)) == [(3 - r) * 8 + (7 - c) for r in range(4) for c in range(8)]
    # a point on the sensor's z axis: alpha = 0, eps = +-pi/2
    pole = lr.Model(0.0, PI / 2, -PI / 2, PI / 3, 4, 4)
    assert list(_pix(pole, [[0, 0, 2], [0, 0, -2]])) == [3 * 4 + 0, 0 * 4 + 0]
    assert list(_pix(m, [[0, 0, 2]])) == [-1]


def test_nearest_wins_and_ties_go_to_the_lower_index():
    m = _model(4, 8)
    a, b, c = _dir(0.1, 0.05, 3.0), _dir(0.12, 0.04, 2.0), _dir(0.1, 0.05, 3.0)
    assert len(set(_pix(m, [a, b, c]))) == 1
    pix = int(_pix(m, [a])[0])
    for order in ([a, b, c], [b, a, c], [c, a, b]):
        r = lr.adapt_lidar_sweep(order, m, col_gap=0, row_gap=0)
        assert lr.same_bits(r["points"][pix], np.asarray(b, F)) and r["candidates"][pix] == 3 and r["num_in_range"] == 1
    # equal ranges: the lowest input index; the stored point is that input verbatim
    r = lr.adapt_lidar_sweep([a, c], m, col_gap=0, row_gap=0, intensity=[5.0, 6.0], compact=True)
    assert r["intensity"].tolist() == [5.0] and r["global_indices"].tolist() == [pix] and r["normals"] is None
    w, _ = lr.bin_sweep(np.asarray([a, c], F), m)
    assert int(w[pix]) & 0xFFFFFFFF == 0
    # NaN / inf inputs never enter; an empty sweep is an empty scene
    r = lr.adapt_lidar_sweep([[np.nan, 0, 0], [np.inf, 1, 1], a], m)
    assert r["num_raw"] == 3 and r["num_in_range"] == 1 and r["num_valid"] == 0 and r["scene_size"] == 32
    e = lr.adapt_lidar_sweep(np.zeros((0, 3), F), m)
    assert e["status"] == lr.ADAPTOR_INITIALIZING and e["scene_size"] == 0


def test_normals_wrap_gates_and_degenerate_neighbours():
    m = _model(4, 8)
    P = lc.full_image(m)
    r = lr.adapt_lidar_sweep(P, m, max_distance_squared=100.0)
    hn = r["has_normal"].reshape(4, 8)
    assert hn[1:3].all() and not hn[0].any() and not hn[3].any()  # wrap: every column of the inner rows
    q = P.reshape(4, 8, 3)[1:3]
    nn = r["normals"].reshape(4, 8, 3)[1:3]
    assert ((nn * q).sum(-1) < 0).all() and np.allclose(np.linalg.norm(nn, axis=-1), 1.0, atol=1e-6)  # facing the sensor
    assert r["num_valid"] == 16 and np.isnan(r["points"].reshape(4, 8, 3)[0]).all()  # dropped without a normal
    keep = lr.adapt_lidar_sweep(P, m, max_distance_squared=100.0, drop_points_without_normal=False)
    assert keep["num_valid"] == 32 and np.isnan(keep["normals"].reshape(4, 8, 3)[0]).all()
    # the same image under a model that does not wrap (9th column missing from a 9-column sector): border columns get none
    s = lr.Model(m.azimuth_min, m.azimuth_increment, m.elevation_min, m.elevation_increment, 4, 7)
    hs = lr.adapt_lidar_sweep(P, s, max_distance_squared=100.0)["has_normal"].reshape(4, 7)
    assert hs[1:3, 1:6].all() and not hs[:, 0].any() and not hs[:, 6].any()
    # gaps larger than the image, the gate, one missing neighbour
    assert not lr.adapt_lidar_sweep(P, m, col_gap=1, row_gap=2, max_distance_squared=100.0)["has_normal"].any()
    assert lr.adapt_lidar_sweep(P, m, col_gap=9, row_gap=1, max_distance_squared=100.0)["has_normal"].sum() == 16  # 9 mod 8
    assert not lr.adapt_lidar_sweep(P, m, col_gap=8, row_gap=1, max_distance_squared=100.0)["has_normal"].any()  # dc = 0
    assert not lr.adapt_lidar_sweep(P, m, max_distance_squared=0.5)["has_normal"].any()
    hole = lr.adapt_lidar_sweep(np.delete(P, 1 * 8 + 3, axis=0), m, max_distance_squared=100.0)["has_normal"].reshape(4, 8)
    assert not hole[1, 2] and not hole[1, 3] and not hole[1, 4] and not hole[2, 3] and hole[2, 2] and hole[1, 5]
    # collinear neighbours: the cross product vanishes, the pixel is occupied and gets no normal
    cm, line, centre = lc.collinear_sweep()
    r = lr.adapt_lidar_sweep(line, cm, max_distance_squared=100.0, drop_points_without_normal=False)
    assert r["num_in_range"] == 5 and r["occupied"][centre] and not r["has_normal"].any() and r["valid"][centre]
    r = lr.adapt_lidar_sweep(lc.collinear_sweep(0.05)[1], cm, max_distance_squared=100.0)
    assert r["num_in_range"] == 5 and r["has_normal"][centre] and r["num_valid"] == 1


def test_clipper_margins_ties_and_clip_ball_bits():
    m = _model(4, 8)
    rng = np.random.default_rng(5)
    base = lc.full_image(m, 2.0)
    pts = np.concatenate([base, base, base * F(1.5), rng.uniform(-4, 4, (200, 3)).astype(F),
                          [[np.nan, 0, 0], [0.1, 0.1, 0.0], [0, 0, 0]]]).astype(F)
    L = lc.pose(0.2, -0.1, 0.05, yaw_deg=12.0)
    S = lc.pose(0.1, 0.0, 0.2, yaw_deg=-30.0, pitch_deg=4.0)
    fov = lr.clip_spherical(pts, L, m, S, -1.0)
    zero = lr.clip_spherical(pts, L, m, S, 0.0)
    inf = lr.clip_spherical(pts, L, m, S, float("inf"))
    assert fov["num_valid"] == len(pts) - 1 and 0 < zero["num_kept"] < fov["num_kept"] == fov["num_in_view"] < fov["num_valid"]
    assert np.array_equal(inf["global_indices"], fov["global_indices"]) and lr.same_bits(inf["points"], fov["points"])
    # margin 0 keeps every point that ties for its pixel's minimum: the exact duplicates come in pairs
    ident = lr.clip_spherical(pts, I34, m, None, 0.0)
    g = set(ident["global_indices"].tolist())
    assert all((i in g) == (i + 32 in g) for i in range(32)) and sum(i in g for i in range(32)) > 8
    per_pixel = np.bincount(ident["pix"][ident["global_indices"]], minlength=32)
    assert per_pixel.max() >= 2
    # a kept point comes out as clip_ball writes it
    ball_pts, ball_g = lr.clip_ball(pts, L, 1.0e3)
    where = np.searchsorted(ball_g, zero["global_indices"])
    assert np.array_equal(ball_g[where], zero["global_indices"]) and lr.same_bits(ball_pts[where], zero["points"])
    # normals are rotated, features travel
    nrm = rng.normal(size=pts.shape).astype(F)
    withn = lr.clip_spherical(pts, L, m, S, 0.0, normals=nrm, intensity=np.arange(len(pts), dtype=F))
    assert withn["normals"].shape == withn["points"].shape and np.array_equal(withn["intensity"], zero["global_indices"].astype(F))
    e = lr.clip_spherical(np.zeros((0, 3), F), L, m, S, 0.0)
    assert e["status"] == lr.CLIPPER_READY and e["num_kept"] == 0


def test_the_case_is_not_vacuous():
    a = lc.main_case()
    m = a["model"]
    assert (m.rows, m.cols) == (16, 360) and m.valid() and m.columns_wrap() and 5000 < len(a["points"]) < 6500
    r = lr.adapt_lidar_sweep(a["points"], m)
    occ = r["occupied"]
    assert occ.mean() >= 0.80
    assert (r["candidates"][occ] > 1).mean() >= 0.03
    with_normal = r["has_normal"][occ].mean()
    assert 0.60 <= with_normal <= 0.95
    o = lc.occlusion_case()
    fov = lr.clip_spherical(o["points"], o["robot_in_local_map"], o["model"], o["sensor_in_robot"], -1.0)
    occl = lr.clip_spherical(o["points"], o["robot_in_local_map"], o["model"], o["sensor_in_robot"], o["margin"])
    dropped = 1.0 - occl["num_kept"] / fov["num_in_view"]
    assert 0.10 <= dropped <= 0.90 and fov["num_in_view"] < fov["num_valid"]


def test_the_edge_cases_reach_their_edges():
    """every hand-made input does what its name says, on the restatement"""
    got = {}
    for name, m, pts, kw in lc.edge_cases():
        assert m.valid() and 2 <= m.rows <= 4 and 4 <= m.cols <= 8, name
        got[name] = lr.adapt_lidar_sweep(pts, m, drop_points_without_normal=False, **kw)
    assert got["tie goes to the lower index"]["num_in_range"] == 1 and got["tie goes to the lower index"]["candidates"].max() == 4
    for name in ("nearer wins, far first", "nearer wins, near first"):
        r = got[name]
        assert lr.same_bits(r["points"][r["occupied"]], np.asarray([lc.direction(0.12, 0.04, 2.0)], F)), name
    assert got["pixel boundaries"]["occupied"].tolist() == [True, True, False, False, True, True, False, False]
    assert got["pixel boundaries"]["candidates"][5] == 2
    assert got["range gates"]["candidates"].sum() == 2 and got["outside the image"]["candidates"].tolist().count(1) == 1
    assert got["seam, wrapping"]["has_normal"].sum() == 16 and got["seam, wrapping"]["candidates"].max() >= 2
    sec = got["seam, sector across pi"]
    assert sec["occupied"].all() and sec["candidates"].sum() == 32 and sec["has_normal"].reshape(4, 4)[1:3, 1:3].all()
    assert sec["has_normal"].sum() == 4
    assert got["clockwise, rows from the top"]["has_normal"].sum() == 16
    assert got["no wrap: border columns get no normal"]["has_normal"].sum() == 10
    assert got["z axis"]["occupied"].tolist() == [True] + [False] * 11 + [True] + [False] * 3 and got["z axis"]["candidates"][12] == 3
    assert got["column gap beyond one turn"]["has_normal"].sum() == 16
    for name in ("gaps larger than the image", "column gap of one turn", "gate closes", "every point out of view"):
        assert not got[name]["has_normal"].any(), name
    assert got["column gap of one turn"]["occupied"].all() and got["every point out of view"]["num_in_range"] == 0
    assert got["gate on one difference"]["has_normal"].sum() == 12
    assert got["one missing neighbour"]["has_normal"].sum() == 12 and got["collinear neighbours"]["has_normal"].sum() == 0
    assert got["collinear neighbours"]["num_in_range"] == 5 and got["nearly collinear neighbours"]["has_normal"].sum() == 1
    assert got["NaN and inf"]["num_raw"] == 36 and got["NaN and inf"]["has_normal"].sum() == 16
