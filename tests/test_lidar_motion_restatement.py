"""CPU: the restatement of the ring tables and the motion de-skew (tests/lidar_motion_restatement.py) against plain float64 numpy
(np.sin, np.cos, matrix Rodrigues: tests/lidar_motion_cases.py) and against the geometry of the room the sweeps were cast in."""
import numpy as np
import pytest

import lidar_cases as lc
import lidar_motion_cases as mc
import lidar_motion_restatement as mr
import lidar_restatement as lr

F = np.float32
D = np.float64


def _ulp_of_largest(points):
    """per point: one float32 ulp of its largest coordinate magnitude"""
    return np.spacing(np.abs(np.asarray(points, F)).max(axis=1)).astype(D)


@pytest.mark.parametrize("reference", [0.0, 0.5, 1.0])
def test_deskew_agrees_with_float64(reference):
    """every coordinate within 1 float32 ulp of the largest coordinate magnitude of its (de-skewed) point"""
    c = mc.moving_case()
    motions = [c["motion"], mc.motion(0.1, -0.3, 0.0, yaw_deg=-100.0, pitch_deg=20.0), mc.motion(0, 0, 0, yaw_deg=0.01)]
    for M in motions:
        got = mr.deskew(c["points"], c["s"], M, reference)
        want = mc.deskew_float64(c["points"], c["s"], M, reference)
        err = np.abs(got.astype(D) - want.astype(D)).max(axis=1)
        assert np.all(err <= _ulp_of_largest(want)), (reference, (err / _ulp_of_largest(want)).max())


def test_identity_motion_returns_the_input_values():
    c = mc.moving_case()
    for reference in (0.0, 0.5, 1.0):
        out = mr.deskew(c["points"], c["s"], np.eye(3, 4, dtype=F), reference)
        assert np.array_equal(out, c["points"])


def test_pure_translation_takes_the_zero_axis_branch():
    c = mc.moving_case()
    M = np.eye(3, 4, dtype=F)
    M[:, 3] = (0.3, -0.2, 0.05)
    theta, a, t = mr.axis_angle(M)
    assert theta == 0.0 and list(a) == [0.0, 0.0, 1.0] and np.array_equal(t, M[:, 3].astype(D))
    for reference in (0.0, 0.5, 1.0):
        want = (c["points"].astype(D) + (c["s"] - reference)[:, None] * M[:, 3].astype(D)).astype(F)
        got = mr.deskew(c["points"], c["s"], M, reference)
        assert np.all(np.abs(got.astype(D) - want.astype(D)).max(axis=1) <= _ulp_of_largest(want))


def test_axis_angle_of_the_motion():
    theta, a, t = mr.axis_angle(mc.motion())
    th, ax, tt = mc.axis_angle(mc.motion())
    assert abs(theta - th) < 1e-12 and np.abs(a - ax).max() < 1e-9 and np.array_equal(t, tt)
    assert 0.17 < theta < 0.18 and 0.40 < np.linalg.norm(t) < 0.42  # about 10 degrees and 0.41 m


def test_uniform_table_gives_the_uniform_pixels():
    """on every point of the main case (its points stay at least 0.05 pixel from a row boundary)"""
    a = lc.main_case()
    m = a["model"]
    x, y, z = a["points"].T
    pix_u, rho_u = lr.project(x, y, z, m)
    pix_r, rho_r, _ = mr.project_rings(x, y, z, m, mc.uniform_table())
    assert np.array_equal(pix_u, pix_r) and np.array_equal(rho_u, rho_r) and (pix_u >= 0).all()
    el = np.arctan2(z.astype(D), np.hypot(x.astype(D), y.astype(D)))
    rf = (el - m.elevation_min) / m.elevation_increment + 0.5
    assert np.abs(rf - np.round(rf)).min() >= 0.05
    # the descending table: the same rows counted from the top
    pix_d, _, _ = mr.project_rings(x, y, z, m, mc.uniform_table()[::-1].copy())
    assert np.array_equal(pix_d // m.cols, m.rows - 1 - pix_u // m.cols) and np.array_equal(pix_d % m.cols, pix_u % m.cols)


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_boundary_points_of_the_symmetric_tables(descending):
    """z = 0 lies exactly on b[2] = 0 and gets row 2 either way; just outside b[0] / b[rows] is out of view"""
    e, pts, rows = mc.boundary_points(descending)
    B, desc = mr.ring_boundaries(e)
    assert desc == descending and B[2] == 0.0 and np.all(np.diff(B) > 0)
    m = lr.Model.full_turn(4, 8, e[0], e[-1])
    pix, _, _ = mr.project_rings(pts[:, 0], pts[:, 1], pts[:, 2], m, e)
    assert np.array_equal(np.where(pix < 0, -1, pix // m.cols), rows)
    assert rows[0] == rows[1] == 2 and (rows == -1).sum() == 2


def test_ring_table_refusals():
    ok = mc.two_block_table()
    assert mr.ring_table_status(ok, 16) is None and mr.ring_table_status(ok[::-1], 16) is None
    assert mr.ring_table_status(ok[:1], 1) == "invalid"
    assert mr.ring_table_status(np.linspace(-1, 1, 257), 257) == "unsupported"
    for k, v in ((3, np.nan), (3, np.inf), (15, 1.5708), (3, ok[2]), (3, ok[5])):
        bad = ok.copy()
        bad[k] = v
        assert mr.ring_table_status(bad, 16) == "invalid", (k, v)
    edge = ok.copy()
    edge[15] = np.pi / 2 * (1 + 2.0 ** -20)  # the slack admits it
    assert mr.ring_table_status(edge, 16) is None


@pytest.mark.parametrize("table", ["uniform", "two_block", "two_block_desc"])
@pytest.mark.parametrize("reference", [0.0, 0.5, 1.0])
def test_deskewed_sweep_lies_on_the_room(table, reference):
    """16 x 360, 0.41 m and 10 degrees per sweep: de-skewed and carried into the room by the TRUE pose at `reference`, every point
    lies within 1e-5 m of a surface (float32 half-ulps of inputs and outputs below 16 m sum to under 3e-6); raw, the worst is
    beyond 0.1 m"""
    c = mc.moving_case(table)
    out = mr.deskew(c["points"], c["s"], c["motion"], reference)
    pose = mc.pose_at(c["start_in_room"], c["motion"], reference)
    d = mc.surface_distance(mc.to_room(out, pose))
    raw = mc.surface_distance(mc.to_room(c["points"], pose))
    print("reference %.1f %s: de-skewed max %.3g m, raw max %.3g m median %.3g m" % (reference, table, d.max(), raw.max(), np.median(raw)))
    assert d.max() <= 1e-5
    assert raw.max() > 0.1


def test_adaptor_restatement_bins_raw_and_stores_deskewed():
    """the image is the firing grid: occupancy and winners are those of the raw sweep, the stored points the de-skewed winners"""
    c = mc.moving_case()
    m = c["model"]
    plain = lr.adapt_lidar_sweep(c["points"], m, col_gap=0, row_gap=0)
    got = mr.adapt_lidar_sweep_ex(c["points"], m, motion=c["motion"], times=c["times"], time_begin=0.0, time_end=1.0, col_gap=0,
                                  row_gap=0)
    assert np.array_equal(plain["occupied"], got["occupied"]) and got["num_in_range"] == plain["num_in_range"] > 5000
    w = got["winner_index"]
    occ = w >= 0
    assert np.array_equal(plain["points"][occ], c["points"][w[occ]])
    assert np.array_equal(got["points"][occ], mr.deskew(c["points"], c["s"], c["motion"], 1.0)[w[occ]])
    # the azimuth fallback: without the columns fired twice the time is the firing fraction up to rounding
    n = mc.moving_case(overlap=False)
    fb = mr.adapt_lidar_sweep_ex(n["points"], m, motion=n["motion"])
    pose = mc.pose_at(n["start_in_room"], n["motion"], 1.0)
    keep = fb["valid"]
    assert mc.surface_distance(mc.to_room(fb["points"][keep], pose)).max() <= 1e-5
    # defaults: the plain restatement
    same = mr.adapt_lidar_sweep_ex(c["points"], m)
    assert lr.same_bits(same["points"], lr.adapt_lidar_sweep(c["points"], m)["points"])
    # a NaN time takes its point out of the image
    tm = c["times"].copy()
    k = int(w[occ][10])
    tm[k] = np.nan
    nan = mr.adapt_lidar_sweep_ex(c["points"], m, motion=c["motion"], times=tm, time_begin=0.0, time_end=1.0, col_gap=0, row_gap=0)
    assert k not in set(nan["winner_index"].tolist()) and nan["num_in_range"] in (got["num_in_range"], got["num_in_range"] - 1)
