"""CPU: the numpy restatement of the occupancy grid (tests/gridmap_restatement.py) pinned against a plain per-beam, per-step
Python loop written from DESIGN.md section 4 "Occupancy grid" alone, and its properties: what the GPU test then holds the library
to, bit for bit, is itself held here."""
import math

import numpy as np
import pytest

import gridmap_cases as gc
import gridmap_restatement as gr
from adaptor_restatement import adapt_laser_scan, sincos

F = np.float32
PI = math.pi


def _plain_cell(x, o, res):
    u = np.floor(F(F(x - o) / res))
    if not (u >= F(-2.0 ** 30) and u < F(2.0 ** 30)):
        return None
    return int(u)


def plain_integrate(hits, misses, ranges, poses, sc, g, weight=1):
    """one beam after the other, one step after the other, Python integers behind the end point"""
    nb = sc["num_beams"]
    out = dict(num_beams_total=0, num_returns=0, num_cleared_only=0, num_skipped=0, num_hits_in_grid=0, num_miss_updates=0)
    S = sc["sensor_in_robot"].astype(np.float64)
    rmin, rmax = sc["range_min"], sc["range_max"]
    for k, P in enumerate(np.asarray(poses, F).reshape(-1, 3, 3)):
        A = P.astype(np.float64)
        T = [[F(A[i, 0] * S[0, j] + A[i, 1] * S[1, j]) for j in range(2)] + [F((A[i, 0] * S[0, 2] + A[i, 1] * S[1, 2]) + A[i, 2])]
             for i in range(2)]
        for j in range(nb):
            out["num_beams_total"] += 1
            r = F(np.asarray(ranges, F).reshape(-1, nb)[k, j])
            if np.isfinite(r) and rmin <= r <= rmax:
                reach, hit = r, True
                out["num_returns"] += 1
            elif r > rmax and sc["clear_beyond_max"]:
                reach, hit = rmax, False
                out["num_cleared_only"] += 1
            else:
                out["num_skipped"] += 1
                continue
            s, c = sincos(np.array([sc["angle_min"] + float(j) * sc["angle_increment"]]))
            bx, by = F(F(c[0]) * reach), F(F(s[0]) * reach)
            ex = F(F(F(T[0][0] * bx) + F(T[0][1] * by)) + T[0][2])
            ey = F(F(F(T[1][0] * bx) + F(T[1][1] * by)) + T[1][2])
            cells = [_plain_cell(T[0][2], g["ox"], g["res"]), _plain_cell(T[1][2], g["oy"], g["res"]),
                     _plain_cell(ex, g["ox"], g["res"]), _plain_cell(ey, g["oy"], g["res"])]
            if None in cells:
                continue
            x0, y0, x1, y1 = cells
            dx, dy = x1 - x0, y1 - y0
            n = max(abs(dx), abs(dy))
            if n > 32767:
                continue
            sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
            for i in range(n + 1):
                cx = x0 + (sx * ((2 * i * abs(dx) + n) // (2 * n)) if n else 0)
                cy = y0 + (sy * ((2 * i * abs(dy) + n) // (2 * n)) if n else 0)
                if not (0 <= cx < g["cols"] and 0 <= cy < g["rows"]):
                    continue
                if i < n:
                    misses[cy, cx] += weight
                    out["num_miss_updates"] += 1
                elif hit:
                    hits[cy, cx] += weight
                    out["num_hits_in_grid"] += 1
    return out


def _both(g, sc, poses, ranges, weight=1):
    h, m = gr.new_planes(g)
    out = gr.integrate(h, m, ranges, poses, sc, g, weight)
    hp, mp = gr.new_planes(g)
    outp = plain_integrate(hp, mp, ranges, poses, sc, g, weight)
    assert out == outp
    assert np.array_equal(h, hp) and np.array_equal(m, mp)
    return h, m, out


SMALL = [s for s in gc.SHAPES if s[1] * s[2] <= 400]


@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_restatement_equals_the_plain_loop(shape):
    g, sc, poses, ranges = gc.shape_case(shape, seed=3)
    h, m, out = _both(g, sc, poses, ranges)
    assert out["num_beams_total"] == shape[1] * shape[2]
    if shape[1] * shape[2] and shape[0] != (1, 1):
        assert out["num_hits_in_grid"] > 0 and out["num_miss_updates"] > 0


def test_plain_loop_on_mixed_ranges_a_mounted_and_a_clockwise_scanner():
    mount = gc.pose(0.11, -0.07, 0.4)
    a0, inc = gc.fan(65, clockwise=True)
    for clear in (True, False):
        for origin in ((-1.0, 0.5), (0.3, 0.2)):  # (the second grid leaves the sensor outside for some poses)
            g = gr.grid(7, 5, 0.05, origin)
            sc = gr.scanner(a0, inc, 65, range_min=0.03, range_max=0.6, sensor_in_robot=mount, clear_beyond_max=clear)
            poses = gc.trajectory((-1.0, -0.7, 0.5, 0.9), 3, seed=5)
            ranges = gc.mixed(gc.room_scans((-1.2, -0.6, 0.4, 1.0), poses, sc), seed=6)
            h, m, out = _both(g, sc, poses, ranges)
            assert out["num_skipped"] > 0 and out["num_returns"] > 0
            assert (out["num_cleared_only"] > 0) == clear
    # and taken out again
    _both(g, sc, poses, ranges, weight=-1)


def _ray(x0, y0, x1, y1):
    n = max(abs(x1 - x0), abs(y1 - y0))
    a = np.array
    return [tuple(int(v[0]) for v in gr.step_cells(a([x0]), a([y0]), a([x1]), a([y1]), i)) for i in range(n + 1)]


def test_a_beam_touches_n_plus_1_cells_and_consecutive_cells_are_neighbours():
    rng = np.random.default_rng(1)
    ends = [tuple(int(v) for v in rng.integers(-40, 40, 4)) for _ in range(300)]
    ends += [(0, 0, 0, 0), (3, 3, 3, 9), (3, 3, 9, 3), (3, 3, 3, -9), (3, 3, -9, 3), (0, 0, 7, 7), (0, 0, -7, 7), (0, 0, 7, -7),
             (0, 0, -7, -7), (0, 0, 32767, 1), (5, 5, 5 - 32767, 5 + 32766)]
    for x0, y0, x1, y1 in ends:
        cells = _ray(x0, y0, x1, y1)
        n = max(abs(x1 - x0), abs(y1 - y0))
        assert len(cells) == n + 1 and len(set(cells)) == n + 1
        assert cells[0] == (x0, y0) and cells[-1] == (x1, y1)
        for (ax, ay), (bx, by) in zip(cells, cells[1:]):
            assert max(abs(bx - ax), abs(by - ay)) == 1
        # the reversed ray visits cells that differ from these by at most one cell (rounding of the half falls the other way)
        back = _ray(x1, y1, x0, y0)[::-1]
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) <= 1 for p, q in zip(cells, back))


def _one_beam(g, x, y, bearing, r, **kw):
    sc = gr.scanner(bearing, 0.1, 1, range_min=0.001, range_max=10.0, **kw)
    h, m = gr.new_planes(g)
    out = gr.integrate(h, m, np.array([[r]], F), gc.pose(x, y, 0.0)[None], sc, g)
    return h, m, out


def test_the_end_cell_gets_the_hit_and_no_miss():
    g = gr.grid(9, 9, 0.1, (0.0, 0.0))
    for k in range(16):  # the four axes, the four diagonals and a beam inside every octant
        h, m, out = _one_beam(g, 0.45, 0.45, k * PI / 8, 0.3)
        assert h.sum() == 1 and out["num_hits_in_grid"] == 1
        (iy,), (ix,) = np.nonzero(h)
        assert m[iy, ix] == 0 and m[4, 4] == 1
        n = max(abs(ix - 4), abs(iy - 4))
        assert n == 3 or (k % 4 == 2 and n == 2)  # (0.3 m along a diagonal is 2.1 cells)
        assert m.sum() == n == out["num_miss_updates"] and m.max() == 1
    # n = 0: a hit in the sensor's own cell and nothing else
    h, m, out = _one_beam(g, 0.45, 0.45, 0.7, 0.01)
    assert h[4, 4] == 1 and h.sum() == 1 and m.sum() == 0
    # the end point outside: misses up to the edge, no hit; the sensor outside looking in: the part inside, and the hit
    h, m, out = _one_beam(g, 0.45, 0.45, 0.0, 2.0)
    assert h.sum() == 0 and np.array_equal(np.flatnonzero(m[4]), np.arange(4, 9)) and m.sum() == 5
    h, m, out = _one_beam(g, -0.55, 0.45, 0.0, 0.8)
    assert h[4, 2] == 1 and np.array_equal(np.flatnonzero(m[4]), [0, 1]) and m.sum() == 2
    # through a corner of the grid from outside to outside: only the cells inside count
    h, m, out = _one_beam(g, -0.15, 0.25, -PI / 4, 0.6)
    assert h.sum() == 0 and m.sum() == out["num_miss_updates"] > 0 and m[3:, :].sum() == 0 and m[:, 3:].sum() == 0


def test_plus_one_then_minus_one_restores_zero_and_order_and_split_do_not_matter():
    g, sc, poses, ranges = gc.shape_case(((64, 64), 9, 65), seed=8)
    ranges = gc.mixed(ranges, seed=9)
    h, m = gr.new_planes(g)
    a = gr.integrate(h, m, ranges, poses, sc, g, +1)
    assert h.any() and m.any()
    whole = (h.copy(), m.copy())
    b = gr.integrate(h, m, ranges, poses, sc, g, -1)
    assert not h.any() and not m.any() and a == b
    order = np.random.default_rng(0).permutation(9)
    gr.integrate(h, m, ranges[order], poses[order], sc, g)
    assert np.array_equal(h, whole[0]) and np.array_equal(m, whole[1])
    h2, m2 = gr.new_planes(g)
    parts = [gr.integrate(h2, m2, ranges[s], poses[s], sc, g) for s in (slice(0, 4), slice(4, 5), slice(5, 9))]
    assert np.array_equal(h2, whole[0]) and np.array_equal(m2, whole[1])
    assert {k: sum(p[k] for p in parts) for k in a} == a
    # a removal that was never integrated leaves negative counts: unknown
    h3, m3 = gr.new_planes(g)
    gr.integrate(h3, m3, ranges, poses, sc, g, -1)
    assert h3.min() < 0 and m3.min() < 0
    assert set(np.unique(gr.render(h3, m3))) == {gr.UNKNOWN}


def test_the_three_beam_classes_and_clear_beyond_max():
    g = gr.grid(1, 9, 0.1, (0.0, 0.0))
    rs = np.array([[0.3, np.inf, 5.0, np.nan, 0.0, -1.0, 0.01, -np.inf, 0.5, 0.05]], F)
    for clear in (True, False):
        sc = gr.scanner(0.0, 1e-9, 10, range_min=0.05, range_max=0.5, clear_beyond_max=clear)
        ret, clr = gr.classify(rs, sc)
        assert list(ret[0]) == [True, False, False, False, False, False, False, False, True, True]
        assert list(clr[0]) == [False, clear, clear, False, False, False, False, False, False, False]
        h, m = gr.new_planes(g)
        out = gr.integrate(h, m, rs, gc.pose(0.05, 0.05, 0.0)[None], sc, g)
        assert (out["num_returns"], out["num_cleared_only"], out["num_skipped"]) == (3, 2 * clear, 7 - 2 * clear)
        assert list(h[0]) == [0, 1, 0, 1, 0, 1, 0, 0, 0]  # 0.05 -> cell 1 (0.1), 0.3 -> cell 3 (0.35), 0.5 -> cell 5 (0.55)
        # misses: the three returns (1 + 3 + 5 steps) and, cleared, two rays of 5 steps towards the point at range_max
        assert list(m[0]) == [3 + 2 * clear] + [2 + 2 * clear] * 2 + [1 + 2 * clear] * 2 + [0] * 4
        assert out["num_miss_updates"] == 9 + 10 * clear and out["num_hits_in_grid"] == 3
    assert gr.refuses(g, gr.scanner(0, 0.1, 4, range_max=3300.0)) and not gr.refuses(g, gr.scanner(0, 0.1, 4, range_max=3100.0))
    assert gr.refuses(g, gr.scanner(0, 0.1, 4, range_max=np.inf))


def test_beam_end_points_are_the_scan_adaptors_points():
    """identity pose and mount: the end cell of beam k is the cell of the point srrg2_adapt_laser_scan writes for it"""
    g = gr.grid(64, 64, 0.05, (-1.6, -1.6))
    a0, inc = gc.fan(361)
    sc = gr.scanner(a0, inc, 361, range_min=0.05, range_max=30.0)
    ranges = gc.room_scans((-1.3, 1.2, -1.1, 1.4), np.eye(3)[None], sc)
    b = gr.beams(ranges, np.eye(3, dtype=F)[None], sc, g)
    pts = adapt_laser_scan(ranges[0], a0, inc, half_window=0)["points"]
    assert np.array_equal(b["x1"][0], np.floor((pts[:, 0] - g["ox"]) / g["res"]).astype(np.int64))
    assert np.array_equal(b["y1"][0], np.floor((pts[:, 1] - g["oy"]) / g["res"]).astype(np.int64))


def test_render_and_scene_export():
    h = np.array([[0, 1, 1, 3, 0, -1, 5, 2 ** 31 - 1]], np.int32)
    m = np.array([[0, 0, 1, 1, 7, 4, -1, 2 ** 31 - 1]], np.int32)
    assert list(gr.render(h, m)[0]) == [255, 100, 50, 75, 0, 255, 255, 50]
    assert list(gr.render(h, m, 3)[0]) == [255, 255, 255, 75, 0, 255, 255, 50]
    assert list(gr.render(h, m, -5)[0]) == list(gr.render(h, m, 0)[0]) == list(gr.render(h, m, 1)[0])
    assert list(gr.render(np.array([[1, 1, 199]], np.int32), np.array([[199, 200, 1]], np.int32))[0]) == [1, 0, 100]  # (x.5 rounds up)
    g = gr.grid(1, 8, 0.25, (1.0, -2.0))
    pts, idx = gr.to_scene(h, m, g, 1, 50)
    assert list(idx) == [1, 2, 3, 7] and idx.dtype == np.int32 and pts.dtype == F
    assert np.array_equal(pts, np.array([[1.375, -1.875], [1.625, -1.875], [1.875, -1.875], [2.875, -1.875]], F))
    assert list(gr.to_scene(h, m, g, 1, 0)[1]) == [1, 2, 3, 4, 7] and list(gr.to_scene(h, m, g, 1, 100)[1]) == [1]
    assert list(gr.to_scene(h, m, g, 10 ** 9, 0)[1]) == [7]  # (2^32 - 2 observations)
    assert gr.to_scene(h[:, :7], m[:, :7], gr.grid(1, 7, 0.25), 10 ** 9, 0)[0].shape == (0, 2)


def test_a_room_renders_its_walls_occupied_and_its_interior_free():
    """walls a hair outside cell borders (so every return of a wall lands in ONE column or row of cells), a scanner that sees all
    round, 12 seeded poses in the middle of the room: every wall cell away from the corners renders >= 50, every cell of the
    interior <= 10 (so none is unknown)"""
    g = gr.grid(64, 64, 0.05, (0.0, 0.0))
    room = (0.398, 2.802, 0.398, 2.802)  # wall cells: columns / rows 7 and 56
    sc = gr.scanner(-PI, 2 * PI / 360, 361, range_min=0.05, range_max=10.0)
    poses = gc.trajectory(room, 12, seed=21)
    ranges = gc.room_scans(room, poses, sc)
    h, m = gr.new_planes(g)
    out = gr.integrate(h, m, ranges, poses, sc, g)
    assert out["num_returns"] == out["num_hits_in_grid"] == 12 * 361
    img = gr.render(h, m)
    walls = np.concatenate([img[10:54, 7], img[10:54, 56], img[7, 10:54], img[56, 10:54]])
    print("walls: min %d, interior: max %d" % (walls.min(), img[8:56, 8:56].max()))
    assert walls.min() >= 50
    assert img[8:56, 8:56].max() <= 10
    assert (img[:6] == 255).all() and (img[58:] == 255).all() and (img[:, :6] == 255).all() and (img[:, 58:] == 255).all()
    pts, idx = gr.to_scene(h, m, g)
    assert set(np.flatnonzero(img.reshape(-1) <= 100)[img.reshape(-1)[img.reshape(-1) <= 100] >= 50]) == set(idx)
    assert len(idx) >= 4 * 44 and np.all((np.abs(pts - 1.6).max(axis=1) > 1.15))  # every exported point lies on the walls
