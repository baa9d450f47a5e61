"""CPU: the numpy restatement of the scan clipper (tests/clip_scan_restatement.py): its atan2 against the oracle's bit for bit,
hand-made scenes with known answers, the round trip with the laser scan adaptor's restatement (every beam of a scan falls into
its own bin) and the monotonicity of the kept set in the occlusion margin."""
import math

import numpy as np
import pytest

import adaptor_restatement as ar
import clip_scan_restatement as cs

F = np.float32
I3 = np.eye(3, dtype=F)
PI = math.pi
FULL360 = (-PI, 2 * PI / 360, 360)
# the scanners of the issue: (angle_min, angle_increment, num_beams)
SCANNERS = [(-PI, 2 * PI / 360, 360), (-PI, 2 * PI / 360, 361), (-2.35619, 4.71238 / 1080, 1081), (0.0, 2 * PI / 1000, 1000),
            (2.0, -0.004, 1000), (-1.0, 0.002, 1000), (PI / 2, 2 * PI / 720, 720)]


def _clip(points, scanner=FULL360, **kw):
    kw.setdefault("robot_in_local_map", I3)
    return cs.clip_scan(np.asarray(points, F).reshape(-1, 2), kw.pop("robot_in_local_map"), *scanner, **kw)


def _polar(rho, bearing):
    return [rho * math.cos(bearing), rho * math.sin(bearing)]


def test_atan2_is_the_oracles_bit_for_bit(oracle):
    rng = np.random.default_rng(1)
    y = np.concatenate([rng.normal(size=4000) * 10.0 ** rng.integers(-6, 6, 4000), rng.uniform(-1, 1, 3000),
                        rng.normal(size=3000).astype(F).astype(np.float64)])
    x = np.concatenate([rng.normal(size=4000) * 10.0 ** rng.integers(-6, 6, 4000), rng.uniform(-1, 1, 3000),
                        rng.normal(size=3000).astype(F).astype(np.float64)])
    # the reduction's interval borders, the axes, the origin and signed zeros
    edge = [0.4375, 0.6875, 1.1875, 2.4375, 1.0, np.nextafter(0.4375, 0), np.nextafter(2.4375, 9)]
    ys = [0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 5e-324, 1e300] + edge + [-e for e in edge]
    xs = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0, -1e300, 5e-324] + [1.0] * 7 + [-1.0] * 7
    y, x = np.concatenate([y, ys]), np.concatenate([x, xs])
    got = cs.atan2(y, x)
    want = np.array([oracle.atan2(float(a), float(b)) for a, b in zip(y, x)])
    assert len(y) > 10_000 and got.tobytes() == want.tobytes()
    assert float(cs.atan2(-0.0, -1.0)) == float(cs.atan2(0.0, -1.0)) == PI  # y = -0 counts as +0 (libm would answer -pi)
    assert np.max(np.abs(got - np.arctan2(y, x))[np.abs(np.abs(np.arctan2(y, x)) - PI) > 1e-9]) < 1e-15


def test_a_point_behind_a_wall_on_the_same_beam():
    pts = [[1.0, 0.0], [2.0, 0.0], [1.04, 0.0], [0.0, 3.0], [0.0, 1.5]]
    r = _clip(pts, occlusion_margin=0.0)
    assert list(r["beam"]) == [180, 180, 180, 270, 270] and list(r["rho"]) == [F(1.0), F(2.0), F(1.04), F(3.0), F(1.5)]
    assert list(r["global_indices"]) == [0, 4]
    assert (r["num_valid"], r["num_in_view"], r["num_kept"], r["status"]) == (5, 5, 2, cs.CLIPPER_SUCCESSFUL)
    assert list(_clip(pts, occlusion_margin=0.05)["global_indices"]) == [0, 2, 4]
    assert list(_clip(pts, occlusion_margin=1.2)["global_indices"]) == [0, 1, 2, 4]  # larger than the first gap, not the second
    for everything in (_clip(pts, occlusion_margin=1.6), _clip(pts, occlusion_margin=np.inf), _clip(pts)):
        assert list(everything["global_indices"]) == [0, 1, 2, 3, 4]
    assert cs.same_bits(r["points"], np.asarray(pts, F)[[0, 4]])  # identity pose: the coordinates as they were


def test_exact_ties_in_range_are_all_kept_at_margin_zero():
    pts = [[3.0, 4.0], [3.0, 4.0], [3.0000002, 4.0], [5.0 * math.cos(0.9273), 5.0 * math.sin(0.9273)], [6.0, 8.0]]
    r = _clip(pts, occlusion_margin=0.0)
    assert len(set(r["beam"])) == 1 and r["rho"][0] == r["rho"][1] == F(5.0)
    ties = np.flatnonzero(r["rho"] == r["rho"].min())
    assert len(ties) >= 2 and list(r["global_indices"]) == list(ties)


@pytest.mark.parametrize("y", [0.0, -0.0], ids=["plus_zero", "minus_zero"])
def test_the_negative_x_axis_on_a_full_circle(y):
    pts = np.array([[-1.0, y], [-2.0, y]], F)
    assert np.signbit(pts[0, 1]) == (math.copysign(1.0, y) < 0)
    r360 = _clip(pts, (-PI, 2 * PI / 360, 360))
    assert list(r360["beam"]) == [0, 0] and r360["num_in_view"] == 2  # bearing +pi: one turn back, into the first bin
    r361 = _clip(pts, (-PI, 2 * PI / 360, 361))
    assert list(r361["beam"]) == [360, 360] and r361["num_in_view"] == 2  # the closing beam has a bin of its own
    # just below the axis both scanners put it into bin 0
    below = np.array([[-1.0, -1e-4]], F)
    assert list(_clip(below, (-PI, 2 * PI / 360, 360))["beam"]) == [0] and list(_clip(below, (-PI, 2 * PI / 360, 361))["beam"]) == [0]


def test_a_clockwise_scanner():
    scanner = (2.0, -0.004, 1000)  # beams from 2.0 rad down to -1.996 rad
    pts = [_polar(2.0, 0.0), _polar(2.0, 2.0), _polar(2.0, -1.9), _polar(2.0, 2.5), _polar(2.0, PI - 0.01), _polar(2.0, -2.1),
           _polar(3.0, 0.0)]
    r = _clip(pts, scanner, occlusion_margin=0.0)
    assert list(r["beam"]) == [500, 0, 975, -1, -1, -1, 500]
    assert list(r["global_indices"]) == [0, 1, 2] and r["num_in_view"] == 4


def test_half_an_increment_outside_each_end_of_a_270_degree_sector():
    a0, inc, nb = scanner = (-2.35619, 4.71238 / 1080, 1081)
    last = a0 + (nb - 1) * inc
    # a beam's bin reaches half an increment to either side: 0.49 increments outside the end beams is inside, 0.51 outside
    pts = [_polar(5.0, a0 - 0.49 * inc), _polar(5.0, a0 - 0.51 * inc), _polar(5.0, last + 0.49 * inc), _polar(5.0, last + 0.51 * inc),
           _polar(5.0, a0), _polar(5.0, last), _polar(5.0, PI), _polar(5.0, -PI + 0.2)]
    assert list(_clip(pts, scanner)["beam"]) == [0, -1, 1080, -1, 0, 1080, -1, -1]


def exact_bin_edges():
    """one point and two scanners (increment 0.25, 2 beams) whose bin edges fall EXACTLY on its bearing: angle_min = beta + 0.125
    puts it on the lower edge of bin 0 (tf == 0: in), angle_min = beta - 0.375 on the upper edge of bin 1 (tf == num_beams:
    out).  beta lies in [0.5, 0.75), where both sums are exact in float64."""
    pt = np.array([[1.0, 0.7]], F)
    beta = float(cs.atan2(np.float64(pt[0, 1]), np.float64(pt[0, 0])))
    assert 0.5 <= beta < 0.75
    low, high = beta + 0.125, beta - 0.375
    assert beta - low == -0.125 and beta - high == 0.375
    return pt, (low, 0.25, 2), (high, 0.25, 2)


def test_a_bearing_exactly_on_a_bin_edge():
    pt, on_lower, on_upper = exact_bin_edges()
    assert list(_clip(pt, on_lower)["beam"]) == [0] and list(_clip(pt, on_upper)["beam"]) == [-1]
    # the scanner turned by 1e-12 rad: now inside the upper edge, and outside the lower one
    assert list(_clip(pt, (on_upper[0] + 1e-12, 0.25, 2))["beam"]) == [1]
    assert list(_clip(pt, (on_lower[0] + 1e-12, 0.25, 2))["beam"]) == [-1]


def test_range_interval_is_inclusive_at_both_ends():
    pts = [[0.5, 0.0], [8.0, 0.0], [0.0, -8.0], [np.nextafter(F(0.5), F(0)), 0.0], [np.nextafter(F(8.0), F(9)), 0.0], [4.8, 6.4],
           [0.0, 0.0]]
    r = _clip(pts, range_min=0.5, range_max=8.0)
    assert r["rho"][5] == F(8.0)
    assert list(r["global_indices"]) == [0, 1, 2, 5] and (r["num_valid"], r["num_in_view"]) == (7, 4)


def test_invalid_points_keep_their_index_out_of_the_result():
    pts = [[np.nan, 1.0], [1.0, 0.0], [0.0, np.inf], [-np.inf, 0.0], [1.0, 1.0], [1.0, np.nan]]
    inten = np.arange(6, dtype=F)
    desc = np.arange(6 * 32, dtype=np.uint8).reshape(6, 32)
    nrm = np.tile(np.array([[0.0, 1.0]], F), (6, 1))
    r = _clip(pts, intensity=inten, descriptors=desc, normals=nrm, occlusion_margin=0.0)
    assert list(r["global_indices"]) == [1, 4] and r["num_valid"] == 2 and r["num_in_view"] == 2
    assert list(r["intensity"]) == [1.0, 4.0] and np.array_equal(r["descriptors"], desc[[1, 4]]) and cs.same_bits(r["normals"], nrm[:2])
    empty = _clip(np.zeros((0, 2), F), normals=np.zeros((0, 2), F))
    assert empty["status"] == cs.CLIPPER_READY and empty["num_kept"] == 0 and empty["normals"].shape == (0, 2)


def test_a_sensor_mounted_off_centre_and_rotated():
    S = np.array([[0, -1, 0.5], [1, 0, 0], [0, 0, 1]], F)  # 0.5 m ahead of the robot's centre, looking to its left
    L = np.array([[1, 0, 1.0], [0, 1, 0], [0, 0, 1]], F)    # the robot stands at x = 1 in the local map
    scanner = (-PI / 4, PI / 180, 91)                        # 90 degrees, one beam per degree, beam 45 straight ahead
    pts = np.array([[1.5, 2.0],    # robot (0.5, 2) = sensor (2, 0): straight ahead
                    [1.5, 4.0],    # behind it on the same beam
                    [3.5, 0.0],    # robot (2.5, 0) = sensor (0, -2): to the sensor's right, out of the sector
                    [0.5, 1.0],    # sensor (1, 1): the last beam
                    [1.5, -2.0]], F)  # behind the sensor
    nrm = np.array([[0, -1.0], [0, -1.0], [1.0, 0], [1.0, 0], [0, 1.0]], F)
    r = cs.clip_scan(pts, L, *scanner, sensor_in_robot=S, normals=nrm)
    assert list(r["beam"]) == [45, 45, -1, 90, -1] and list(r["rho"][:2]) == [2.0, 4.0]
    assert cs.same_bits(r["points"], [[0.5, 2.0], [0.5, 4.0], [-0.5, 1.0]]) and cs.same_bits(r["normals"], nrm[[0, 1, 3]])
    assert list(cs.clip_scan(pts, L, *scanner, sensor_in_robot=S, occlusion_margin=0.5)["global_indices"]) == [0, 3]
    # a robot yawed by +90 degrees: points and normals turn into its frame
    Lr = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    q = cs.clip_scan(np.array([[-2.0, 0.5]], F), Lr, *scanner, sensor_in_robot=S, normals=np.array([[1.0, 0]], F))
    assert q["num_kept"] == 1 and cs.same_bits(q["points"], [[0.5, 2.0]]) and cs.same_bits(q["normals"], [[0.0, -1.0]])


@pytest.mark.parametrize("scanner", SCANNERS, ids=lambda s: "%g_%d" % (s[0], s[2]))
def test_round_trip_with_the_scan_adaptor(scanner):
    """every Valid beam k of an organised scan comes back in bin k, nothing is dropped.  (The ranges stay clear of range_min and
    range_max: the adaptor tests the raw range, the clipper the length of the float32 point, which may differ by an ulp.)"""
    a0, inc, nb = scanner
    rng = np.random.default_rng(nb)
    k = np.arange(nb)
    ranges = (6.0 + 3.0 * np.sin(k * 0.05) + rng.uniform(-0.5, 0.5, nb) + 15.0 * (k % 97 == 0)).astype(F)
    ranges[rng.integers(0, nb, nb // 20)] = rng.choice(np.array([0.0, np.nan, np.inf, 31.0, 0.01], F), nb // 20)
    scan = ar.adapt_laser_scan(ranges, a0, inc, half_window=1, drop_points_without_normal=False)
    valid = scan["valid"]
    assert 0.9 * nb < valid.sum() < nb
    r = cs.clip_scan(scan["points"], I3, a0, inc, nb, occlusion_margin=0.0, normals=scan["normals"])
    assert r["num_in_view"] == r["num_valid"] == r["num_kept"] == int(valid.sum())
    assert np.array_equal(r["global_indices"], np.flatnonzero(valid))
    assert np.array_equal(r["beam"][valid], k[valid]) and np.all(r["beam"][~valid] == -1)
    assert cs.same_bits(r["points"], scan["points"][valid])


def test_the_kept_set_grows_with_the_margin():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-12, 12, (20_000, 2)).astype(F)
    pts[::50] = np.nan
    L = np.array([[math.cos(0.3), -math.sin(0.3), 0.4], [math.sin(0.3), math.cos(0.3), -0.2], [0, 0, 1]], F)
    kept = {m: set(cs.clip_scan(pts, L, -2.35619, 4.71238 / 1080, 1081, 0.05, 10.0, occlusion_margin=m)["global_indices"])
            for m in (-1.0, np.inf, 1.0, 0.05, 0.0)}
    assert kept[-1.0] == kept[np.inf] and kept[np.inf] > kept[1.0] > kept[0.05] > kept[0.0]
    assert 0 < len(kept[0.0]) <= 1081
