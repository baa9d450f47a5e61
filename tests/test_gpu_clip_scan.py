"""GPU: srrg2_scene_clip_scan (csrc/scene.hip) against the numpy restatement of its contract (tests/clip_scan_restatement.py),
BIT FOR BIT: coordinates, normals, features, global indices and counts, through both per-beam minimum kernels (the LDS table and
the global one); refusals leave `clipped` as it was; and through the stack: a 2-D frame adapt -> clip -> align -> merge equals
the same frame on the oracle with restatement-made inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import adaptor_restatement as ar
import clip_scan_restatement as cs
from helpers import assert_same_run, cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
I3 = np.eye(3, dtype=F)
PI = math.pi
E_INVALID, E_UNSUPPORTED = -1, -4
# num_beams -> (angle_min, angle_increment): one wide bin, a full circle, a 270-degree scanner, and a clockwise full circle
# with more bins than any LDS table holds (160 KB / 4 B = 40 960)
SCANNERS = {1: (0.3, 0.5), 360: (-PI, 2 * PI / 360), 1081: (-2.35619, 4.71238 / 1080), 100_000: (PI, -2 * PI / 100_000)}
MARGINS = (-1.0, 0.0, 0.05, 1.0, float("inf"))


def _random_scene(n, seed, invalid=True, duplicates=True):
    """points around the robot (some beyond the range interval, exact duplicates for range ties), unit normals, descriptors,
    intensities"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-12, 12, (n, 2)).astype(F)
    if duplicates and n >= 8:
        src = rng.integers(0, n, n // 8)
        pts[rng.integers(0, n, n // 8)] = pts[src]
    if invalid and n >= 4:
        bad = rng.integers(0, n, max(1, n // 50))
        pts[bad, rng.integers(0, 2, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    nrm = rng.normal(size=(n, 2))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    return pts, nrm, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F)


def _pose(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return syn.se2(*(scale * rng.uniform(-0.5, 0.5, 2)), scale * np.deg2rad(rng.uniform(-40, 40))).astype(F)


def _fill(scene, pts, nrm=None, desc=None, inten=None):
    scene.set(pts, nrm)
    if desc is not None or inten is not None:
        scene.set_features(desc, inten)


def _clipper(b, full, clipped, beams, pose=I3, sensor=None, margin=-1.0, ranges=(0.05, 10.0), scanner=None):
    cl = mapping.SceneClipperScan(b)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    if sensor is not None:
        cl.set_sensor_in_robot(sensor)
    cl.params.angle_min, cl.params.angle_increment = scanner or SCANNERS[beams]
    cl.params.num_beams = beams
    cl.params.range_min, cl.params.range_max = ranges
    cl.params.occlusion_margin = margin
    return cl


def _restate(pts, beams, pose=I3, sensor=None, margin=-1.0, ranges=(0.05, 10.0), scanner=None, **kw):
    a0, inc = scanner or SCANNERS[beams]
    return cs.clip_scan(pts, pose, a0, inc, beams, ranges[0], ranges[1], sensor_in_robot=sensor, occlusion_margin=margin, **kw)


def _check(clipped, r, res, what):
    assert clipped.size() == r["num_kept"], what
    pts, nrm = clipped.get()
    assert cs.same_bits(pts, r["points"]), what
    _, nptr, _ = clipped.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and cs.same_bits(nrm, r["normals"]), what
    assert clipped.has_features() == (r["descriptors"] is not None, r["intensity"] is not None), what
    d, i = clipped.features()
    if r["descriptors"] is not None:
        assert np.array_equal(d, r["descriptors"]), what
    if r["intensity"] is not None:
        assert cs.same_bits(i, r["intensity"]), what
    assert np.array_equal(clipped.global_indices(), r["global_indices"]), what
    if res is not None:
        assert res == {k: r[k] for k in ("status", "num_valid", "num_in_view", "num_kept")}, (what, res)


def _snapshot(scene):
    pts, nrm = scene.get()
    d, i = scene.features()
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if d is None else d.tobytes(),
            None if i is None else i.tobytes(), scene.global_indices().tobytes())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 300_000])
def test_random_scenes_match_the_restatement(product, n):
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    pts, nrm, desc, inten = _random_scene(n, 100 + n)
    kept, ran = [], set()
    for fi, feats in enumerate(((None, None, None), (nrm, None, None), (nrm, desc, None), (None, None, inten), (nrm, desc, inten))):
        _fill(full, pts, *feats)
        for mi, margin in enumerate(MARGINS):
            if n > 1000 and fi not in (0, 4) and mi not in (0, 1):
                continue  # (the large scene: every margin with and without everything, two margins in between)
            # (the large scene: ONE scanner per combination, in turn; fi and mi are such that each meets margins >= 0)
            for beams in (SCANNERS if n <= 1000 else [list(SCANNERS)[(fi + mi) % 4]]):
                pose, sensor = _pose(7 * fi + mi), (None if mi % 2 else _pose(50 + mi, 0.5))
                cl = _clipper(b, full, clipped, beams, pose, sensor, margin)
                res = cl.compute()
                assert cl.status() == (mapping.CLIPPER_SUCCESSFUL if n else mapping.CLIPPER_READY)
                r = _restate(pts, beams, pose, sensor, margin, normals=feats[0], descriptors=feats[1], intensity=feats[2])
                _check(clipped, r, res, (n, fi, margin, beams))
                kept.append((margin, beams, r["num_kept"], r["num_in_view"], r["num_valid"]))
                if margin >= 0:
                    ran.add(beams)
        # +inf is sector-only mode
        a = _clipper(b, full, clipped, 1081, margin=float("inf")).compute()
        snap = _snapshot(clipped)
        assert a == _clipper(b, full, clipped, 1081, margin=-1.0).compute() and _snapshot(clipped) == snap
    assert ran == set(SCANNERS)  # both minimum kernels ran: tables that fit the LDS and one that cannot
    if n >= 1000:  # not vacuous: occlusion removes points, invalid points exist, not everything is in view
        for beams in (360, 1081):
            assert any(m == 0.0 and nb == beams and 0 < k < v < nv < n for m, nb, k, v, nv in kept), kept


def test_contended_beams_with_many_exact_ties(product):
    """200 000 points on 8 beams: every workgroup hits the same few bins; the points are drawn from 64 positions, so each beam's
    minimum is taken thousands of times over"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    rng = np.random.default_rng(8)
    bearing, radius = np.meshgrid(np.arange(8) * (2 * PI / 8) - PI + 0.01, 1.0 + 0.75 * np.arange(8), indexing="ij")
    base = np.stack([radius * np.cos(bearing), radius * np.sin(bearing)], -1).reshape(64, 2).astype(F)
    pts = base[rng.integers(0, 64, 200_000)]
    inten = rng.random(len(pts), dtype=F)
    _fill(full, pts, None, None, inten)
    scanner = (-PI, 2 * PI / 8)
    for margin, sensor in ((0.0, None), (0.0, _pose(3, 0.2)), (0.75, None)):
        res = _clipper(b, full, clipped, 8, _pose(1, 0.1), sensor, margin, scanner=scanner).compute()
        r = _restate(pts, 8, _pose(1, 0.1), sensor, margin, scanner=scanner, intensity=inten)
        _check(clipped, r, res, ("contended", margin))
        assert len(set(r["beam"])) == 8 and 8 * 1000 < r["num_kept"] < r["num_in_view"] == len(pts)


def test_a_bearing_exactly_on_a_bin_edge(product):
    from test_clip_scan_restatement import exact_bin_edges

    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    pt, on_lower, on_upper = exact_bin_edges()
    full.set(pt)
    for scanner, kept in ((on_lower, 1), (on_upper, 0), ((on_upper[0] + 1e-12, 0.25, 2), 1),
                          ((on_lower[0] + 1e-12, 0.25, 2), 0)):
        for margin in (-1.0, 0.0):
            res = _clipper(b, full, clipped, 2, margin=margin, scanner=scanner[:2]).compute()
            _check(clipped, _restate(pt, 2, margin=margin, scanner=scanner[:2]), res, (scanner, margin))
            assert res["num_kept"] == kept


def test_result_pointer_may_be_null(product):
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    pts, nrm, _, _ = _random_scene(5000, 21)
    _fill(full, pts, nrm)
    cl = _clipper(b, full, clipped, 360, margin=0.0)
    assert cl.compute(want_result=False) is None and cl.status() == mapping.CLIPPER_SUCCESSFUL
    _check(clipped, _restate(pts, 360, margin=0.0, normals=nrm), None, "out == NULL")


def test_reused_handle_follows_a_moving_pose(product):
    """the same `clipped` as the pose moves: the scatter runs behind the scan without the host knowing the total; then a clip whose
    total exceeds the room left from the call before (= the result on a fresh handle); then smaller clips, ball and scan in turn"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    pts, nrm, desc, inten = _random_scene(300_000, 33)
    _fill(full, pts, nrm, desc, inten)
    kw = dict(normals=nrm, descriptors=desc, intensity=inten)
    # a thin ring first: a small result, little room
    res = _clipper(b, full, clipped, 1081, ranges=(3.0, 3.005)).compute()
    r = _restate(pts, 1081, ranges=(3.0, 3.005), **kw)
    _check(clipped, r, res, "narrow")
    small = r["num_kept"]
    assert 0 < small < 1000
    res = _clipper(b, full, clipped, 1081, margin=float("inf")).compute()
    r = _restate(pts, 1081, margin=float("inf"), **kw)
    assert r["num_kept"] > 20 * max(small, 1024)  # beyond any room the small result left
    _check(clipped, r, res, "grown")
    fresh = mapping.Scene(b, 2)
    _clipper(b, full, fresh, 1081, margin=float("inf")).compute()
    assert _snapshot(fresh) == _snapshot(clipped)
    for k in range(6):  # the room is there now: every one of these takes the speculative scatter
        pose, margin = _pose(200 + k, 0.3 * k), (-1.0, 0.0, 0.05)[k % 3]
        res = _clipper(b, full, clipped, 360, pose, margin=margin, ranges=(0.05, 6.0)).compute()
        _check(clipped, _restate(pts, 360, pose, margin=margin, ranges=(0.05, 6.0), **kw), res, ("moving", k))
    ball = mapping.SceneClipperBall(b, range_max=4.0)
    ball.set_full_scene(full); ball.set_clipped_scene_in_robot(clipped)
    for k in range(3):
        pose = _pose(300 + k)
        ball.set_robot_in_local_map(pose); ball.compute()
        with np.errstate(all="ignore"):
            q = cs.xform(cs.se2_inverse(pose), pts)
            inside = np.isfinite(pts).all(1) & (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] <= F(4.0) * F(4.0))
        assert np.array_equal(clipped.global_indices(), np.flatnonzero(inside)) and cs.same_bits(clipped.get()[0], q[inside])
        res = _clipper(b, full, clipped, 1081, pose, margin=0.0).compute()
        _check(clipped, _restate(pts, 1081, pose, margin=0.0, **kw), res, ("alternating", k))


def test_coordinates_are_clip_balls(product):
    b = product.scene_binding(0)
    full, by_ball, by_scan = mapping.Scene(b, 2), mapping.Scene(b, 2), mapping.Scene(b, 2)
    pts, nrm, _, _ = _random_scene(50_000, 44)
    _fill(full, pts, nrm)
    pose = _pose(5)
    ball = mapping.SceneClipperBall(b, range_max=1000.0)
    ball.set_full_scene(full); ball.set_clipped_scene_in_robot(by_ball); ball.set_robot_in_local_map(pose); ball.compute()
    _clipper(b, full, by_scan, 1081, pose, _pose(6, 0.5), 0.1).compute()
    gb, gc = by_ball.global_indices(), by_scan.global_indices()
    assert len(gc) > 1000 and np.all(np.isin(gc, gb))
    at = np.searchsorted(gb, gc)
    for k in (0, 1):  # coordinates, normals
        assert by_ball.get()[k][at].tobytes() == by_scan.get()[k].tobytes()


def test_refusals_leave_clipped_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    b = product.scene_binding(0)
    full, clipped, s3a, s3b = mapping.Scene(b, 2), mapping.Scene(b, 2), mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, desc, inten = _random_scene(3000, 55)
    _fill(full, pts, nrm, desc, inten)
    _clipper(b, full, clipped, 360, margin=0.0, ranges=(0.05, 30.0)).compute()  # (what call() below asks for)
    p3 = np.random.default_rng(1).uniform(-3, 3, (100, 3)).astype(F)
    s3a.set(p3); s3b.set(p3[:50])
    before, before3 = _snapshot(clipped), _snapshot(s3b)
    assert before[0] > 100
    pp = np.ascontiguousarray(I3).ctypes.data_as(C.POINTER(C.c_float))
    fn = lib.srrg2_scene_clip_scan
    inc = 2 * PI / 360

    def call(f=full, c=clipped, T=pp, params=True, **edit):
        p = mapping.default_scan_clip_params()
        p.angle_min, p.angle_increment, p.num_beams, p.occlusion_margin = -PI, inc, 360, 0.0
        for k, v in edit.items():
            setattr(p, k, v)
        out = mapping.ClipResult()
        return fn(f._h, T, C.byref(p) if params else None, c._h, C.byref(out))

    none = mapping.Scene.__new__(mapping.Scene)
    none._h = None
    nan, inf = float("nan"), float("inf")
    invalid = [dict(f=none), dict(c=none), dict(T=None), dict(params=False), dict(c=full), dict(c=s3b), dict(f=s3a),
               dict(num_beams=0), dict(num_beams=-5), dict(angle_increment=0.0), dict(angle_increment=nan),
               dict(angle_increment=inf), dict(angle_min=nan), dict(angle_min=-inf), dict(angle_min=6.3), dict(angle_min=-6.3),
               dict(num_beams=362), dict(num_beams=720), dict(angle_increment=-inc, num_beams=362),
               dict(range_min=0.0), dict(range_min=-1.0), dict(range_min=nan), dict(range_max=0.04), dict(range_max=nan),
               dict(occlusion_margin=nan)]
    for kw in invalid:
        assert call(**kw) == E_INVALID, kw
        assert b.err()  # (the error text is set)
    assert call(f=s3a, c=s3b) == E_UNSUPPORTED  # 3-D scenes
    assert _snapshot(clipped) == before and _snapshot(s3b) == before3
    if _capi.device_count() > 1:
        other = mapping.Scene(product.scene_binding(1), 2)
        assert call(c=other) == E_INVALID
    assert call() == 0 and _snapshot(clipped) == before  # the same call without a mistake goes through
    # a sector may close on itself once, also with an increment that was rounded to float32 on its way
    assert call(num_beams=361) == 0 and call(num_beams=361, angle_increment=float(F(inc))) == 0
    assert call(angle_min=2 * PI, num_beams=90) == 0 and call(occlusion_margin=inf) == 0 and call(range_max=0.05) == 0


def test_one_2d_frame_end_to_end_equals_the_oracle(product, oracle):
    """adapt (laser scan -> compact measurement) -> clip_scan of a map at a slightly wrong pose -> set_moving / set_fixed on device
    arrays -> point-to-plane alignment -> merge_from_aligner; the oracle runs the same frame on restatement-made inputs"""
    kind, beams = abi.SE2_RIGHT, 1000
    ang = np.deg2rad(np.linspace(-135.0, 135.0, beams))
    a0, inc = float(ang[0]), float(ang[1] - ang[0])
    X_gt = syn.se2(0.10, 0.05, np.deg2rad(3.0))          # where the robot is in the local map
    robot_in_map = syn.se2(0.08, 0.04, np.deg2rad(2.5)).astype(F)  # where the tracker believes it is
    scans = [np.linalg.norm(syn.scan_2d(pose, beams=beams)[0], axis=1).astype(F) for pose in (syn.se2(0, 0, 0), X_gt)]
    want = dict(range_min=0.05, range_max=30.0, half_window=1, max_distance_squared=0.01, drop_points_without_normal=True, compact=True)
    # the local map: the first scan and, 0.4 m behind every wall it saw, a second layer the scanner cannot see
    m0 = ar.adapt_laser_scan(scans[0], a0, inc, **want)
    order = np.random.default_rng(2).permutation(2 * len(m0["points"]))
    rho0 = np.linalg.norm(m0["points"].astype(np.float64), axis=1, keepdims=True)
    map_pts = np.concatenate([m0["points"], m0["points"] * (1.0 + 0.4 / rho0)])[order].astype(F)
    map_nrm = np.concatenate([m0["normals"], m0["normals"]])[order].astype(F)
    meas_r = ar.adapt_laser_scan(scans[1], a0, inc, **want)
    clip_r = cs.clip_scan(map_pts, robot_in_map, a0, inc, beams, 0.05, 30.0, occlusion_margin=0.1, normals=map_nrm)
    assert 0 < clip_r["num_kept"] < clip_r["num_in_view"] <= clip_r["num_valid"] == len(map_pts)
    assert clip_r["num_kept"] < 0.7 * len(map_pts)  # the hidden layer is (mostly) gone
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.5, robust=abi.ROBUST_CAUCHY)
    Lh = robot_in_map.astype(np.float64)

    def to_map(X):  # the measurement in the local map through the estimate: map <- robot (believed) <- robot (now)
        return (Lh @ np.linalg.inv(X.astype(np.float64))).astype(F)

    runs = {}
    for side in ("oracle", "gpu"):
        b = oracle.scene_binding() if side == "oracle" else product.scene_binding(0)
        scene, meas, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2), mapping.Scene(b, 2)
        scene.set(map_pts, map_nrm)
        al = oracle.OracleAligner(kind) if side == "oracle" else product.MultiAligner(kind, device=0)
        si = al.add_slice(cfg)
        if side == "oracle":
            meas.set(meas_r["points"], meas_r["normals"])
            gidx = clip_r["global_indices"]
            al.set_fixed(si, meas_r["points"], meas_r["normals"])
            al.set_moving(si, clip_r["points"], clip_r["normals"])
        else:
            p = adaptors.default_scan_params()
            p.angle_min, p.angle_increment, p.compact = a0, inc, 1
            ad = adaptors.MeasurementAdaptorLaserScan(p)
            ad.set_meas(meas); ad.set_raw_data(scans[1]); ad.compute(False)
            cl = _clipper(b, scene, clipped, beams, robot_in_map, None, 0.1, (0.05, 30.0), scanner=(a0, inc))
            res = cl.compute()
            _check(clipped, clip_r, res, "frame clip")
            cp, cn, n = clipped.device_arrays()
            mp, mn, m = meas.device_arrays()
            assert m == meas_r["num_valid"] and mn is not None and cn is not None
            al.set_cloud_device("set_moving", si, cp, 16, cn, 16, n, kept=True)
            al.set_cloud_device("set_fixed", si, mp, 16, mn, 16, m, kept=True)
        al.set_moving_in_fixed(syn.identity(2))
        al.compute()
        assert al.status() == abi.SUCCESS
        X = al.moving_in_fixed()
        mg = mapping.MergerCorrespondenceHomo(b)
        mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(to_map(X))
        if side == "gpu":
            out = mg.compute_from_aligner(al, si, clipped)
        else:
            c = al.correspondences(si)
            flipped = np.zeros(len(c), dtype=c.dtype)
            flipped["fixed_idx"], flipped["moving_idx"], flipped["response"] = gidx[c["moving_idx"]], c["fixed_idx"], c["response"]
            mg.set_correspondences(flipped)
            out = mg.compute()
        runs[side] = (X.copy(), out, scene.get(), al)
    (Xr, outr, (pr, nr), alr), (Xg, outg, (pg, ng), alg) = runs["oracle"], runs["gpu"]
    ncorr = alg.iteration_stats()[-1]["num_correspondences"]
    print("2-D frame: %d correspondences, merge %s" % (ncorr, outg))
    assert_same_run(alr, alg)  # status, every iteration's statistics, the estimate and the correspondences, bit for bit
    assert ncorr > 500 and Xr.tobytes() == Xg.tobytes()
    assert outr == outg and outg["num_merged"] > 100
    assert cs.same_bits(pr, pg) and cs.same_bits(nr, ng)
    # the estimate takes the believed pose to the true one, X = robot_now^-1 * robot_believed: closer to it than the start was
    X_true = np.linalg.inv(X_gt) @ Lh
    err, err0 = float(np.max(np.abs(Xg.astype(np.float64) - X_true))), float(np.max(np.abs(np.eye(3) - X_true)))
    print("2-D frame: max |X - X_true| = %.3g (at the start %.3g)" % (err, err0))
    assert err < err0
