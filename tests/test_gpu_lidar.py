"""GPU: srrg2_adapt_lidar_sweep (csrc/adaptor.hip) and srrg2_scene_clip_spherical (csrc/scene.hip) against the numpy restatement
of their contract (tests/lidar_restatement.py), BIT FOR BIT: coordinates, normals, intensities, global indices and counts;
refusals leave the target as it was; and through the stack: adapt -> clip -> align equals the oracle's alignment of the
restatement-made clouds."""
import ctypes as C
import math

import numpy as np
import pytest

import lidar_cases as lc
import lidar_restatement as lr
from helpers import assert_same_run, cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
I34 = np.eye(3, 4, dtype=F)
E_INVALID, E_UNSUPPORTED = -1, -4


def _set_model(dst, m):
    dst.azimuth_min, dst.azimuth_increment = float(m.azimuth_min), float(m.azimuth_increment)
    dst.elevation_min, dst.elevation_increment = float(m.elevation_min), float(m.elevation_increment)
    dst.rows, dst.cols, dst.range_min, dst.range_max = m.rows, m.cols, float(m.range_min), float(m.range_max)


def _lidar_params(m, want):
    p = adaptors.default_lidar_params()
    _set_model(p.model, m)
    p.normal_col_gap, p.normal_row_gap = want["col_gap"], want["row_gap"]
    p.normal_max_distance_squared = want["max_distance_squared"]
    p.drop_points_without_normal = int(want["drop_points_without_normal"])
    p.compact = int(want["compact"])
    return p


def _adapt(scene, points, m, intensity=None, layout="separate", device=False, want_result=True, **kw):
    """-> (restated, result of compute(), what must stay alive).  layout: 'separate' arrays or interleaved 'xyzi' records"""
    want = dict(col_gap=1, row_gap=1, max_distance_squared=1.0, drop_points_without_normal=True, compact=False)
    want.update(kw)
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    ad = adaptors.MeasurementAdaptorLidarSweep(_lidar_params(m, want))
    ad.set_meas(scene)
    keep = []
    xyzi = None if intensity is None or layout != "xyzi" else np.concatenate([points, np.asarray(intensity, F)[:, None]], axis=1)
    if device:
        import torch

        n = len(points)
        t = torch.from_numpy(np.ascontiguousarray(points if xyzi is None else xyzi)).cuda()
        keep.append(t)
        ipair = None
        if xyzi is not None:
            ipair = (t.data_ptr() + 12, 16)
        elif intensity is not None:
            ti = torch.from_numpy(np.ascontiguousarray(intensity, F)).cuda()
            keep.append(ti)
            ipair = (ti.data_ptr(), 4)
        torch.cuda.synchronize()
        ad.set_raw_data((t.data_ptr() if n else 0, 12 if xyzi is None else 16, n), ipair)
    elif xyzi is not None:
        ad.set_raw_data(xyzi)
    else:
        ad.set_raw_data(points, intensity)
    assert ad.status() == abi.ADAPTOR_ERROR  # not computed yet
    res = ad.compute(want_result)
    if want_result:
        assert ad.status() == (abi.ADAPTOR_READY if len(points) else abi.ADAPTOR_INITIALIZING)
    return lr.adapt_lidar_sweep(points, m, intensity=intensity, **want), res, keep


def _check_scene(scene, r, res, what):
    n = r["points"].shape[0]
    assert scene.size() == n == r["scene_size"], what
    pts, nrm = scene.get()
    assert lr.same_bits(pts, r["points"]), what
    _, nptr, _ = scene.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and lr.same_bits(nrm, r["normals"]), what
    hd, hi = scene.has_features()
    assert not hd and hi == (r["intensity"] is not None), what
    if hi:
        assert lr.same_bits(scene.features()[1], r["intensity"]), what
    g = scene.global_indices()
    assert np.array_equal(g, r["global_indices"] if r["global_indices"] is not None else np.zeros(0, np.int32)), what
    if res is not None:
        assert res == {k: r[k] for k in ("status", "num_raw", "num_in_range", "num_valid", "scene_size")}, (what, res)


# ---- adaptor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("compact", [False, True], ids=["organised", "compact"])
def test_main_case_matches_the_restatement(product, compact, device):
    a = lc.main_case()
    scene = mapping.Scene(product.scene_binding(0), 3)
    for gaps in (1, 0):
        for drop in (False, True):
            for inten, layout in ((None, "separate"), (a["intensity"], "separate"), (a["intensity"], "xyzi")):
                r, res, _ = _adapt(scene, a["points"], a["model"], inten, layout, device, compact=compact, col_gap=gaps, row_gap=gaps,
                                   drop_points_without_normal=drop)
                _check_scene(scene, r, res, (gaps, drop, layout, inten is not None))
                assert 0 < r["num_valid"] <= r["num_in_range"] < r["num_raw"]


def test_edge_inputs_match_the_restatement(product):
    scene = mapping.Scene(product.scene_binding(0), 3)
    for name, m, pts, kw in lc.edge_cases():
        inten = np.arange(len(pts), dtype=F) + F(0.5)
        for compact in (False, True):
            for drop in (False, True):
                r, res, _ = _adapt(scene, pts, m, inten, "xyzi" if compact else "separate", device=drop, compact=compact,
                                   drop_points_without_normal=drop, **kw)
                _check_scene(scene, r, res, (name, compact, drop))


def test_empty_sweep_and_reuse_of_the_scene(product):
    a = lc.main_case()
    scene = mapping.Scene(product.scene_binding(0), 3)
    for compact in (False, True):
        r, res, _ = _adapt(scene, a["points"], a["model"], a["intensity"], compact=compact)
        _check_scene(scene, r, res, "full")
        for inten in (None, np.zeros(0, F)):
            r, res, _ = _adapt(scene, np.zeros((0, 3), F), a["model"], inten, compact=compact)
            assert res["status"] == abi.ADAPTOR_INITIALIZING and res["num_raw"] == 0 and scene.size() == 0
            _check_scene(scene, r, res, "empty")
    # a smaller image after a larger one, and back: nothing of the earlier winners shows through
    m = lr.Model.full_turn(4, 8, -0.3, 0.3)
    r, res, _ = _adapt(scene, lc.full_image(m)[::3], m, max_distance_squared=100.0)
    _check_scene(scene, r, res, "small after large")
    r, res, _ = _adapt(scene, a["points"], a["model"], compact=True)
    _check_scene(scene, r, res, "large after small")


@pytest.mark.parametrize("compact", [False, True], ids=["organised", "compact"])
def test_past_the_launch_cap(product, compact):
    """140 000 input points into a 66 x 2048 image: more points and more pixels than 512 workgroups of 256 threads cover in one
    stride of the bin, the organised and the flag / scatter kernels"""
    rows, cols, n = 66, 2048, 140_000
    rng = np.random.default_rng(66)
    m = lr.Model.full_turn(rows, cols, math.radians(-25), math.radians(15))
    assert n > 512 * 256 and rows * cols > 512 * 256
    az = rng.uniform(-math.pi, math.pi, n)
    el = rng.uniform(math.radians(-27), math.radians(17), n)
    rho = 6.0 + 2.0 * np.sin(3 * az) + rng.normal(0, 0.01, n)
    pts = np.stack([rho * np.cos(el) * np.cos(az), rho * np.cos(el) * np.sin(az), rho * np.sin(el)], axis=1).astype(F)
    pts[rng.integers(0, n, 200)] = np.nan
    pts[rng.integers(0, n, 2000)] = pts[rng.integers(0, n, 2000)]  # exact duplicates: ties between distant indices
    inten = rng.random(n, dtype=F)
    scene = mapping.Scene(product.scene_binding(0), 3)
    r, res, _ = _adapt(scene, pts, m, inten, "xyzi", device=compact, compact=compact, max_distance_squared=4.0)
    _check_scene(scene, r, res, "large")
    assert r["num_valid"] > 10_000 and (r["candidates"] > 1).sum() > 10_000 and r["occupied"][-cols:].any()


def test_queued_organised_adapt_feeds_the_aligner(product):
    """organised mode without a result only queues its work: device arrays + set_fixed(..., SRRG2_MEM_DEVICE_KEPT) follow at once
    and the run equals the one fed the restatement's arrays from the host"""
    kind = abi.SE3_QUAT_RIGHT
    a, b = lc.main_case(), lc.second_sweep()
    scene = mapping.Scene(product.scene_binding(0), 3)
    moving = lr.adapt_lidar_sweep(b["points"], b["model"], compact=True)
    runs = []
    for from_scene in (False, True):
        al = product.MultiAligner(kind, device=0)
        si = al.add_slice(cue_config(kind, abi.SLICE_P2PLANE, lc.GATE, robust=abi.ROBUST_CAUCHY))
        if from_scene:
            r, res, keep = _adapt(scene, a["points"], a["model"], device=True, want_result=False)
            assert res is None
            cp, cn, n = scene.device_arrays()
            assert n == a["model"].rows * a["model"].cols and cn is not None
            al.set_cloud_device("set_fixed", si, cp, 16, cn, 16, n, kept=True)
        else:
            r = lr.adapt_lidar_sweep(a["points"], a["model"])
            al.set_fixed(si, r["points"], r["normals"])
        al.set_moving(si, moving["points"], moving["normals"])
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()
        runs.append(al)
    assert runs[0].status() == abi.SUCCESS
    assert_same_run(runs[0], runs[1])
    _check_scene(scene, r, None, "after the run")


def _snapshot(scene):
    pts, nrm = scene.get()
    d, i = scene.features()
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if d is None else d.tobytes(),
            None if i is None else i.tobytes(), scene.global_indices().tobytes())


BAD_MODELS = [dict(rows=0), dict(cols=-1), dict(rows=70000, cols=70000), dict(azimuth_increment=0.0),
              dict(azimuth_increment=float("inf")), dict(elevation_increment=0.0), dict(elevation_increment=float("nan")),
              dict(azimuth_min=float("nan")), dict(azimuth_min=7.0), dict(azimuth_increment=2 * math.pi / 300),
              dict(elevation_min=float("inf")), dict(elevation_min=-1.7), dict(elevation_increment=0.2), dict(range_min=0.0),
              dict(range_min=float("nan")), dict(range_max=0.4), dict(range_max=float("nan"))]


def test_adaptor_refusals_leave_the_scene_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    a = lc.main_case()
    b = product.scene_binding(0)
    s3, s2 = mapping.Scene(b, 3), mapping.Scene(b, 2)
    _adapt(s3, a["points"], a["model"], a["intensity"], compact=True)
    before = _snapshot(s3)
    xyzi = np.concatenate([a["points"], a["intensity"][:, None]], axis=1)
    pp, n = C.c_void_p(xyzi.ctypes.data), len(xyzi)

    def call(scene=s3, ptr=pp, st=16, iptr=C.c_void_p(xyzi.ctypes.data + 12), ist=16, n=n, mem=abi.MEM_HOST, params=True, **kw):
        p = _lidar_params(a["model"], dict(col_gap=1, row_gap=1, max_distance_squared=1.0, drop_points_without_normal=True,
                                           compact=True))
        for k, v in kw.items():
            setattr(p.model if hasattr(p.model, k) else p, k, v)
        return lib.srrg2_adapt_lidar_sweep(scene._h, ptr, st, iptr, ist, n, mem, C.byref(p) if params else None, None)

    bad = [dict(scene=s2), dict(params=False), dict(ptr=None), dict(n=-1), dict(st=8), dict(st=14), dict(ist=2), dict(ist=6),
           dict(ptr=C.c_void_p(xyzi.ctypes.data + 2)), dict(iptr=C.c_void_p(xyzi.ctypes.data + 13)), dict(mem=abi.MEM_DEVICE_KEPT),
           dict(mem=7), dict(normal_col_gap=-1), dict(normal_row_gap=-2), dict(normal_col_gap=0), dict(normal_row_gap=0),
           dict(reserved=1)] + BAD_MODELS
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"adapt_lidar_sweep" in b.err()
        assert _snapshot(s3) == before, kw
    assert call() == 0 and _snapshot(s3) == before  # the same call without the mistake goes through, to the same scene


# ---- clipper ---------------------------------------------------------------------------------------------------------------
def _fill(scene, pts, nrm=None, desc=None, inten=None):
    scene.set(pts, nrm)
    if desc is not None or inten is not None:
        scene.set_features(desc, inten)


def _clipper(b, full, clipped, m, pose=I34, sensor=None, margin=-1.0):
    cl = mapping.SceneClipperSpherical(b)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    if sensor is not None:
        cl.set_sensor_in_robot(sensor)
    _set_model(cl.params.model, m)
    cl.params.occlusion_margin = margin
    return cl


def _check_clip(clipped, r, res, what):
    assert clipped.size() == r["num_kept"], what
    pts, nrm = clipped.get()
    assert lr.same_bits(pts, r["points"]), what
    _, nptr, _ = clipped.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and lr.same_bits(nrm, r["normals"]), what
    assert clipped.has_features() == (r["descriptors"] is not None, r["intensity"] is not None), what
    d, i = clipped.features()
    if r["descriptors"] is not None:
        assert np.array_equal(d, r["descriptors"]), what
    if r["intensity"] is not None:
        assert lr.same_bits(i, r["intensity"]), what
    assert np.array_equal(clipped.global_indices(), r["global_indices"]), what
    if res is not None:
        assert res == {k: r[k] for k in ("status", "num_valid", "num_in_view", "num_kept")}, (what, res)


MARGINS = (-1.0, 0.0, 0.1, float("inf"))


def test_clip_of_the_room_matches_the_restatement(product):
    """the occlusion case: a non-identity robot pose and sensor mount, every margin, with and without normals and features; the
    kept points are what clip_ball writes for them"""
    o = lc.occlusion_case()
    b = product.scene_binding(0)
    full, clipped, ball = mapping.Scene(b, 3), mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, m, L, S = o["points"].copy(), o["model"], o["robot_in_local_map"], o["sensor_in_robot"]
    pts[::97, 1] = np.nan  # a map has invalid points
    pts[5::101] = pts[4::101][:len(pts[5::101])]  # ... and exact duplicates: ties for a pixel's minimum
    desc = np.random.default_rng(3).integers(0, 256, (len(pts), 32), dtype=np.uint8)
    kept = {}
    for feats in ((None, None, None), (o["normals"], None, None), (None, None, o["intensity"]), (o["normals"], desc, o["intensity"])):
        _fill(full, pts, *feats)
        for margin in MARGINS:
            for pose, sensor in ((L, S), (I34, None)):
                cl = _clipper(b, full, clipped, m, pose, sensor, margin)
                res = cl.compute()
                assert cl.status() == mapping.CLIPPER_SUCCESSFUL
                r = lr.clip_spherical(pts, pose, m, sensor, margin, normals=feats[0], descriptors=feats[1], intensity=feats[2])
                _check_clip(clipped, r, res, (margin, sensor is not None))
                kept[(margin, sensor is not None)] = r
    fov, zero, tenth, inf = (kept[(mg, True)] for mg in MARGINS)
    assert 0 < zero["num_kept"] < tenth["num_kept"] < fov["num_kept"] == fov["num_in_view"] < fov["num_valid"] < len(pts)
    assert np.array_equal(inf["global_indices"], fov["global_indices"])
    # clipped == clip_ball's output on the kept indices (normals and features included)
    _fill(full, pts, o["normals"], desc, o["intensity"])
    cb = mapping.SceneClipperBall(b, range_max=1.0e3)
    cb.set_full_scene(full); cb.set_clipped_scene_in_robot(ball); cb.set_robot_in_local_map(L)
    cb.compute()
    _clipper(b, full, clipped, m, L, S, 0.1).compute()
    where = np.searchsorted(ball.global_indices(), clipped.global_indices())
    assert np.array_equal(ball.global_indices()[where], clipped.global_indices())
    for got, ref in zip(clipped.get() + clipped.features(), ball.get() + ball.features()):
        assert got.tobytes() == ref[where].tobytes()


def test_clip_with_a_sector_camera_across_pi_and_odd_models(product):
    """a sector that crosses +-pi, a clockwise sensor with rows from the top, one pixel; nothing kept; an empty full"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    rng = np.random.default_rng(21)
    pts = rng.uniform(-6, 6, (3000, 3)).astype(F)
    pts[:, 2] *= F(0.3)
    pts[::50] = pts[1::50]
    nrm = rng.normal(size=pts.shape).astype(F)
    ft = lr.Model.full_turn(8, 64, -0.4, 0.4)
    models = {"sector": lr.Model(math.pi - 0.6, 0.05, -0.3, 0.1, 7, 25, range_min=0.5, range_max=7.0),
              "clockwise": lr.Model(-ft.azimuth_min, -ft.azimuth_increment, 0.4, -0.8 / 7, 8, 64, range_min=1.0, range_max=6.0),
              "one pixel": lr.Model(0.3, 0.5, 0.0, 0.4, 1, 1)}
    pose, sensor = lc.pose(0.4, -0.2, 0.1, yaw_deg=25.0), lc.pose(0.1, 0.05, 0.3, yaw_deg=-170.0, pitch_deg=3.0)
    _fill(full, pts, nrm)
    for name, m in models.items():
        assert m.valid(), name
        for margin in MARGINS:
            res = _clipper(b, full, clipped, m, pose, sensor, margin).compute()
            r = lr.clip_spherical(pts, pose, m, sensor, margin, normals=nrm)
            _check_clip(clipped, r, res, (name, margin))
            assert 0 < r["num_kept"] < len(pts), (name, margin)
        seam = lr.clip_spherical(pts, pose, m, sensor, -1.0)
        if name == "sector":  # both sides of the seam are in view
            az = np.arctan2(*(lr.xform(lr.se3_inverse(sensor), lr.xform(lr.se3_inverse(pose), pts))[seam["global_indices"]][:, [1, 0]].T))
            assert (az > 3.0).any() and (az < -3.0).any()
    # nothing kept: Successful, an empty scene that still shows the normals' presence
    far = lr.Model(ft.azimuth_min, ft.azimuth_increment, -0.4, 0.8 / 7, 8, 64, range_min=50.0, range_max=60.0)
    cl = _clipper(b, full, clipped, far, pose, sensor, 0.0)
    res = cl.compute()
    _check_clip(clipped, lr.clip_spherical(pts, pose, far, sensor, 0.0, normals=nrm), res, "nothing kept")
    assert res["num_kept"] == 0 and res["num_in_view"] == 0 and cl.status() == mapping.CLIPPER_SUCCESSFUL
    # an empty full: Ready
    _fill(full, np.zeros((0, 3), F))
    cl = _clipper(b, full, clipped, ft, pose, sensor, 0.0)
    res = cl.compute()
    assert cl.status() == mapping.CLIPPER_READY and res == dict(status=mapping.CLIPPER_READY, num_valid=0, num_in_view=0, num_kept=0)
    assert clipped.size() == 0


@pytest.mark.parametrize("n,margins", [(300_000, (-1.0, 0.0, 0.25)), (540_000, (0.1,))])
def test_clip_of_large_maps(product, n, margins):
    """300 000 points, and 540 000: blocks_for stops at 2048 x 256 = 524 288 threads, so past that every kernel of the clip strides"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    rng = np.random.default_rng(n)
    pts = rng.uniform(-15, 15, (n, 3)).astype(F)
    pts[:, 2] *= F(0.2)
    pts[rng.integers(0, n, n // 10)] = pts[rng.integers(0, n, n // 10)]
    pts[rng.integers(0, n, 500), rng.integers(0, 3, 500)] = np.inf
    nrm, inten = rng.normal(size=pts.shape).astype(F), rng.random(n, dtype=F)
    m = lr.Model.full_turn(32, 1024, math.radians(-20), math.radians(20), range_max=18.0)
    pose, sensor = lc.pose(1.0, -2.0, 0.3, yaw_deg=70.0), lc.pose(0.2, 0.0, 0.5, pitch_deg=-2.0)
    _fill(full, pts, nrm, None, inten)
    for margin in margins:
        res = _clipper(b, full, clipped, m, pose, sensor, margin).compute()
        r = lr.clip_spherical(pts, pose, m, sensor, margin, normals=nrm, intensity=inten)
        _check_clip(clipped, r, res, margin)
        assert 10_000 < r["num_kept"] <= r["num_in_view"] < r["num_valid"] < n
    assert r["num_kept"] < r["num_in_view"] and r["global_indices"][-1] > n - 1000


def test_clipper_refusals_leave_clipped_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    o = lc.occlusion_case()
    b = product.scene_binding(0)
    full, clipped, other = mapping.Scene(b, 3), mapping.Scene(b, 3), mapping.Scene(b, 3)
    f2, c2 = mapping.Scene(b, 2), mapping.Scene(b, 2)
    _fill(full, o["points"], o["normals"], None, o["intensity"])
    f2.set(o["points"][:100, :2].copy())
    _clipper(b, full, clipped, o["model"], o["robot_in_local_map"], o["sensor_in_robot"], 0.1).compute()
    before = _snapshot(clipped)
    assert before[0] > 0
    pose = np.ascontiguousarray(o["robot_in_local_map"], F)
    fp = pose.ctypes.data_as(C.POINTER(C.c_float))

    def call(f=full, c=clipped, pose=fp, params=True, **kw):
        p = mapping.default_spherical_clip_params()
        _set_model(p.model, o["model"])
        p.occlusion_margin = 0.1
        for i, v in enumerate(o["sensor_in_robot"].reshape(12)):
            p.sensor_in_robot[i] = float(v)
        for k, v in kw.items():
            setattr(p.model if hasattr(p.model, k) else p, k, v)
        return lib.srrg2_scene_clip_spherical(f._h if f else None, pose, C.byref(p) if params else None, c._h if c else None, None)

    bad = [dict(f=None), dict(c=None), dict(pose=None), dict(params=False), dict(f=clipped), dict(c=c2), dict(f=f2),
           dict(occlusion_margin=float("nan")), dict(reserved=3)] + BAD_MODELS
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"scene_clip_spherical" in b.err()
        assert _snapshot(clipped) == before, kw
    assert call(f=f2, c=c2) == E_UNSUPPORTED and b"srrg2_scene_clip_scan" in b.err()  # 2-D scenes have their own clipper
    assert lib.srrg2_scene_clip_scan(full._h, fp, C.byref(mapping.default_scan_clip_params()), other._h, None) == E_UNSUPPORTED
    assert call() == 0 and _snapshot(clipped) == before


# ---- through the stack -----------------------------------------------------------------------------------------------------
def test_adapt_clip_align_through_the_stack(product, oracle):
    """two sweeps of the room 5 cm and 1 degree apart: adapt both (compact), clip a map built from the first to the lidar's view,
    align the clipped map against the second from the device arrays -- bit for bit the oracle's alignment of the
    restatement-made clouds, and nearer the true relative pose than the identity guess"""
    kind = abi.SE3_QUAT_RIGHT
    s = lc.stack_case()
    b = product.scene_binding(0)
    meas_a, meas_b, full, clipped = (mapping.Scene(b, 3) for _ in range(4))
    for scene, sweep, want in ((meas_a, s["a"], s["meas_a"]), (meas_b, s["b"], s["meas_b"])):
        r, res, _ = _adapt(scene, sweep["points"], sweep["model"], compact=True)
        _check_scene(scene, r, res, "adapt")
        assert lr.same_bits(r["points"], want["points"])
    pts_a, nrm_a = meas_a.get()
    hidden = len(s["map_points"]) - len(pts_a)
    full.set(np.concatenate([pts_a, s["map_points"][-hidden:]]), np.concatenate([nrm_a, s["map_normals"][-hidden:]]))
    res = _clipper(b, full, clipped, s["a"]["model"], I34, None, 0.1).compute()
    _check_clip(clipped, s["clipped"], res, "clip")
    assert res["num_kept"] < res["num_in_view"] == len(s["map_points"])  # the wall next door is in the field of view, and hidden
    al = product.MultiAligner(kind, device=0)
    si = al.add_slice(cue_config(kind, abi.SLICE_P2PLANE, lc.GATE, robust=abi.ROBUST_CAUCHY))
    fp, fn, nf = meas_b.device_arrays()
    mp, mn, nm = clipped.device_arrays()
    al.set_cloud_device("set_fixed", si, fp, 16, fn, 16, nf)
    al.set_cloud_device("set_moving", si, mp, 16, mn, 16, nm)
    al.set_moving_in_fixed(syn.identity(3))
    al.compute()
    ref = lc.stack_oracle_run(oracle, s["meas_b"]["points"], s["meas_b"]["normals"], s["clipped"]["points"], s["clipped"]["normals"])
    assert ref.status() == abi.SUCCESS
    assert_same_run(ref, al)
    X, truth = al.moving_in_fixed().astype(np.float64), s["true_b_from_a"]
    err, guess = np.abs(X - truth).max(), np.abs(np.eye(3, 4) - truth).max()
    print("lidar frame: max |X - X_true| = %.3g (identity guess: %.3g), %d correspondences"
          % (err, guess, al.iteration_stats()[-1]["num_correspondences"]))
    assert err < guess
