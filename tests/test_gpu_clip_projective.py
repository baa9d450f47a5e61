"""GPU: srrg2_scene_clip_projective (csrc/scene.hip) against the numpy restatement of its contract
(tests/clip_projective_restatement.py), BIT FOR BIT: coordinates, normals, features, global indices and counts; refusals leave
`clipped` as it was; and through the stack: the aligner finds on the clipped cloud what it finds on the whole one, and a frame
adapt -> clip -> align -> merge equals the same frame on the oracle with restatement-made inputs."""
import ctypes as C

import numpy as np
import pytest

import adaptor_restatement as ar
import clip_projective_cases as cases
import clip_projective_restatement as cr
from helpers import projective_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
I34 = np.eye(3, 4, dtype=F)
E_INVALID, E_UNSUPPORTED = -1, -4


def _camera(rows, cols, cx=None, cy=None):
    f = 0.8 * max(cols, 4)
    return np.array([[f, 0, (cols - 1) / 2.0 if cx is None else cx], [0, f, (rows - 1) / 2.0 if cy is None else cy], [0, 0, 1.0]], F)


def _random_scene(n, seed, invalid=True, duplicates=True):
    """points around a camera looking along +z (some behind it, some beyond the depth range, exact duplicates for depth ties),
    unit normals, descriptors, intensities"""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-1.0, 10.0, n)], 1).astype(F)
    if duplicates and n >= 8:
        src = rng.integers(0, n, n // 8)
        pts[rng.integers(0, n, n // 8)] = pts[src]
    if invalid and n >= 4:
        bad = rng.integers(0, n, max(1, n // 50))
        pts[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    return pts, nrm, rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F)


def _pose(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return syn.se3(scale * rng.uniform(-0.3, 0.3, 3), scale * np.deg2rad(rng.uniform(-10, 10, 3))).astype(F)


def _fill(scene, pts, nrm=None, desc=None, inten=None):
    scene.set(pts, nrm)
    if desc is not None or inten is not None:
        scene.set_features(desc, inten)


def _clipper(b, full, clipped, K, rows, cols, pose=I34, sensor=None, margin=-1.0, depth=(0.4, 8.0)):
    cl = mapping.SceneClipperProjective(b)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    cl.set_camera_matrix(K)
    if sensor is not None:
        cl.set_sensor_in_robot(sensor)
    cl.params.image_rows, cl.params.image_cols = rows, cols
    cl.params.depth_min, cl.params.depth_max = depth
    cl.params.occlusion_margin = margin
    return cl


def _check(clipped, r, res, what):
    assert clipped.size() == r["num_kept"], what
    pts, nrm = clipped.get()
    assert cr.same_bits(pts, r["points"]), what
    _, nptr, _ = clipped.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and cr.same_bits(nrm, r["normals"]), what
    assert clipped.has_features() == (r["descriptors"] is not None, r["intensity"] is not None), what
    d, i = clipped.features()
    if r["descriptors"] is not None:
        assert np.array_equal(d, r["descriptors"]), what
    if r["intensity"] is not None:
        assert cr.same_bits(i, r["intensity"]), what
    assert np.array_equal(clipped.global_indices(), r["global_indices"]), what
    if res is not None:
        assert res == {k: r[k] for k in ("status", "num_valid", "num_in_view", "num_kept")}, (what, res)


def _snapshot(scene):
    pts, nrm = scene.get()
    d, i = scene.features()
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if d is None else d.tobytes(),
            None if i is None else i.tobytes(), scene.global_indices().tobytes())


MARGINS = (-1.0, 0.0, 0.05, 1.0, float("inf"))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 300_000])
def test_random_scenes_match_the_restatement(product, n):
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, desc, inten = _random_scene(n, 100 + n)
    rows, cols = (480, 640) if n > 1000 else (48, 64)
    K = _camera(rows, cols)
    kept = []
    for fi, feats in enumerate(((None, None, None), (nrm, None, None), (nrm, desc, None), (None, None, inten), (nrm, desc, inten))):
        _fill(full, pts, *feats)
        for mi, margin in enumerate(MARGINS):
            if n > 1000 and fi not in (0, 4) and mi not in (0, 1):
                continue  # (the large scene: every margin with and without everything, two margins in between)
            pose, sensor = _pose(7 * fi + mi), (None if mi % 2 else _pose(50 + mi, 0.5))
            cl = _clipper(b, full, clipped, K, rows, cols, pose, sensor, margin)
            res = cl.compute()
            assert cl.status() == (mapping.CLIPPER_SUCCESSFUL if n else mapping.CLIPPER_READY)
            r = cr.clip_projective(pts, pose, K, rows, cols, sensor_in_robot=sensor, occlusion_margin=margin, normals=feats[0],
                                   descriptors=feats[1], intensity=feats[2])
            _check(clipped, r, res, (n, fi, margin))
            kept.append((margin, r["num_kept"], r["num_in_view"], r["num_valid"]))
        # +inf is frustum-only mode
        a = _clipper(b, full, clipped, K, rows, cols, I34, None, float("inf")).compute()
        snap = _snapshot(clipped)
        assert a == _clipper(b, full, clipped, K, rows, cols, I34, None, -1.0).compute() and _snapshot(clipped) == snap
    if n >= 1000:  # not vacuous: occlusion removes points, invalid points exist, not everything is in view
        assert any(m == 0.0 and 0 < k < v < nv < n for m, k, v, nv in kept), kept


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (3, 3), (480, 640)])
def test_image_shapes_and_principal_point_outside(product, shape):
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, desc, inten = _random_scene(20_000, 9)
    pts[:, :2] *= F(0.02) if max(shape) < 10 else F(1.0)  # (tiny images: squeeze the cloud so that some of it is seen)
    _fill(full, pts, nrm, None, inten)
    rows, cols = shape
    seen = 0
    for K in (_camera(rows, cols), _camera(rows, cols, cx=-50.0), _camera(rows, cols, cx=cols + 20.0, cy=-3.0)):
        for margin in (-1.0, 0.0, 0.2):
            res = _clipper(b, full, clipped, K, rows, cols, _pose(3, 0.2), None, margin).compute()
            r = cr.clip_projective(pts, _pose(3, 0.2), K, rows, cols, occlusion_margin=margin, normals=nrm, intensity=inten)
            _check(clipped, r, res, (shape, K[0, 2], margin))
            seen += r["num_kept"]
    assert seen > 0


def test_result_pointer_may_be_null(product):
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, _, _ = _random_scene(5000, 21)
    _fill(full, pts, nrm)
    K = _camera(48, 64)
    cl = _clipper(b, full, clipped, K, 48, 64, margin=0.0)
    assert cl.compute(want_result=False) is None and cl.status() == mapping.CLIPPER_SUCCESSFUL
    _check(clipped, cr.clip_projective(pts, I34, K, 48, 64, occlusion_margin=0.0, normals=nrm), None, "out == NULL")


def test_reused_handle_follows_a_moving_pose(product):
    """the same `clipped` as the pose moves: the scatter runs behind the scan without the host knowing the total; then a clip whose
    total exceeds the room left from the call before (= the result on a fresh handle); then ball and projective clips in turn"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, desc, inten = _random_scene(300_000, 33)
    _fill(full, pts, nrm, desc, inten)
    rows, cols = 480, 640
    K = _camera(rows, cols)
    kw = dict(normals=nrm, descriptors=desc, intensity=inten)
    # a narrow depth range first: a small result, little room
    res = _clipper(b, full, clipped, K, rows, cols, depth=(0.4, 0.41)).compute()
    r = cr.clip_projective(pts, I34, K, rows, cols, 0.4, 0.41, **kw)
    _check(clipped, r, res, "narrow")
    small = r["num_kept"]
    assert 0 < small < 1000
    res = _clipper(b, full, clipped, K, rows, cols, margin=0.05).compute()
    r = cr.clip_projective(pts, I34, K, rows, cols, occlusion_margin=0.05, **kw)
    assert r["num_kept"] > 20 * max(small, 1024)  # beyond any room the small result left
    _check(clipped, r, res, "grown")
    fresh = mapping.Scene(b, 3)
    _clipper(b, full, fresh, K, rows, cols, margin=0.05).compute()
    assert _snapshot(fresh) == _snapshot(clipped)
    for k in range(6):  # the room is there now: every one of these takes the speculative scatter
        pose, margin = _pose(200 + k, 0.3 * k), (-1.0, 0.0, 0.05)[k % 3]
        res = _clipper(b, full, clipped, K, rows, cols, pose, margin=margin, depth=(0.4, 6.0)).compute()
        _check(clipped, cr.clip_projective(pts, pose, K, rows, cols, 0.4, 6.0, occlusion_margin=margin, **kw), res, ("moving", k))
    ball = mapping.SceneClipperBall(b, range_max=4.0)
    ball.set_full_scene(full); ball.set_clipped_scene_in_robot(clipped)
    for k in range(4):
        pose = _pose(300 + k)
        ball.set_robot_in_local_map(pose); ball.compute()
        with np.errstate(all="ignore"):
            q = cr.xform(cr.se3_inverse(pose), pts)
            inside = np.isfinite(pts).all(1) & ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2] <= F(4.0) * F(4.0))
        assert np.array_equal(clipped.global_indices(), np.flatnonzero(inside)) and cr.same_bits(clipped.get()[0], q[inside])
        res = _clipper(b, full, clipped, K, rows, cols, pose, margin=0.0).compute()
        _check(clipped, cr.clip_projective(pts, pose, K, rows, cols, occlusion_margin=0.0, **kw), res, ("alternating", k))


def test_coordinates_are_clip_balls(product):
    b = product.scene_binding(0)
    full, by_ball, by_camera = mapping.Scene(b, 3), mapping.Scene(b, 3), mapping.Scene(b, 3)
    pts, nrm, _, _ = _random_scene(50_000, 44)
    _fill(full, pts, nrm)
    pose = _pose(5)
    ball = mapping.SceneClipperBall(b, range_max=1000.0)
    ball.set_full_scene(full); ball.set_clipped_scene_in_robot(by_ball); ball.set_robot_in_local_map(pose); ball.compute()
    _clipper(b, full, by_camera, _camera(48, 64), 48, 64, pose, _pose(6, 0.5), 0.1).compute()
    gb, gc = by_ball.global_indices(), by_camera.global_indices()
    assert len(gc) > 1000 and np.all(np.isin(gc, gb))
    at = np.searchsorted(gb, gc)
    for k in (0, 1):  # coordinates, normals
        assert by_ball.get()[k][at].tobytes() == by_camera.get()[k].tobytes()


def test_refusals_leave_clipped_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    b = product.scene_binding(0)
    full, clipped, s2a, s2b = mapping.Scene(b, 3), mapping.Scene(b, 3), mapping.Scene(b, 2), mapping.Scene(b, 2)
    pts, nrm, desc, inten = _random_scene(3000, 55)
    _fill(full, pts, nrm, desc, inten)
    K = _camera(48, 64)
    _clipper(b, full, clipped, K, 48, 64, margin=0.0).compute()
    s2a.set(pts[:100, :2]); s2b.set(pts[:50, :2])
    before, before2 = _snapshot(clipped), _snapshot(s2b)
    assert before[0] > 100
    pose = np.ascontiguousarray(I34)
    pp = pose.ctypes.data_as(C.POINTER(C.c_float))
    fn = lib.srrg2_scene_clip_projective
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(mapping.ProjectiveClipParams), C.c_void_p,
                   C.POINTER(mapping.ClipResult)]

    def call(f=full, c=clipped, T=pp, params=True, **edit):
        p = mapping.default_projective_clip_params()
        for i, v in enumerate(K.reshape(9)):
            p.camera_matrix[i] = float(v)
        p.image_rows, p.image_cols, p.occlusion_margin = 48, 64, 0.0
        for k, v in edit.items():
            if k.startswith("K"):
                p.camera_matrix[int(k[1:])] = v
            else:
                setattr(p, k, v)
        out = mapping.ClipResult()
        return fn(f._h, T, C.byref(p) if params else None, c._h, C.byref(out))

    none = mapping.Scene.__new__(mapping.Scene)
    none._h = None
    invalid = [dict(f=none), dict(c=none), dict(T=None), dict(params=False), dict(c=full), dict(c=s2b), dict(f=s2a),
               dict(image_rows=0), dict(image_cols=0), dict(image_rows=-3), dict(image_rows=70000, image_cols=70000),
               dict(depth_min=0.0), dict(depth_min=-1.0), dict(depth_min=float("nan")), dict(depth_max=0.3),
               dict(depth_max=float("nan")), dict(K0=0.0), dict(K4=0.0), dict(K0=float("inf")), dict(K4=float("nan")),
               dict(occlusion_margin=float("nan"))]
    for kw in invalid:
        assert call(**kw) == E_INVALID, kw
        assert b.err()  # (the error text is set)
    assert call(K1=0.5) == E_UNSUPPORTED
    assert call(f=s2a, c=s2b) == E_UNSUPPORTED  # 2-D scenes
    assert _snapshot(clipped) == before and _snapshot(s2b) == before2
    if torch_devices() > 1:
        other = mapping.Scene(product.scene_binding(1), 3)
        assert call(c=other) == E_INVALID
    assert call() == 0 and _snapshot(clipped) == before  # the same call without a mistake goes through


def torch_devices():
    from srrg2_slam_interfaces_amd import _capi

    return _capi.device_count()


@pytest.mark.parametrize("sensor", [None, cases.SENSOR_IN_ROBOT], ids=["identity", "sensor_in_robot"])
def test_clipped_cloud_gives_the_aligner_the_same_correspondences(product, oracle, sensor):
    d = cases.c3_layers(sensor_in_robot=sensor)
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    _fill(full, d["map"], d["map_normals"])
    cl = _clipper(b, full, clipped, d["K"], d["rows"], d["cols"], I34, sensor, 0.0, (d["depth_min"], d["depth_max"]))
    res = cl.compute()
    assert 0 < res["num_kept"] < res["num_in_view"] < res["num_valid"]
    pts, nrm = clipped.get()
    make = lambda: product.MultiAligner(cases.KIND, device=0)
    c_full = cases.first_association(make, d, d["map"], d["map_normals"], sensor)
    c_clip = cases.first_association(make, d, pts, nrm, sensor)
    assert len(c_full) > 5000
    cases.assert_same_association(c_clip, cl.global_indices(), c_full)
    # ... and they are the oracle's on the whole cloud
    c_ref = cases.first_association(oracle.OracleAligner, d, d["map"], d["map_normals"], sensor)
    cases.assert_same_association(c_clip, cl.global_indices(), c_ref)


def test_one_frame_end_to_end_equals_the_oracle(product, oracle):
    """adapt (depth image -> organised measurement) -> clip_projective -> set_moving / set_fixed on device arrays -> projective
    point-to-plane next to a reprojection slice -> merge_from_aligner; the oracle runs the same frame on restatement-made inputs"""
    rows, cols = 120, 160
    d = cases.c3_layers(rows, cols, sensor_in_robot=cases.SENSOR_IN_ROBOT)
    S = cases.SENSOR_IN_ROBOT
    depth = np.ascontiguousarray(d["fixed"][:, 2].reshape(rows, cols), F)  # NaN = no reading
    robot_in_map = _pose(77, 0.2)
    Lh = np.vstack([robot_in_map.astype(np.float64), [0, 0, 0, 1]])
    map_pts = np.ascontiguousarray(d["map"].astype(np.float64) @ Lh[:3, :3].T + Lh[:3, 3], F)  # the local map's own frame
    map_nrm = np.ascontiguousarray(d["map_normals"].astype(np.float64) @ Lh[:3, :3].T, F)
    want = dict(depth_scale=0.001, depth_min=d["depth_min"], depth_max=d["depth_max"], col_gap=1, row_gap=1,
                max_distance_squared=0.0625, drop_points_without_normal=True, compact=False)
    meas_r = ar.adapt_depth_image(depth, d["K"], **want)
    clip_r = cr.clip_projective(map_pts, robot_in_map, d["K"], rows, cols, d["depth_min"], d["depth_max"], sensor_in_robot=S,
                                occlusion_margin=0.02, normals=map_nrm)
    assert 0 < clip_r["num_kept"] < clip_r["num_in_view"] < clip_r["num_valid"]
    cfgs = [projective_config(cases.KIND, kind, d, gate=0.05) for kind in (abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION)]

    def to_map(X):  # measurement (sensor frame) in the local map, through the estimate: map <- robot(prev) <- robot(now) <- sensor
        Xh = np.vstack([X.astype(np.float64), [0, 0, 0, 1]])
        Sh = np.vstack([S.astype(np.float64), [0, 0, 0, 1]])
        return (Lh @ np.linalg.inv(Xh) @ Sh)[:3].astype(F)

    runs = {}
    for side in ("oracle", "gpu"):
        b = oracle.scene_binding() if side == "oracle" else product.scene_binding(0)
        scene, meas, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3), mapping.Scene(b, 3)
        scene.set(map_pts, map_nrm)
        al = oracle.OracleAligner(cases.KIND) if side == "oracle" else product.MultiAligner(cases.KIND, device=0)
        sis = [al.add_slice(c) for c in cfgs]
        for si in sis:
            al.set_sensor_in_robot(si, S)
        if side == "oracle":
            meas.set(meas_r["points"], meas_r["normals"])
            gidx = clip_r["global_indices"]
            for si in sis:
                al.set_fixed(si, meas_r["points"], meas_r["normals"])
                al.set_moving(si, clip_r["points"], clip_r["normals"])
        else:
            p = adaptors.default_depth_params()
            for i, v in enumerate(d["K"].reshape(9)):
                p.camera_matrix[i] = float(v)
            p.depth_min, p.depth_max = d["depth_min"], d["depth_max"]
            ad = adaptors.MeasurementAdaptorDepthImage(p)
            ad.set_meas(meas); ad.set_raw_data(depth); ad.compute(False)
            cl = _clipper(b, scene, clipped, d["K"], rows, cols, robot_in_map, S, 0.02, (d["depth_min"], d["depth_max"]))
            res = cl.compute()
            _check(clipped, clip_r, res, "frame clip")
            cp, cn, n = clipped.device_arrays()
            mp, mn, m = meas.device_arrays()
            assert m == rows * cols and mn is not None and cn is not None
            for si in sis:
                al.set_cloud_device("set_moving", si, cp, 16, cn, 16, n, kept=True)
                al.set_cloud_device("set_fixed", si, mp, 16, mn, 16, m, kept=True)
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()
        assert al.status() == abi.SUCCESS
        X = al.moving_in_fixed()
        mg = mapping.MergerCorrespondenceHomo(b)
        mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(to_map(X))
        if side == "gpu":
            out = mg.compute_from_aligner(al, sis[0], clipped)
        else:
            c = al.correspondences(sis[0])
            flipped = np.zeros(len(c), dtype=c.dtype)
            flipped["fixed_idx"], flipped["moving_idx"], flipped["response"] = gidx[c["moving_idx"]], c["fixed_idx"], c["response"]
            mg.set_correspondences(flipped)
            out = mg.compute()
        runs[side] = (X.copy(), out, scene.get(), al.iteration_stats()[-1]["num_correspondences"])
    (Xr, outr, (pr, nr), ncr), (Xg, outg, (pg, ng), ncg) = runs["oracle"], runs["gpu"]
    print("frame: %d correspondences, merge %s" % (ncg, outg))
    assert ncr == ncg > 5000 and Xr.tobytes() == Xg.tobytes()
    assert outr == outg and outg["num_merged"] > 1000
    assert cr.same_bits(pr, pg) and cr.same_bits(nr, ng)
