"""GPU: the measurement adaptors (srrg2_adapt_depth_image / srrg2_adapt_laser_scan, csrc/adaptor.hip) against the numpy
restatement of their contract (tests/adaptor_restatement.py), BIT FOR BIT: coordinates, normals, intensities, global indices
and counts; misuse leaves the scene as it was; and through the stack: an aligner fed from the adapted scene's device arrays
runs exactly as one fed the restatement's arrays from the host, and a tracker frame runs on an adapted measurement."""
import ctypes as C

import numpy as np
import pytest

import adaptor_restatement as ar
from helpers import assert_same_run, cue_config, projective_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32


def _rgbd_depth():
    d = syn.rgbd_pair()
    z = np.ascontiguousarray(d["fixed"][:, 2].reshape(d["rows"], d["cols"]), F)
    mm = np.where(np.isfinite(z), np.rint(z.astype(np.float64) * 1000.0), 0).astype(np.uint16)
    return d, z, mm


def _padded(img, pad):
    """the same image inside rows that are `pad` elements longer (a row stride larger than the row)"""
    if not pad:
        return img
    big = np.zeros((img.shape[0], img.shape[1] + pad), img.dtype)
    big[:, :img.shape[1]] = img
    return big[:, :img.shape[1]]


def _to_device(img):
    """(tensor kept alive, (pointer, row stride in bytes)): the image's rows at their stride in device memory"""
    import torch

    rows, cols = img.shape
    stride, row_bytes = img.strides[0], cols * img.itemsize
    buf = np.zeros((rows, stride), np.uint8)
    buf[:, :row_bytes] = np.ascontiguousarray(img).view(np.uint8).reshape(rows, row_bytes)
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), stride)


def _depth_params(K, want):
    p = adaptors.default_depth_params()
    for i, v in enumerate(np.asarray(K, F).reshape(9)):
        p.camera_matrix[i] = float(v)
    p.depth_scale, p.depth_min, p.depth_max = want["depth_scale"], want["depth_min"], want["depth_max"]
    p.normal_col_gap, p.normal_row_gap = want["col_gap"], want["row_gap"]
    p.normal_max_distance_squared = want["max_distance_squared"]
    p.drop_points_without_normal = int(want["drop_points_without_normal"])
    p.compact = int(want["compact"])
    return p


def _check_scene(scene, r, res, what):
    n = r["points"].shape[0]
    assert scene.size() == n, what
    pts, nrm = scene.get()
    assert ar.same_bits(pts, r["points"]), what
    _, nptr, _ = scene.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and ar.same_bits(nrm, r["normals"]), what
    hd, hi = scene.has_features()
    assert not hd and hi == (r["intensity"] is not None), what
    if hi:
        assert ar.same_bits(scene.features()[1], r["intensity"]), what
    g = scene.global_indices()
    assert np.array_equal(g, r["global_indices"] if r["global_indices"] is not None else np.zeros(0, np.int32)), what
    if res is not None:
        assert res == {"status": abi.ADAPTOR_READY if r["num_raw"] else abi.ADAPTOR_INITIALIZING, "num_raw": r["num_raw"],
                       "num_in_range": r["num_in_range"], "num_valid": r["num_valid"], "scene_size": n}, (what, res)


def _adapt_depth(scene, depth, K, intensity=None, device=False, want_result=True, **kw):
    want = dict(depth_scale=0.001, depth_min=0.4, depth_max=8.0, col_gap=1, row_gap=1, max_distance_squared=0.0625,
                drop_points_without_normal=True, compact=False)
    want.update(kw)
    ad = adaptors.MeasurementAdaptorDepthImage(_depth_params(K, want))
    ad.set_meas(scene)
    keep = []
    if device:
        td, dpair = _to_device(depth)
        keep.append(td)
        ad.params.rows, ad.params.cols = depth.shape
        ipair = itype = None
        if intensity is not None:
            ti, ipair = _to_device(intensity)
            keep.append(ti)
            itype = adaptors._IMAGE_TYPES[intensity.dtype]
        ad.set_raw_data(dpair, ipair, depth_type=adaptors._IMAGE_TYPES[depth.dtype], intensity_type=itype)
    else:
        ad.set_raw_data(depth, intensity)
    assert ad.status() == abi.ADAPTOR_ERROR  # not computed yet
    res = ad.compute(want_result)
    assert ad.status() == (abi.ADAPTOR_READY if depth.size else abi.ADAPTOR_INITIALIZING) or not want_result
    r = ar.adapt_depth_image(np.ascontiguousarray(depth), K, intensity=None if intensity is None else np.ascontiguousarray(intensity), **want)
    return r, res, keep


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_depth_image_full_size(product, dtype, device):
    d, z, mm = _rgbd_depth()
    depth = mm if dtype == "u16" else z
    scene = mapping.Scene(product.scene_binding(0), 3)
    for pad in (0, 6):
        img = _padded(depth, pad)
        for compact in (False, True):
            for gaps in ((0, 0), (1, 1), (3, 3), (2, 5)):
                for drop in ((True,) if gaps == (0, 0) else (False, True)):
                    if pad and (gaps == (3, 3) or not drop):
                        continue  # (the stride does not interact with the gates: two gap settings are enough)
                    what = (dtype, device, pad, compact, gaps, drop)
                    r, res, _ = _adapt_depth(scene, img, d["K"], device=device, col_gap=gaps[0], row_gap=gaps[1],
                                             drop_points_without_normal=drop, compact=compact, depth_min=d["depth_min"],
                                             depth_max=d["depth_max"])
                    _check_scene(scene, r, res, what)
    assert r["num_valid"] > 200000


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_depth_image_with_intensity(product, device):
    d, z, mm = _rgbd_depth()
    rng = np.random.default_rng(11)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for inten in (rng.integers(0, 256, z.shape, dtype=np.uint8), rng.random(z.shape, dtype=F)):
        for compact in (False, True):
            for pad in (0, 4):
                r, res, _ = _adapt_depth(scene, mm, d["K"], intensity=_padded(inten, pad), device=device, compact=compact,
                                         col_gap=3, row_gap=3)
                _check_scene(scene, r, res, (inten.dtype, compact, pad))
    # the next adapt without an intensity image drops the feature
    r, res, _ = _adapt_depth(scene, mm, d["K"], device=device)
    _check_scene(scene, r, res, "no intensity")


def test_depth_image_small_shapes(product):
    K = np.array([[2.0, 0, 1.0], [0, 2.0, 1.0], [0, 0, 1.0]], F)
    scene = mapping.Scene(product.scene_binding(0), 3)
    rng = np.random.default_rng(3)
    shapes = [((1, 1), 1), ((1, 37), 1), ((41, 1), 1), ((3, 3), 2), ((5, 5), 1), ((0, 5), 1), ((4, 0), 1), ((7, 9), 3)]
    for shape, gap in shapes:
        for compact in (False, True):
            for drop in (False, True):
                z = (0.5 + rng.random(shape)).astype(F)
                r, res, _ = _adapt_depth(scene, z, K, compact=compact, col_gap=gap, row_gap=gap, drop_points_without_normal=drop,
                                         max_distance_squared=100.0)
                _check_scene(scene, r, res, (shape, gap, compact, drop))
                if shape == (3, 3):
                    assert not r["has_normal"].any()  # no pixel has both neighbours inside the image
    # an image without a single valid depth: READY with nothing Valid; NaN / inf / zero / out of range
    bad = np.array([[np.nan, np.inf, -np.inf], [0.0, 0.39, 8.5]], F)
    for compact in (False, True):
        r, res, _ = _adapt_depth(scene, bad, K, compact=compact)
        assert res["status"] == abi.ADAPTOR_READY and res["num_valid"] == 0 and res["num_in_range"] == 0
        _check_scene(scene, r, res, "all invalid")
    r, res, _ = _adapt_depth(scene, np.zeros((4, 4), np.uint16), K, compact=True)
    _check_scene(scene, r, res, "all zero counts")


def test_second_compute_into_the_same_scene_shrinks_and_grows(product):
    d, z, mm = _rgbd_depth()
    scene = mapping.Scene(product.scene_binding(0), 3)
    for rows, cols in ((120, 160), (30, 40), (480, 640), (64, 64)):
        for compact in (False, True):
            r, res, _ = _adapt_depth(scene, np.ascontiguousarray(z[:rows, :cols]), d["K"], compact=compact,
                                     intensity=np.ascontiguousarray(mm[:rows, :cols]).astype(F))
            _check_scene(scene, r, res, (rows, cols, compact))


def _scan_ranges(beams):
    pts, _ = syn.scan_2d(syn.se2(0, 0, 0), beams=beams)
    assert pts.shape[0] == beams
    ang = np.deg2rad(np.linspace(-135.0, 135.0, beams))
    return np.linalg.norm(pts, axis=1).astype(F), float(ang[0]), float(ang[1] - ang[0])


def _adapt_scan(scene, ranges, amin, ainc, device=False, want_result=True, **kw):
    want = dict(range_min=0.05, range_max=30.0, half_window=1, max_distance_squared=0.01, drop_points_without_normal=True,
                compact=False)
    want.update(kw)
    p = adaptors.default_scan_params()
    p.angle_min, p.angle_increment = amin, ainc
    p.range_min, p.range_max, p.normal_half_window = want["range_min"], want["range_max"], want["half_window"]
    p.normal_max_distance_squared = want["max_distance_squared"]
    p.drop_points_without_normal, p.compact = int(want["drop_points_without_normal"]), int(want["compact"])
    ad = adaptors.MeasurementAdaptorLaserScan(p)
    ad.set_meas(scene)
    keep = None
    if device:
        import torch

        keep = torch.from_numpy(np.ascontiguousarray(ranges, F)).cuda()
        torch.cuda.synchronize()
        ad.set_raw_data((keep.data_ptr(), len(ranges)))
    else:
        ad.set_raw_data(ranges)
    res = ad.compute(want_result)
    return ar.adapt_laser_scan(ranges, amin, ainc, **want), res, keep


@pytest.mark.parametrize("beams", [1000, 7, 1, 0])
def test_laser_scan(product, beams):
    scene = mapping.Scene(product.scene_binding(0), 2)
    if beams >= 7:
        clean, amin, ainc = _scan_ranges(beams)
    else:
        clean, amin, ainc = np.full(beams, 2.0, F), -0.3, 0.01
    dirty = clean.copy()
    if beams >= 7:
        dirty[2] = np.nan
        dirty[beams // 2] = np.inf
        dirty[beams - 2] = 0.01  # below range_min
    if beams == 1000:
        dirty[100:140] = 31.0  # runs of bad beams
        dirty[400:403] = -np.inf
        dirty[700:760] = np.nan
    for ranges in (clean, dirty):
        for w in (0, 1, 3):
            for compact in (False, True):
                for drop in (False, True):
                    for device in (False, True):
                        r, res, _ = _adapt_scan(scene, ranges, amin, ainc, device=device, half_window=w, compact=compact,
                                                drop_points_without_normal=drop, max_distance_squared=0.01 if w < 3 else 0.09)
                        _check_scene(scene, r, res, (beams, w, compact, drop, device))
    if beams == 1000:
        assert r["num_valid"] > 800


def _snapshot(scene):
    pts, nrm = scene.get()
    inten = scene.features()[1]
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if inten is None else inten.tobytes(),
            scene.global_indices().tobytes())


def test_misuse_leaves_the_scene_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    d, z, mm = _rgbd_depth()
    z = np.ascontiguousarray(z[:48, :64])
    b = product.scene_binding(0)
    s3, s2 = mapping.Scene(b, 3), mapping.Scene(b, 2)
    _adapt_depth(s3, z, d["K"], compact=True, intensity=z)
    rng, amin, ainc = _scan_ranges(50)
    _adapt_scan(s2, rng, amin, ainc, compact=True)
    before3, before2 = _snapshot(s3), _snapshot(s2)
    good = dict(depth_scale=0.001, depth_min=0.4, depth_max=8.0, col_gap=1, row_gap=1, max_distance_squared=0.0625,
                drop_points_without_normal=True, compact=False)
    zp, stride = C.c_void_p(z.ctypes.data), z.strides[0]

    def depth_call(scene=s3, ptr=zp, dtype=abi.IMAGE_F32, st=stride, iptr=None, itype=abi.IMAGE_NONE, ist=0, mem=abi.MEM_HOST,
                   edit=None):
        p = _depth_params(d["K"], good)
        p.rows, p.cols = z.shape
        if edit:
            edit(p)
        return lib.srrg2_adapt_depth_image(scene._h, ptr, dtype, st, iptr, itype, ist, mem, C.byref(p), None)

    def setter(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p, k, v)
        return edit

    def skew(p):
        p.camera_matrix[1] = 0.5

    def no_fx(p):
        p.camera_matrix[0] = 0.0

    bad = [dict(scene=s2), dict(ptr=None), dict(dtype=abi.IMAGE_NONE), dict(dtype=abi.IMAGE_U8), dict(st=stride - 4),
           dict(st=stride + 2), dict(mem=abi.MEM_DEVICE_KEPT), dict(itype=abi.IMAGE_F32, iptr=None, ist=stride),
           dict(itype=abi.IMAGE_U16, iptr=zp, ist=stride), dict(itype=abi.IMAGE_U8, iptr=zp, ist=8),
           dict(edit=setter(normal_col_gap=-1)), dict(edit=setter(normal_col_gap=0)), dict(edit=setter(normal_row_gap=0)),
           dict(edit=setter(rows=-1)), dict(edit=setter(rows=70000, cols=70000)), dict(edit=no_fx)]
    for kw in bad:
        assert depth_call(**kw) == -1, kw  # SRRG2_E_INVALID
        assert product.scene_binding(0).err()  # (the error text is set)
    assert depth_call(edit=skew) == -4  # SRRG2_E_UNSUPPORTED
    assert lib.srrg2_adapt_depth_image(s3._h, zp, abi.IMAGE_F32, stride, None, abi.IMAGE_NONE, 0, abi.MEM_HOST, None, None) == -1
    assert _snapshot(s3) == before3

    rp = C.c_void_p(rng.ctypes.data)

    def scan_call(scene=s2, ptr=rp, n=50, mem=abi.MEM_HOST, **kw):
        p = adaptors.default_scan_params()
        p.angle_min, p.angle_increment = amin, ainc
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.srrg2_adapt_laser_scan(scene._h, ptr, n, mem, C.byref(p), None)

    for kw in (dict(scene=s3), dict(ptr=None), dict(n=-1), dict(mem=7), dict(normal_half_window=-1), dict(angle_min=float("nan")),
               dict(angle_increment=float("inf")), dict(angle_min=1e9)):
        assert scan_call(**kw) == -1, kw
    assert _snapshot(s2) == before2 and _snapshot(s3) == before3
    assert depth_call() == 0 and scan_call() == 0  # the same calls without the mistake go through


def test_aligner_fed_from_the_adapted_scene(product):
    """the C3 aligner of test_c3_full_resolution with its fixed cloud adapted on the device from the depth image (adapt without a
    result, device arrays, SRRG2_MEM_DEVICE_KEPT) = the same aligner fed the restatement's arrays from the host; and it
    converges to the ground truth within the bound that test uses for analytic normals"""
    kind = abi.SE3_QUAT_RIGHT
    d, z, _ = _rgbd_depth()
    cfg = projective_config(kind, abi.SLICE_P2PLANE, d, gate=0.05)
    scene = mapping.Scene(product.scene_binding(0), 3)
    r, res, _ = _adapt_depth(scene, z, d["K"], want_result=False, depth_min=d["depth_min"], depth_max=d["depth_max"])
    assert res is None
    runs = []
    for from_scene in (False, True):
        al = product.MultiAligner(kind, device=0)
        si = al.add_slice(cfg)
        if from_scene:
            cp, cn, n = scene.device_arrays()
            assert n == z.size and cn is not None
            al.set_cloud_device("set_fixed", si, cp, 16, cn, 16, n, kept=True)
        else:
            al.set_fixed(si, r["points"], r["normals"])
        al.set_moving(si, d["moving"], d["moving_normals"])
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()
        runs.append(al)
    assert runs[0].status() == abi.SUCCESS
    assert_same_run(runs[0], runs[1])
    err = float(np.max(np.abs(runs[1].moving_in_fixed() - d["X_gt"])))
    print("adapted fixed cloud: max |X - X_gt| = %.3g, correspondences %d" % (err, runs[1].iteration_stats()[-1]["num_correspondences"]))
    assert err < 2e-4
    _check_scene(scene, r, None, "after the run")


@pytest.mark.parametrize("dim", [2, 3])
def test_tracker_frame_on_an_adapted_measurement(product, dim):
    """clip -> align -> merge (as tools/bench_tracker.py builds the frame) with the measurement adapted, compact, from a laser
    scan / a depth image"""
    b = product.scene_binding(0)
    scene, clipped, meas = mapping.Scene(b, dim), mapping.Scene(b, dim), mapping.Scene(b, dim)
    kind = abi.SE2_RIGHT if dim == 2 else abi.SE3_QUAT_RIGHT
    if dim == 2:
        X_gt = syn.se2(0.10, 0.05, np.deg2rad(3.0))
        frames = []
        for pose in (syn.se2(0, 0, 0), X_gt):
            pts, _ = syn.scan_2d(pose, beams=1000)
            frames.append(np.linalg.norm(pts, axis=1).astype(F))
        ang = np.deg2rad(np.linspace(-135.0, 135.0, 1000))

        def adapt(k):
            return _adapt_scan(meas, frames[k], float(ang[0]), float(ang[1] - ang[0]), compact=True)[1]
    else:
        rows, cols = 240, 320
        K = syn.default_camera(rows, cols)
        T1 = np.zeros((3, 4))
        T1[:, :3] = np.diag([1.0, -1.0, -1.0])
        T1[:, 3] = [0.0, 0.0, 4.0]
        X_gt = syn.se3(np.array([0.03, 0.01, -0.02]), np.deg2rad(np.array([0.5, 1.0, -0.5])))
        frames = [np.ascontiguousarray(syn.render_depth(T, K, rows, cols)[0][:, 2].reshape(rows, cols), F)
                  for T in (T1, syn.se3_mul(T1, X_gt))]

        def adapt(k):
            return _adapt_depth(meas, frames[k], K.astype(F), compact=True, col_gap=2, row_gap=2)[1]
    mg = mapping.MergerCorrespondenceHomo(b)
    cl = mapping.SceneClipperBall(b, range_max=50.0)
    al = product.MultiAligner(kind, 0)
    si = al.add_slice(cue_config(kind, abi.SLICE_P2PLANE, 0.5 if dim == 2 else 0.25, robust=abi.ROBUST_CAUCHY))
    res = adapt(0)
    assert res["num_valid"] == meas.size() > 900
    mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(syn.identity(dim))
    first = mg.compute()
    assert first["num_added"] == res["num_valid"] == scene.size()
    res = adapt(1)
    cl.set_full_scene(scene); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(syn.identity(dim))
    cl.compute()
    cp, cn, n = clipped.device_arrays()
    mp, mn, m = meas.device_arrays()
    assert m == res["num_valid"] and mn is not None
    al.set_cloud_device("set_moving", si, cp, 16, cn, 16, n, kept=True)
    al.set_cloud_device("set_fixed", si, mp, 16, mn, 16, m, kept=True)
    al.set_moving_in_fixed(syn.identity(dim))
    al.compute()
    assert al.status() == abi.SUCCESS
    # moving = the map (frame 0), fixed = the measurement (frame 1): X maps frame 0 into frame 1 = X_gt^-1
    X = al.moving_in_fixed().astype(np.float64)
    Xh = np.vstack([X, [0, 0, 0, 1]]) if dim == 3 else X
    Gh = np.vstack([X_gt, [0, 0, 0, 1]]) if dim == 3 else X_gt
    err = float(np.max(np.abs(Xh @ Gh - np.eye(dim + 1))))
    print("tracker frame dim %d: |X * X_gt - I| = %.3g" % (dim, err))
    est = (np.linalg.inv(Xh)[:3] if dim == 3 else np.linalg.inv(Xh)).astype(F)
    mg.set_measurement_in_scene(est)
    out = mg.compute_from_aligner(al, si, clipped)
    assert mg.status() == mapping.MERGER_SUCCESS and out["num_merged"] > 0, out
    # compact global indices map the measurement's points back to pixels / beams
    g = meas.global_indices()
    assert len(g) == m and np.all(np.diff(g) > 0)
