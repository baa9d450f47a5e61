"""GPU: the image-feature adaptor (srrg2_adapt_image_features, csrc/features.hip) against the numpy restatement of its contract
(tests/features_restatement.py), BIT FOR BIT: points, intensities, descriptors, global indices, keypoint records and every
counter; depth-gated points against the depth adaptor's own output on the device; misuse leaves the scene as it was; and through
the stack: the descriptor database fed from a feature scene matches as one fed the restatement's descriptors from the host, and
the ball clipper carries the descriptors of the points it keeps."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptor_restatement as ar
import features_cases as fc
import features_restatement as fr
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping

pytestmark = pytest.mark.gpu
F = np.float32
IMAGES = dict(fc.images())


@functools.lru_cache(maxsize=None)
def _want(name, threshold=20, max_features=0, oriented=True, depth=None):
    """the restatement's result for a named case image, computed once and shared"""
    img = _named(name)
    d = None if depth is None else fc.depth_for(img, depth)
    return fr.extract(img, K=fc.CAMERA, fast_threshold=threshold, max_features=max_features, oriented=oriented, depth=d)


def _named(name):
    if name in IMAGES:
        return IMAGES[name]
    return {"quadrant": fc.quadrant_image(), "quadrant_mirrored": fc.quadrant_image(True), "tiled": fc.tiled_image(),
            "32x40": fc.rectangles(32, 40, 1), "0x0": np.zeros((0, 0), np.uint8), "crop_a": fc.crops()[0][1],
            "crop_b": fc.crops()[1][1]}[name]


def _padded(img, pad):
    """the same image inside rows that are `pad` elements longer (a row stride larger than the row)"""
    if not pad:
        return img
    big = np.full((img.shape[0], img.shape[1] + pad), 7, img.dtype)
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


def _adaptor(threshold=20, max_features=0, oriented=True):
    ad = adaptors.MeasurementAdaptorImageFeatures()
    ad.set_camera_matrix(fc.CAMERA)
    ad.params.fast_threshold, ad.params.max_features, ad.params.oriented = threshold, max_features, int(oriented)
    return ad


def _extract(scene, img, depth=None, device=False, pad=0, **params):
    ad = _adaptor(**params)
    ad.set_meas(scene)
    img_p, depth_p = _padded(img, pad), None if depth is None else _padded(depth, pad)
    keep = []
    if device and img.size:
        ti, ipair = _to_device(img_p)
        keep.append(ti)
        dpair = dtype = None
        if depth is not None:
            td, dpair = _to_device(depth_p)
            keep.append(td)
            dtype = adaptors._IMAGE_TYPES[depth.dtype]
        ad.camera.rows, ad.camera.cols = img.shape
        ad.set_raw_data(ipair, dpair, intensity_type=abi.IMAGE_U8, depth_type=dtype)
    else:
        ad.set_raw_data(img_p, depth_p)
    assert ad.status() == abi.ADAPTOR_ERROR  # not computed yet
    res = ad.compute()
    assert ad.status() == (abi.ADAPTOR_READY if img.size else abi.ADAPTOR_INITIALIZING)
    return ad, res


def _check(scene, ad, res, want, what):
    n = want["scene_size"]
    assert res == {k: want[k] for k in ("status", "num_pixels", "num_candidates", "num_maxima", "num_selected", "num_with_depth",
                                        "scene_size")}, (what, res)
    assert scene.size() == n, what
    pts, _ = scene.get()
    assert ar.same_bits(pts, want["points"]), what
    assert scene.device_arrays()[1] is None, what  # no normals
    assert scene.has_features() == (True, True), what
    desc, inten = scene.features()
    assert desc.tobytes() == want["descriptors"].tobytes(), what
    assert inten.tobytes() == want["intensity"].tobytes(), what
    assert np.array_equal(scene.global_indices(), want["global_indices"]), what
    kp = ad.keypoints()
    assert kp.shape == (n, 4) and np.array_equal(kp[:, :3], want["keypoints"]) and not kp[:, 3].any(), what


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_images_bit_for_bit(product, name, device):
    """every size plain and rotated: thresholds 0 / 20 / 254, oriented or not, rows at their own stride and at a larger one"""
    img = IMAGES[name]
    scene = mapping.Scene(product.scene_binding(0), 3)
    for threshold in fc.THRESHOLDS:
        for oriented in (True, False):
            if not oriented and threshold != 20:
                continue
            for pad in (0, 5):
                ad, res = _extract(scene, img, device=device, pad=pad, threshold=threshold, oriented=oriented)
                _check(scene, ad, res, _want(name, threshold, 0, oriented), (name, device, threshold, oriented, pad))
    assert _want(name, 254)["scene_size"] == 0 < _want(name)["scene_size"] <= _want(name, 0)["scene_size"]
    assert (scene.get()[0][:, 2] == 1.0).all()  # without depth: the bearing at z = 1


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_smallest_images(product, device):
    """33 x 33 holds one admissible pixel, a side of 32 none (READY, empty), no pixel at all is INITIALIZING"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad, res = _extract(scene, _named("quadrant"), device=device)
    _check(scene, ad, res, _want("quadrant"), "quadrant")
    assert ad.keypoints()[:, :3].tolist() == [[544, 100, 4]]
    for name in ("quadrant_mirrored", "32x40", "0x0"):
        ad, res = _extract(scene, _named(name), device=device)
        _check(scene, ad, res, _want(name), name)
        assert scene.size() == 0 and res["status"] == (abi.ADAPTOR_INITIALIZING if name == "0x0" else abi.ADAPTOR_READY)
    # ... and the scene is usable again afterwards
    ad, res = _extract(scene, _named("quadrant"), device=device, oriented=False)
    _check(scene, ad, res, _want("quadrant", oriented=False), "quadrant again")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_cap_cuts_inside_a_class_of_equal_scores(product, device):
    img = fc.tiled_image()
    full, caps = fc.tie_caps(img)
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad, res = _extract(scene, img, device=device)
    _check(scene, ad, res, _want("tiled"), "uncapped")
    assert res["scene_size"] == len(full["keypoints"])
    for which, m in sorted(caps.items()):
        ad, res = _extract(scene, img, device=device, max_features=m)
        _check(scene, ad, res, _want("tiled", 20, m), which)
        assert res["num_selected"] == min(m, res["num_maxima"])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_depth_gate_and_points_of_the_depth_adaptor(product, kind, device):
    """holes and out-of-range depths under some keypoints; the kept points are the rows of srrg2_adapt_depth_image's organised
    output at those pixels, bit for bit -- the existing adaptor on the device, not only the restatement"""
    name = "96x128"
    img, depth = IMAGES[name], fc.depth_for(IMAGES[name], kind)
    b = product.scene_binding(0)
    scene, organised = mapping.Scene(b, 3), mapping.Scene(b, 3)
    for pad, m in ((0, 0), (3, 0), (0, 40)):
        ad, res = _extract(scene, img, depth=depth, device=device, pad=pad, max_features=m)
        want = _want(name, 20, m, True, kind)
        _check(scene, ad, res, want, (kind, device, pad, m))
        assert 0 < res["num_with_depth"] < res["num_selected"]  # the cap comes before the depth gate
    dp = adaptors.MeasurementAdaptorDepthImage(ad.camera)
    dp.params.normal_col_gap = dp.params.normal_row_gap = 0
    dp.params.compact = 0
    dp.set_meas(organised)
    dp.set_raw_data(depth)
    dp.compute()
    rows = organised.get()[0][scene.global_indices()]
    assert np.isfinite(rows).all() and ar.same_bits(scene.get()[0], rows)


def test_launch_shape_and_keypoint_capacity(product):
    """128 keypoints (32 workgroups of the describe kernel) over several tile rows; keypoints_out takes what fits"""
    from srrg2_slam_interfaces_amd import _capi

    name = "120x160"
    img = IMAGES[name]
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad, res = _extract(scene, img, max_features=128)
    want = _want(name, 20, 128)
    _check(scene, ad, res, want, name)
    assert res["scene_size"] == 128 < res["num_maxima"]
    rows_of = want["global_indices"] // 160
    assert rows_of.min() < 32 and rows_of.max() >= 96
    lib = _capi.lib()
    for capacity in (0, 5, 128, 500):
        buf = np.full((max(capacity, 1) + 1, 4), -7, np.int32)
        out = abi.FeatureResult()
        assert lib.srrg2_adapt_image_features(scene._h, C.c_void_p(img.ctypes.data), abi.IMAGE_U8, img.strides[0], None,
                                              abi.IMAGE_NONE, 0, abi.MEM_HOST, C.byref(ad.camera), C.byref(ad.params),
                                              buf.ctypes.data_as(C.POINTER(abi.Keypoint)), capacity, C.byref(out)) == 0
        got = min(capacity, 128)
        assert np.array_equal(buf[:got, :3], want["keypoints"][:got]) and (buf[got:] == -7).all()
        assert out.scene_size == 128
    # no result, no keypoints: the scene is complete all the same
    assert lib.srrg2_adapt_image_features(scene._h, C.c_void_p(img.ctypes.data), abi.IMAGE_U8, img.strides[0], None,
                                          abi.IMAGE_NONE, 0, abi.MEM_HOST, C.byref(ad.camera), C.byref(ad.params), None, 0, None) == 0
    assert scene.features()[0].tobytes() == want["descriptors"].tobytes()


def test_shifted_crops_agree_on_common_keypoints(product):
    """two crops of one image shifted by whole pixels: a keypoint present in both has the same score, bin and descriptor"""
    (oa, A), (ob, B) = fc.crops()
    b = product.scene_binding(0)
    sa, sb = mapping.Scene(b, 3), mapping.Scene(b, 3)
    ada, _ = _extract(sa, A)
    adb, _ = _extract(sb, B)
    cols = A.shape[1]
    da, db = sa.features()[0], sb.features()[0]
    where = {(int(p) // cols + oa[0], int(p) % cols + oa[1]): i for i, p in enumerate(sa.global_indices())}
    common = 0
    for j, p in enumerate(sb.global_indices()):
        i = where.get((int(p) // cols + ob[0], int(p) % cols + ob[1]))
        if i is not None:
            common += 1
            assert np.array_equal(ada.keypoints()[i, 1:], adb.keypoints()[j, 1:]) and da[i].tobytes() == db[j].tobytes()
    assert common >= 60 and common < min(sa.size(), sb.size())


def _snapshot(scene):
    pts, nrm = scene.get()
    desc, inten = scene.features()
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if desc is None else desc.tobytes(),
            None if inten is None else inten.tobytes(), scene.global_indices().tobytes())


def test_misuse_leaves_the_scene_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    img = IMAGES["48x64"]
    depth = fc.depth_for(img, "u16")
    b = product.scene_binding(0)
    s3, s2 = mapping.Scene(b, 3), mapping.Scene(b, 2)
    _extract(s3, img)
    s2.set(np.random.default_rng(1).uniform(-1, 1, (40, 2)).astype(F))
    before3, before2 = _snapshot(s3), _snapshot(s2)
    assert before3[0] > 0
    ip, dp = C.c_void_p(img.ctypes.data), C.c_void_p(depth.ctypes.data)
    stride, dstride = img.strides[0], depth.strides[0]
    kp = (abi.Keypoint * 8)()

    def call(scene=s3, iptr=ip, itype=abi.IMAGE_U8, ist=stride, dptr=None, dtype=abi.IMAGE_NONE, dst=0, mem=abi.MEM_HOST,
             cam=None, par=None, capacity=8, null_cam=False, null_par=False):
        ad = _adaptor()
        ad.camera.rows, ad.camera.cols = img.shape
        if cam:
            cam(ad.camera)
        for k, v in (par or {}).items():
            setattr(ad.params, k, v)
        return lib.srrg2_adapt_image_features(scene._h, iptr, itype, ist, dptr, dtype, dst, mem,
                                              None if null_cam else C.byref(ad.camera), None if null_par else C.byref(ad.params),
                                              kp, capacity, None)

    def setter(**kw):
        def edit(p):
            for k, v in kw.items():
                setattr(p, k, v)
        return edit

    def matrix(i, v):
        def edit(p):
            p.camera_matrix[i] = v
        return edit

    assert call() == 0  # (the call itself is good)
    assert _snapshot(s3) == before3
    bad = [dict(scene=s2), dict(null_cam=True), dict(null_par=True), dict(iptr=None), dict(cam=setter(rows=-1)),
           dict(cam=setter(cols=-1)), dict(cam=setter(rows=70000, cols=70000)), dict(ist=stride - 1), dict(ist=0),
           dict(mem=abi.MEM_DEVICE_KEPT), dict(mem=7), dict(itype=abi.IMAGE_NONE), dict(itype=9),
           dict(par=dict(fast_threshold=-1)), dict(par=dict(fast_threshold=255)), dict(par=dict(max_features=-1)),
           dict(par=dict(oriented=2)), dict(par=dict(oriented=-1)), dict(par=dict(reserved=1)), dict(capacity=-1),
           dict(dptr=dp, dtype=abi.IMAGE_NONE, dst=dstride), dict(dptr=dp, dtype=abi.IMAGE_U8, dst=dstride),
           dict(dptr=None, dtype=abi.IMAGE_U16, dst=dstride), dict(dptr=dp, dtype=9, dst=dstride),
           dict(dptr=dp, dtype=abi.IMAGE_U16, dst=dstride - 2), dict(dptr=dp, dtype=abi.IMAGE_U16, dst=dstride + 1),
           dict(dptr=C.c_void_p(depth.ctypes.data + 1), dtype=abi.IMAGE_U16, dst=dstride),
           dict(dptr=dp, dtype=abi.IMAGE_F32, dst=dstride),  # (a row of floats is twice as long)
           dict(cam=matrix(0, 0.0)), dict(cam=matrix(4, 0.0)), dict(cam=matrix(0, float("nan"))), dict(cam=matrix(4, float("inf")))]
    for kw in bad:
        assert call(**kw) == -1, kw  # SRRG2_E_INVALID
        assert b"adapt_image_features" in lib.srrg2_amd_last_error()
    for kw in (dict(itype=abi.IMAGE_F32), dict(itype=abi.IMAGE_U16), dict(cam=matrix(1, 0.5))):
        assert call(**kw) == -4, kw  # SRRG2_E_UNSUPPORTED
    assert _snapshot(s3) == before3 and _snapshot(s2) == before2
    assert call(dptr=dp, dtype=abi.IMAGE_U16, dst=dstride) == 0 and 0 < s3.size() < before3[0]


def _same_match(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.num_matches, b.num_matches)
    assert np.array_equal(a.map_counts, b.map_counts) and len(a.correspondences) == len(b.correspondences)
    for x, y in zip(a.correspondences, b.correspondences):
        assert x.tobytes() == y.tobytes()


def test_through_the_stack(product):
    """the descriptor database fed from feature scenes answers as one fed the restatement's descriptors from the host; the ball
    clipper moves a keypoint's descriptor and intensity with its point"""
    (_, A), (_, B) = fc.crops()
    b = product.scene_binding(0)
    sa, sb = mapping.Scene(b, 3), mapping.Scene(b, 3)
    _extract(sa, A)
    _extract(sb, B)
    wa, wb = _want("crop_a"), _want("crop_b")
    dev, host = product.DescriptorDatabase(0), product.DescriptorDatabase(0)
    ones = lambda w: np.ones(w["scene_size"], np.uint8)  # noqa: E731  (every keypoint's point is finite)
    assert dev.add_scene(sa) == host.add(wa["descriptors"], ones(wa)) == 0
    for kw in (dict(query_index=1), dict(query_index=1, max_distance=12.5, min_matches=10)):
        got, want = dev.match_scene(sb, **kw), host.match(wb["descriptors"], ones(wb), **kw)
        _same_match(got, want)
    assert want.indices.tolist() == [0] and int(want.num_matches[0]) >= 60
    # clip_ball around the principal axis: the bearings within 0.06 of (0, 0, 1)
    clipped = mapping.Scene(b, 3)
    cl = mapping.SceneClipperBall(b, range_max=0.06)
    cl.set_full_scene(sa)
    cl.set_clipped_scene_in_robot(clipped)
    pose = np.eye(3, 4, dtype=F)
    pose[2, 3] = 1.0
    cl.set_robot_in_local_map(pose)
    cl.compute()
    g = cl.global_indices()
    assert 3 < len(g) < sa.size()
    d, i = sa.features()
    cd, ci = clipped.features()
    assert cd.tobytes() == d[g].tobytes() and ci.tobytes() == i[g].tobytes()
