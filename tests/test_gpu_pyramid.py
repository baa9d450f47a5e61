"""GPU: the scale-pyramid feature adaptor (srrg2_adapt_image_features_pyramid, csrc/pyramid.hip) against the numpy restatement of
its contract (tests/pyramid_restatement.py), BIT FOR BIT: points, intensities, descriptors, global indices, keypoint records and
every per-level counter; one level against srrg2_adapt_image_features itself; misuse leaves the scene as it was; and through the
stack: the descriptor database and the tracker fed a pyramid scene."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptor_restatement as ar
import features_cases as fc
import pyramid_cases as pc
import pyramid_restatement as pr
import tracking_restatement as tr
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping

pytestmark = pytest.mark.gpu
F = np.float32
RESULT_KEYS = ("status", "num_levels_built", "scene_size", "rows", "cols", "num_candidates", "num_maxima", "num_selected",
               "num_with_depth", "quota")


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


def _adaptor(num_levels=4, num=6, den=5, threshold=20, max_features=0, oriented=True):
    ad = adaptors.MeasurementAdaptorImageFeaturesPyramid()
    ad.set_camera_matrix(pc.CAMERA)
    ad.params.fast_threshold, ad.params.max_features, ad.params.oriented = threshold, max_features, int(oriented)
    ad.pyramid.num_levels, ad.pyramid.scale_num, ad.pyramid.scale_den = num_levels, num, den
    return ad


def _extract(scene, img, depth=None, device=False, pad=0, **params):
    ad = _adaptor(**params)
    ad.set_meas(scene)
    img_p, depth_p = _padded(img, pad), None if depth is None else _padded(depth, pad)
    keep = []
    if device:
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
    res = ad.compute()
    assert ad.status() == abi.ADAPTOR_READY
    return ad, res


def _records(ad):
    kp = ad.keypoints()
    return np.stack([kp[n] for n in kp.dtype.names], -1).reshape(-1, 8)


def _check(scene, ad, res, want, what):
    n = want["scene_size"]
    assert {k: res[k] for k in RESULT_KEYS} == {k: want[k] for k in RESULT_KEYS} and res["reserved"] == 0, (what, res)
    assert scene.size() == n, what
    pts, _ = scene.get()
    assert ar.same_bits(pts, want["points"]), what
    assert scene.device_arrays()[1] is None, what  # no normals
    assert scene.has_features() == (True, True), what
    desc, inten = scene.features()
    assert desc.tobytes() == want["descriptors"].tobytes(), what
    assert inten.tobytes() == want["intensity"].tobytes(), what
    assert np.array_equal(scene.global_indices(), want["global_indices"]), what
    assert np.array_equal(_records(ad), want["keypoints"]), what


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", pc.CASES, ids=["%s-%dx%d_%d" % (c[0], c[1], c[2], c[3]) for c in pc.CASES])
def test_cases_bit_for_bit(product, case, device):
    """48x64 at 6/5: the third level (33 x 44) finds nothing, the fourth (27 x 36) is not built; 67x101: odd sizes, pitches that
    are no multiple of 4 before padding, 4 levels with 41 / 23 / 11 / 4 keypoints, at 2/1 a level 1 of 33 x 50 without keypoints;
    96x128 and tiled at all three ratios; quadrant: of 2 levels only level 0 exists; 120x160: 8 asked for, 7 built.  Oriented or
    not, rows at their own stride and at a larger one."""
    name, levels, num, den = case
    img = pc.image(name)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for oriented, pad in ((True, 0), (False, 5)):
        ad, res = _extract(scene, img, device=device, pad=pad, num_levels=levels, num=num, den=den, oriented=oriented)
        _check(scene, ad, res, pc.reference(name, levels, num, den, 0, oriented), (case, device, oriented, pad))
    assert res["num_levels_built"] == len(pr.level_sizes(img.shape[0], img.shape[1], levels, num, den))


def test_a_camera_frame_with_eight_levels(product):
    """480 x 640 at 6/5: all 8 levels are built (the last is 132 x 176), under a cap that cuts every level"""
    img = pc.image("frame")
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad, res = _extract(scene, img, num_levels=8, max_features=3000)
    want = pc.reference("frame", 8, 6, 5, 3000)
    _check(scene, ad, res, want, "frame")
    assert res["num_levels_built"] == 8 and res["scene_size"] == 3000 and min(res["num_with_depth"]) > 50
    assert res["num_selected"] == res["quota"] and all(m > q for m, q in zip(res["num_maxima"], res["quota"]))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_depth_gate_reads_the_nearest_level_0_pixel(product, kind, device):
    """holes and out-of-range depths under keypoints of every level; then holes under keypoints of levels >= 1 only"""
    name = "96x128"
    img = pc.image(name)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for pad, m in ((0, 0), (3, 60)):
        ad, res = _extract(scene, img, depth=pc.depth_for(name, kind), device=device, pad=pad, max_features=m)
        _check(scene, ad, res, pc.reference(name, 4, 6, 5, m, True, kind), (kind, device, pad, m))
        assert min(res["num_with_depth"]) > 0 and sum(res["num_with_depth"]) < sum(res["num_selected"])  # (cap, then depth gate)
    depth, punched = pc.upper_levels_depth(name, kind)
    ad, res = _extract(scene, img, depth=depth, device=device)
    want = pr.extract_pyramid(img, K=pc.CAMERA, max_features=0, depth=depth)
    _check(scene, ad, res, want, (kind, device, "upper levels"))
    full = pc.reference(name, 4, 6, 5)
    assert res["num_with_depth"][0] == full["num_with_depth"][0] and sum(res["num_with_depth"][1:]) < sum(full["num_with_depth"][1:])
    assert not np.isin(scene.global_indices(), punched).any()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["96x128", "tiled"])
def test_caps(product, name, device):
    """a cap that leaves the last level a quota of 0 (it keeps nothing, though 0 means "no cap" inside a level), one with a tie
    at a level's cut, one above every level's count"""
    img = pc.image(name)
    caps = pc.cap_settings(name)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for which, m in sorted(caps.items()):
        ad, res = _extract(scene, img, device=device, max_features=m)
        _check(scene, ad, res, pc.reference(name, 4, 6, 5, m), (name, which, m))
        assert res["num_selected"] == [min(q, n) for q, n in zip(res["quota"], res["num_maxima"])] and sum(res["quota"]) == m
    assert pc.reference(name, 4, 6, 5, caps["zero_quota"])["quota"][-1] == 0


def _raw_call(scene, img, ad, buf, capacity, out, pyr=None):
    from srrg2_slam_interfaces_amd import _capi

    return _capi.lib().srrg2_adapt_image_features_pyramid(
        scene._h, C.c_void_p(img.ctypes.data), abi.IMAGE_U8, img.strides[0], None, abi.IMAGE_NONE, 0, abi.MEM_HOST, C.byref(ad.camera),
        C.byref(ad.params), C.byref(ad.pyramid if pyr is None else pyr),
        None if buf is None else buf.ctypes.data_as(C.POINTER(abi.PyramidKeypoint)), capacity, None if out is None else C.byref(out))


def test_keypoint_capacity_below_the_total(product):
    """keypoints_out takes what fits, across the level boundary; no result and no records: the scene is complete all the same"""
    name = "67x101"
    img = pc.image(name)
    want = pc.reference(name, 4, 6, 5)
    total = want["scene_size"]
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = _adaptor()
    ad.camera.rows, ad.camera.cols = img.shape
    for capacity in (0, 5, want["num_with_depth"][0] + 3, total, total + 50):
        buf = np.full((max(capacity, 1) + 1, 8), -7, np.int32)
        out = abi.PyramidResult()
        assert _raw_call(scene, img, ad, buf, capacity, out) == 0
        got = min(capacity, total)
        assert np.array_equal(buf[:got], want["keypoints"][:got]) and (buf[got:] == -7).all()
        assert out.scene_size == total
    assert _raw_call(scene, img, ad, None, 0, None) == 0
    assert scene.features()[0].tobytes() == want["descriptors"].tobytes()


@pytest.mark.parametrize("depth", [None, "u16"])
def test_one_level_is_the_single_scale_extractor(product, depth):
    """num_levels = 1 against srrg2_adapt_image_features on a second scene: the scene, the counters, the records' first three
    fields"""
    name = "96x128"
    img, d = pc.image(name), None if depth is None else pc.depth_for(name, depth)
    b = product.scene_binding(0)
    sp, ss = mapping.Scene(b, 3), mapping.Scene(b, 3)
    for m in (0, 40):
        ad, res = _extract(sp, img, depth=d, num_levels=1, max_features=m)
        plain = adaptors.MeasurementAdaptorImageFeatures()
        plain.set_camera_matrix(pc.CAMERA)
        plain.params.max_features = m
        plain.set_meas(ss)
        plain.set_raw_data(img, d)
        single = plain.compute()
        assert single["scene_size"] == res["scene_size"] > 10 and res["num_levels_built"] == 1
        for k in ("num_candidates", "num_maxima", "num_selected", "num_with_depth"):
            assert res[k] == [single[k]], k
        assert sp.get()[0].tobytes() == ss.get()[0].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(sp.features(), ss.features()))
        assert np.array_equal(sp.global_indices(), ss.global_indices())
        assert np.array_equal(_records(ad)[:, :3], plain.keypoints()[:, :3])


def test_one_scene_for_a_large_a_small_and_a_large_image(product):
    scene = mapping.Scene(product.scene_binding(0), 3)
    for name, levels in (("120x160", 8), ("48x64", 4), ("quadrant", 2), ("120x160", 8)):
        ad, res = _extract(scene, pc.image(name), num_levels=levels)
        _check(scene, ad, res, pc.reference(name, levels, 6, 5), name)
    ad, res = _extract(scene, fc.rectangles(32, 40, 1))  # no admissible pixel on level 0: empty, READY, nothing built
    assert scene.size() == 0 and res["num_levels_built"] == 0 and res["status"] == abi.ADAPTOR_READY and res["rows"] == []
    _extract(scene, pc.image("48x64"))
    from srrg2_slam_interfaces_amd import _capi

    ad.camera.rows = ad.camera.cols = 0  # no pixel at all: empty, INITIALIZING
    out = abi.PyramidResult()
    assert _capi.lib().srrg2_adapt_image_features_pyramid(scene._h, None, abi.IMAGE_U8, 0, None, abi.IMAGE_NONE, 0, abi.MEM_HOST,
                                                          C.byref(ad.camera), C.byref(ad.params), C.byref(ad.pyramid), None, 0,
                                                          C.byref(out)) == 0
    assert scene.size() == 0 and out.status == abi.ADAPTOR_INITIALIZING and out.num_levels_built == 0


def _snapshot(scene):
    pts, nrm = scene.get()
    desc, inten = scene.features()
    return (scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), None if desc is None else desc.tobytes(),
            None if inten is None else inten.tobytes(), scene.global_indices().tobytes())


def test_refusals_leave_the_scene_unchanged(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    img = pc.image("48x64")
    b = product.scene_binding(0)
    s3, s2 = mapping.Scene(b, 3), mapping.Scene(b, 2)
    _extract(s3, img)
    s2.set(np.random.default_rng(1).uniform(-1, 1, (40, 2)).astype(F))
    before3, before2 = _snapshot(s3), _snapshot(s2)
    assert before3[0] > 0
    kp = (abi.PyramidKeypoint * 8)()

    def call(scene=s3, iptr=C.c_void_p(img.ctypes.data), itype=abi.IMAGE_U8, ist=img.strides[0], mem=abi.MEM_HOST, cam=None, par=None,
             pyr=None, capacity=8, null_pyr=False):
        ad = _adaptor()
        ad.camera.rows, ad.camera.cols = img.shape
        for k, v in (cam or {}).items():
            setattr(ad.camera, k, v)
        for k, v in (par or {}).items():
            setattr(ad.params, k, v)
        for k, v in (pyr or {}).items():
            setattr(ad.pyramid, k, v)
        return lib.srrg2_adapt_image_features_pyramid(scene._h, iptr, itype, ist, None, abi.IMAGE_NONE, 0, mem, C.byref(ad.camera),
                                                      C.byref(ad.params), None if null_pyr else C.byref(ad.pyramid), kp, capacity, None)

    assert call() == 0 and _snapshot(s3) == before3  # (the call itself is good)
    bad = [dict(null_pyr=True), dict(pyr=dict(num_levels=0)), dict(pyr=dict(num_levels=9)), dict(pyr=dict(num_levels=-1)),
           dict(pyr=dict(scale_num=5, scale_den=5)), dict(pyr=dict(scale_num=4, scale_den=5)), dict(pyr=dict(scale_num=5, scale_den=2)),
           dict(pyr=dict(scale_num=9, scale_den=8)), dict(pyr=dict(scale_num=1, scale_den=0)), dict(pyr=dict(scale_num=0, scale_den=0)),
           dict(pyr=dict(scale_num=2, scale_den=-1)), dict(pyr=dict(reserved=1)),
           # ... and what srrg2_adapt_image_features refuses
           dict(scene=s2), dict(iptr=None), dict(cam=dict(rows=-1)), dict(cam=dict(rows=70000, cols=70000)), dict(ist=img.strides[0] - 1),
           dict(mem=7), dict(itype=abi.IMAGE_NONE), dict(par=dict(fast_threshold=255)), dict(par=dict(max_features=-1)),
           dict(par=dict(oriented=2)), dict(par=dict(reserved=1)), dict(capacity=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw  # SRRG2_E_INVALID
        assert b"adapt_image_features_pyramid" in lib.srrg2_amd_last_error()
    for kw in (dict(itype=abi.IMAGE_F32), dict(itype=abi.IMAGE_U16), dict(cam=dict(rows=1, cols=4194305), iptr=C.c_void_p(img.ctypes.data),
                                                                         ist=4194305)):
        assert call(**kw) == -4, kw  # SRRG2_E_UNSUPPORTED
    assert _snapshot(s3) == before3 and _snapshot(s2) == before2
    for ok in (dict(num_levels=8, scale_num=8, scale_den=7), dict(num_levels=1, scale_num=2, scale_den=1), dict(scale_num=8, scale_den=4)):
        assert call(pyr=ok) == 0, ok


def _same_match(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.num_matches, b.num_matches)
    assert np.array_equal(a.map_counts, b.map_counts) and len(a.correspondences) == len(b.correspondences)
    for x, y in zip(a.correspondences, b.correspondences):
        assert x.tobytes() == y.tobytes()


@functools.lru_cache(maxsize=None)
def _scaled_wants():
    """the restatement of A's pyramid, of A at a single scale and of B = A resampled by 7/5 at a single scale: (images, results)"""
    A, B = pc.scaled_pair(120, 160, 3, 7, 5)
    imgs = (A, A, B)
    return imgs, tuple(pr.extract_pyramid(img, K=pc.CAMERA, max_features=0, num_levels=n) for img, n in zip(imgs, (4, 1, 1)))


def _scaled_scenes(product):
    """the three scenes of _scaled_wants() on the device, checked against it"""
    imgs, wants = _scaled_wants()
    b = product.scene_binding(0)
    scenes = [mapping.Scene(b, 3) for _ in range(3)]
    for scene, img, want, levels in zip(scenes, imgs, wants, (4, 1, 1)):
        ad, res = _extract(scene, img, num_levels=levels)
        _check(scene, ad, res, want, levels)
    return b, scenes, wants


def test_descriptor_database_takes_a_pyramid_scene(product):
    """add_scene of A's pyramid scene, match_scene of B's single-scale scene (B = A resampled by 7/5): the pairs are those of a
    database fed the restatement's descriptors from the host, and more of them are correct than with A's single-scale scene"""
    _, (s_pyr, s_single, s_b), (w_pyr, w_single, w_b) = _scaled_scenes(product)
    ones = lambda w: np.ones(w["scene_size"], np.uint8)  # noqa: E731  (every keypoint's point is finite)
    correct = []
    for scene, want in ((s_pyr, w_pyr), (s_single, w_single)):
        dev, host = product.DescriptorDatabase(0), product.DescriptorDatabase(0)
        assert dev.add_scene(scene) == host.add(want["descriptors"], ones(want)) == 0
        got = dev.match_scene(s_b, query_index=1, max_distance=64.0)
        _same_match(got, host.match(w_b["descriptors"], ones(w_b), query_index=1, max_distance=64.0))
        assert got.indices.tolist() == [0]
        corr = got.correspondences[0]
        correct.append(pr.correct_matches(want["keypoints"][:, 5:7].astype(np.float64), w_b["keypoints"][:, 5:7].astype(np.float64),
                                          corr["moving_idx"], corr["fixed_idx"], 7, 5))
    assert correct[0] > correct[1] > 0, correct


def _track(b, moving, fixed, rows, cols):
    ft = mapping.FeatureTracker(b)
    ft.set_camera_matrix(pc.CAMERA)
    ft.params.image_rows, ft.params.image_cols = rows, cols
    ft.set_moving(moving)
    ft.set_fixed(fixed)
    return ft


def test_tracker_takes_a_pyramid_scene_as_the_map(product):
    """a pyramid scene as `moving` (the landmarks, in any order) against its own image's single-scale scene as `fixed`: the pairs
    of the tracker's restatement fed the pyramid's restatement; level-0 keypoints find themselves at distance 0"""
    b, (s_pyr, s_single, _), (w_pyr, w_single, _) = _scaled_scenes(product)
    ft = _track(b, s_pyr, s_single, 120, 160)
    pairs = ft.compute()
    want = tr.track(w_pyr["points"], w_pyr["descriptors"], w_single["global_indices"], w_single["descriptors"], np.eye(3, 4, dtype=F),
                    pc.CAMERA, 120, 160)
    assert pairs.tobytes() == want["correspondences"].tobytes() and ft.result["num_moving"] == w_pyr["scene_size"]
    own = pairs[pairs["moving_idx"] < w_pyr["num_with_depth"][0]]
    assert len(own) > 50 and np.array_equal(own["moving_idx"], own["fixed_idx"]) and not own["response"].any()


def test_tracker_accepts_a_pyramid_scene_as_fixed(product):
    """a level-major pyramid scene as `fixed` (its pixels ascend inside a level only, and repeat across levels): the tracker
    searches it level by level and gives the pairs of its restatement, which knows no order; a landmark taken from level l finds
    its own keypoint at distance 0.  With the cross check and without, with a margin; and after the scene's content was replaced
    by other means the same handle is judged by the plain rule again"""
    b, (s_pyr, s_single, s_b), (w_pyr, w_single, w_b) = _scaled_scenes(product)
    assert (np.diff(w_pyr["global_indices"]) <= 0).any() and min(w_pyr["num_with_depth"]) > 0
    eye = np.eye(3, 4, dtype=F)
    for moving, wm in ((s_single, w_single), (s_pyr, w_pyr)):
        if moving is s_pyr:  # (moving and fixed must be two scenes: a second copy of the pyramid scene)
            moving = mapping.Scene(b, 3)
            _extract(moving, _scaled_wants()[0][0])
        for cross, margin, radius in ((1, 0, 16), (0, 0, 16), (1, 8, 5)):
            ft = _track(b, moving, s_pyr, 120, 160)
            ft.params.cross_check, ft.params.min_margin, ft.params.search_radius = cross, margin, radius
            pairs = ft.compute()
            want = tr.track(wm["points"], wm["descriptors"], w_pyr["global_indices"], w_pyr["descriptors"], eye, pc.CAMERA, 120, 160,
                            search_radius=radius, min_margin=margin, cross_check=bool(cross))
            assert pairs.tobytes() == want["correspondences"].tobytes(), (cross, margin, radius)
            assert ft.result["num_fixed"] == w_pyr["scene_size"] and len(pairs) > 50
            assert ft.result["num_correspondences"] == want["num_correspondences"] and ft.result["num_accepted"] == want["num_accepted"]
    assert (pairs["fixed_idx"] >= w_pyr["num_with_depth"][0]).any()  # keypoints of upper levels are matched too
    # the handle's content replaced by a clip of a single-scale scene: ascending again, accepted by the plain rule ...
    cl = mapping.SceneClipperBall(b, range_max=10.0)
    cl.set_full_scene(s_single)
    cl.set_clipped_scene_in_robot(s_pyr)
    cl.set_robot_in_local_map(eye)
    cl.compute()
    assert s_pyr.size() == s_single.size()
    _track(b, s_single, s_pyr, 120, 160).compute()
    # ... and by a set(): no global indices, SRRG2_E_STATE as before
    s_pyr.set(w_pyr["points"])
    s_pyr.set_features(w_pyr["descriptors"])
    with pytest.raises(RuntimeError, match="no global indices"):
        _track(b, s_single, s_pyr, 120, 160).compute()
