"""GPU: the dense stereo adaptor (srrg2_adapt_stereo_dense, csrc/stereo_dense.hip) against the numpy restatement of its contract
(tests/stereo_dense_restatement.py), BIT FOR BIT: the disparity image, every counter and the scene (points, normals, intensity,
global indices); against the depth adaptor on the device under the depth rebuilt from the returned disparity; one handle across
shapes; the queued form feeding an aligner; misuse leaves scene and disparity image as they were.
tests/test_stereo_dense_restatement.py pins the restatement itself."""
import ctypes as C

import numpy as np
import pytest

import adaptor_restatement as ar
import stereo_cases as sc
import stereo_dense_cases as dc
import stereo_dense_restatement as sd
from helpers import assert_same_run, projective_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi, adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = F(-7.5)
CAMERA_KEYS = ("compact", "col_gap", "row_gap", "drop_points_without_normal")
PAIR_NAMES = [n for n, _, _ in sc.pairs()] + ["two_plane_%dx%d" % s for s in dc.TWO_PLANE_SIZES]


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
    stride = img.strides[0]
    buf = np.zeros((rows, stride), np.uint8)
    buf[:, :cols] = img
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), stride)


def _adaptor(**kw):
    ad = adaptors.MeasurementAdaptorStereoDense()
    ad.set_camera_matrix(dc.CAMERA)
    ad.stereo.baseline = dc.BASELINE
    for k, v in kw.items():
        if k == "col_gap":
            ad.camera.normal_col_gap = int(v)
        elif k == "row_gap":
            ad.camera.normal_row_gap = int(v)
        elif k in CAMERA_KEYS:
            setattr(ad.camera, k, int(v))
        else:
            setattr(ad.stereo, k, int(v))
    return ad


def _run(scene, left, right, device=False, pad=0, dpad=0, want_result=True, settle=True, **kw):
    """one compute(); returns (adaptor, counters, the whole disparity buffer with its padding columns as a numpy array -- with
    settle=False, device images only, the device tensor as it is: nothing has waited for a call that only queued)"""
    import torch

    ad = _adaptor(**kw)
    ad.set_meas(scene)
    rows, cols = left.shape
    lp, rp = _padded(left, pad), _padded(right, pad + (3 if pad else 0))  # (the two strides differ)
    if device and left.size:
        tl, lpair = _to_device(lp)
        tr, rpair = _to_device(rp)
        ad.camera.rows, ad.camera.cols = rows, cols
        ad.set_raw_data(lpair, rpair)
        td = torch.full((rows, cols + dpad), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        res = ad.compute(want_result, (td.data_ptr(), 4 * (cols + dpad)))
        if not settle:
            return ad, res, (td, tl, tr)
        if scene is not None:
            scene.size()  # (a queued call is settled by the first read of the scene)
        torch.cuda.synchronize()
        buf = td.cpu().numpy()
    else:
        ad.set_raw_data(lp, rp)
        buf = np.full((rows, cols + dpad), SENTINEL, F)
        res = ad.compute(want_result, buf[:, :cols] if left.size else False)
    return ad, res, buf


def _check_scene(scene, r, what):
    n = r["points"].shape[0]
    assert scene.size() == n, what
    pts, nrm = scene.get()
    assert ar.same_bits(pts, r["points"]), what
    _, nptr, _ = scene.device_arrays()
    if r["normals"] is None:
        assert nptr is None, what
    else:
        assert nptr is not None and ar.same_bits(nrm, r["normals"]), what
    assert scene.has_features() == (False, True), what
    assert ar.same_bits(scene.features()[1], r["intensity"]), what
    g = scene.global_indices()
    assert np.array_equal(g, r["global_indices"] if r["global_indices"] is not None else np.zeros(0, np.int32)), what


def _check(scene, res, buf, want, what):
    cols = want["disparity"].shape[1]
    assert buf[:, :cols].tobytes() == want["disparity"].tobytes(), what
    assert (buf[:, cols:] == SENTINEL).all(), what  # (the bytes between rows are the caller's)
    if res is not None:
        assert res == {k: want[k] for k in sd.COUNTERS}, (what, res)
    if scene is not None:
        _check_scene(scene, want, what)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", PAIR_NAMES)
def test_pairs_bit_for_bit(product, name, device):
    """every pair under every variant (both path counts, penalties 0/0, 8/48, 255/255, u 0 / 10 / 99, lr_check off and
    tolerance 0, subpixel off), organised with gaps 1/1; the defaults also with rows at larger, unequal strides and a padded
    disparity stride, without normals, and compact with and without normals"""
    left, right = dc.named(name)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for kw in dc.VARIANTS:
        kw = dict(dc.PAIR_RANGE, **kw)
        _, res, buf = _run(scene, left, right, device=device, **kw)
        _check(scene, res, buf, dc.want(name, **kw), (name, device, kw))
    for cam, pad, dpad in ((dict(), 5, 3), (dict(col_gap=0, row_gap=0), 0, 0), (dict(compact=1), 0, 2),
                           (dict(compact=1, col_gap=0, row_gap=0), 5, 0), (dict(drop_points_without_normal=0), 0, 0)):
        kw = dict(dc.PAIR_RANGE, **cam)
        _, res, buf = _run(scene, left, right, device=device, pad=pad, dpad=dpad, **kw)
        _check(scene, res, buf, dc.want(name, **kw), (name, device, kw, pad, dpad))
    want = dc.want(name, **dc.PAIR_RANGE)
    assert want["num_consistent"] > want["num_evaluated"] // 2 and want["num_valid"] > 100


@pytest.mark.parametrize("nd", dc.ND_COUNTS)
def test_disparity_counts_around_the_wave_width(product, nd):
    """1, 2, 3, 63, 64, 65, 128 and 129 disparities from min_disparity 11 on 120 x 160 (one, two and four slots per lane; 129
    leaves a narrow rectangle), with and without aggregation, from host and device memory"""
    left, right = dc.named(dc.ND_PAIR)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for paths in (4, 0):
        kw = dict(min_disparity=dc.ND_MIN, max_disparity=dc.ND_MIN + nd - 1, paths=paths)
        want = dc.want(dc.ND_PAIR, **kw)
        assert want["num_evaluated"] == (120 - 6) * (160 - 8 - (dc.ND_MIN + nd - 1)) > 0
        for device in (False, True):
            _, res, buf = _run(scene, left, right, device=device, **kw)
            _check(scene, res, buf, want, (nd, paths, device))


def test_256_disparities_on_a_strip(product):
    name, kw = dc.STRIP
    left, right = dc.named(name)
    scene = mapping.Scene(product.scene_binding(0), 3)
    for extra in (dict(), dict(paths=0), dict(uniqueness_ratio=0, lr_tolerance=0)):
        k = dict(kw, **extra)
        want = dc.want(name, **k)
        assert want["num_evaluated"] == 14 * 36
        for device in (False, True):
            _, res, buf = _run(scene, left, right, device=device, **k)
            _check(scene, res, buf, want, (extra, device))
    assert dc.want(name, **kw)["num_consistent"] > 100


@pytest.mark.parametrize("width", dc.WIDTHS)
def test_rectangle_widths_and_a_single_row(product, width):
    """rectangles of 1, 63, 64 and 65 columns, one row (rows = 7) and six rows high: the lines of the path passes end where the
    rectangle ends"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    for rows in (7, 12):
        name = dc.WIDTH_NAME % (rows, width + 8 + dc.WIDTH_RANGE["max_disparity"])
        left, right = dc.named(name)
        for extra in (dict(), dict(paths=0), dict(uniqueness_ratio=0, lr_check=0)):
            kw = dict(dc.WIDTH_RANGE, **extra)
            want = dc.want(name, **kw)
            assert want["num_evaluated"] == (rows - 6) * width
            for device in (False, True):
                _, res, buf = _run(scene, left, right, device=device, **kw)
                _check(scene, res, buf, want, (rows, width, extra, device))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_empty_rectangle_zero_pixels_flat_and_tiled(product, device):
    scene = mapping.Scene(product.scene_binding(0), 3)
    # cols = max_disparity + 8: no rectangle, READY, a scene of NaN points; rows = 6 likewise
    for name, kw in (("noise_12x28", dict(min_disparity=4, max_disparity=20)), ("noise_6x64", dict(dc.PAIR_RANGE))):
        for cam in (dict(), dict(compact=1)):
            k = dict(kw, **cam)
            want = dc.want(name, **k)
            assert want["num_evaluated"] == 0 and want["status"] == 0 and want["num_valid"] == 0
            _, res, buf = _run(scene, *dc.named(name), device=device, **k)
            _check(scene, res, buf, want, (name, cam))
    # zero pixels: an empty scene, INITIALIZING
    ad, res, _ = _run(scene, *dc.named("0x0"), device=device)
    want = dc.want("0x0")
    assert res == {k: want[k] for k in sd.COUNTERS} and res["status"] == abi.ADAPTOR_INITIALIZING and scene.size() == 0
    assert ad.status() == abi.ADAPTOR_INITIALIZING
    # the flat pair: rejected everywhere at u = 10, min_disparity everywhere at u = 0; the tiled pair: 10 and 34 tie
    for name, kw in (("flat", dict(min_disparity=3, max_disparity=12)), ("tiled", dict(min_disparity=1, max_disparity=40))):
        for u in (10, 0):
            k = dict(kw, uniqueness_ratio=u)
            want = dc.want(name, **k)
            assert want["num_unique"] == (want["num_evaluated"] if u == 0 else 0) and want["num_evaluated"] > 0
            _, res, buf = _run(scene, *dc.named(name), device=device, **k)
            _check(scene, res, buf, want, (name, u))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_disparity_without_a_scene(product, device):
    """dst == NULL: the disparity image and the first five counters, the scene's counters 0"""
    left, right = dc.named("two_plane_67x101")
    want = dc.want("two_plane_67x101", **dc.TWO_PLANE_RANGE)
    for want_result in (True, False):
        _, res, buf = _run(None, left, right, device=device, dpad=1, want_result=want_result, **dc.TWO_PLANE_RANGE)
        assert buf[:, :101].tobytes() == want["disparity"].tobytes() and (buf[:, 101:] == SENTINEL).all()
        if want_result:
            zeroed = dict({k: want[k] for k in sd.COUNTERS}, num_in_range=0, num_valid=0, scene_size=0)
            assert res == zeroed, res


@pytest.mark.parametrize("compact", [0, 1])
def test_composition_with_the_depth_adaptor(product, compact):
    """the composition rule on the device: srrg2_adapt_depth_image on the depth rebuilt from the returned disparity leaves the
    same scene"""
    left, right = dc.named("two_plane_96x128")
    a, b = (mapping.Scene(product.scene_binding(0), 3) for _ in range(2))
    ad, res, buf = _run(a, left, right, compact=compact, **dc.TWO_PLANE_RANGE)
    depth = sd.depth_of(buf, dc.CAMERA, dc.BASELINE)
    dep = adaptors.MeasurementAdaptorDepthImage()
    C.memmove(C.byref(dep.params), C.byref(ad.camera), C.sizeof(abi.DepthAdaptorParams))
    dep.set_meas(b)
    dep.set_raw_data(depth, left)
    got = dep.compute()
    assert got["scene_size"] == res["scene_size"] > 1000
    assert (got["num_in_range"], got["num_valid"]) == (res["num_in_range"], res["num_valid"])
    pa, na = a.get()
    pb, nb = b.get()
    assert ar.same_bits(pa, pb) and ar.same_bits(na, nb)
    assert ar.same_bits(a.features()[1], b.features()[1]) and np.array_equal(a.global_indices(), b.global_indices())


def test_one_handle_across_shapes_and_behind_a_queued_adapt(product):
    """the workspaces grow and are reused: shapes growing and shrinking on one scene; then behind an organised depth adapt that
    only queued its work on the scene's stream"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    order = [("two_plane_48x64", dc.TWO_PLANE_RANGE), ("120x160", dict(min_disparity=1, max_disparity=70)),
             ("two_plane_67x101", dc.TWO_PLANE_RANGE), ("noise_7x19_s5", dc.WIDTH_RANGE), ("120x160", dc.PAIR_RANGE),
             ("two_plane_48x64", dict(dc.TWO_PLANE_RANGE, compact=1))]
    for device in (False, True):
        for name, kw in order:
            _, res, buf = _run(scene, *dc.named(name), device=device, **kw)
            _check(scene, res, buf, dc.want(name, **kw), (name, device))
    depth = np.full((96, 128), 2.0, F)
    dep = adaptors.MeasurementAdaptorDepthImage()
    dep.set_camera_matrix(dc.CAMERA)
    dep.set_meas(scene)
    dep.set_raw_data(depth)
    assert dep.compute(want_result=False) is None
    _, res, buf = _run(scene, *dc.named("two_plane_67x101"), **dc.TWO_PLANE_RANGE)
    _check(scene, res, buf, dc.want("two_plane_67x101", **dc.TWO_PLANE_RANGE), "behind a queued adapt")


def test_queued_form_feeds_a_projective_aligner(product):
    """out == NULL, organised, the disparity on the device: the call only queues; device_arrays + set_fixed(DEVICE_KEPT) follow
    at once and a projective compute() runs exactly as one fed the restatement's arrays from the host"""
    name, kw = "two_plane_96x128", dict(dc.TWO_PLANE_RANGE)
    left, right = dc.named(name)
    want = dc.want(name, **kw)
    compact = dc.want(name, compact=1, **kw)
    assert compact["scene_size"] > 3000
    kind = abi.SE3_QUAT_RIGHT
    data = dict(K=dc.CAMERA, rows=96, cols=128, depth_min=0.4, depth_max=8.0)
    cfg = projective_config(kind, abi.SLICE_P2PLANE, data, gate=0.05)
    scene = mapping.Scene(product.scene_binding(0), 3)
    _, res, tensors = _run(scene, left, right, device=True, want_result=False, settle=False, **kw)
    assert res is None
    runs = []
    for from_scene in (True, False):
        al = product.MultiAligner(kind, device=0)
        si = al.add_slice(cfg)
        if from_scene:
            cp, cn, n = scene.device_arrays()
            assert n == 96 * 128 and cn is not None
            al.set_cloud_device("set_fixed", si, cp, 16, cn, 16, n, kept=True)
        else:
            al.set_fixed(si, want["points"], want["normals"])
        al.set_moving(si, compact["points"], compact["normals"])
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()
        runs.append(al)
    assert runs[0].iteration_stats()[-1]["num_correspondences"] > 3000
    assert_same_run(runs[1], runs[0])
    _check(scene, None, tensors[0].cpu().numpy(), want, "after the run")


def _snapshot(scene):
    pts, nrm = scene.get()
    return scene.size(), pts.tobytes(), nrm.tobytes(), scene.has_features(), scene.global_indices().tobytes()


def test_misuse_leaves_scene_and_disparity_unchanged(product):
    lib = _capi.lib()
    left, right = dc.named("two_plane_48x64")
    scene = mapping.Scene(product.scene_binding(0), 3)
    two = mapping.Scene(product.scene_binding(0), 2)
    _run(scene, left, right, compact=1, **dc.TWO_PLANE_RANGE)
    before = _snapshot(scene)
    assert before[0] > 100
    disp = np.full((48, 64), SENTINEL, F)
    out = abi.DenseStereoResult()

    def call(dst=scene, lptr=left.ctypes.data, lst=64, rptr=right.ctypes.data, rst=64, mem=abi.MEM_HOST, dptr=disp.ctypes.data, dst_stride=256,
             cam=None, sp=None, null_sp=False, null_cam=False):
        ad = _adaptor(**dc.TWO_PLANE_RANGE)
        ad.camera.rows, ad.camera.cols = 48, 64
        for k, v in (cam or {}).items():
            if k == "skew":
                ad.camera.camera_matrix[1] = v
            elif k == "fx":
                ad.camera.camera_matrix[0] = v
            else:
                setattr(ad.camera, k, v)
        for k, v in (sp or {}).items():
            setattr(ad.stereo, k, v)
        return lib.srrg2_adapt_stereo_dense(None if dst is None else dst._h, lptr, lst, rptr, rst, mem,
                                            None if null_cam else C.byref(ad.camera), None if null_sp else C.byref(ad.stereo), dptr,
                                            dst_stride, C.byref(out))

    invalid = [dict(null_sp=True), dict(null_cam=True), dict(sp=dict(baseline=0.0)), dict(sp=dict(baseline=float("nan"))),
               dict(sp=dict(baseline=float("inf"))), dict(sp=dict(baseline=-0.1)), dict(sp=dict(min_disparity=0)),
               dict(sp=dict(min_disparity=25)), dict(sp=dict(paths=8)), dict(sp=dict(paths=1)), dict(sp=dict(p1=-1)),
               dict(sp=dict(p1=49)), dict(sp=dict(p2=256)), dict(sp=dict(uniqueness_ratio=-1)), dict(sp=dict(uniqueness_ratio=100)),
               dict(sp=dict(lr_check=2)), dict(sp=dict(subpixel=-1)), dict(sp=dict(lr_tolerance=-1)), dict(sp=dict(lr_tolerance=17)),
               dict(sp=dict(reserved=1)), dict(dst=None, dptr=None), dict(dst_stride=252), dict(dst_stride=258), dict(dst=two),
               dict(mem=abi.MEM_DEVICE_KEPT), dict(mem=7), dict(lptr=None), dict(rptr=None), dict(lst=63), dict(rst=63),
               dict(cam=dict(rows=-1)), dict(cam=dict(normal_col_gap=0)), dict(cam=dict(normal_row_gap=-1)), dict(cam=dict(fx=0.0)),
               dict(cam=dict(fx=float("nan")))]
    unsupported = [dict(cam=dict(skew=0.25)), dict(sp=dict(min_disparity=1, max_disparity=257)),
                   dict(cam=dict(rows=20000, cols=100000), lst=100000, rst=100000, dst_stride=400000)]
    for code, cases in ((-1, invalid), (-4, unsupported)):
        for kw in cases:
            assert call(**kw) == code, kw
            assert b"adapt_stereo_dense" in lib.srrg2_amd_last_error(), kw
            assert _snapshot(scene) == before and (disp == SENTINEL).all(), kw
    assert call() == 0 and out.num_consistent > 100 and not (disp == SENTINEL).any()  # the same call without the mistake
