"""GPU: the rectification stage (srrg2_rectifier_*, srrg2_rectify_image / _pair, csrc/rectify.hip) against the numpy restatement of
its contract (tests/rectify_restatement.py), BIT FOR BIT: the map and its counters for every named camera model; the remap of
U8 / U16 / F32 images over the shape list, from and to host and device memory, at padded strides and a misaligned destination;
the pair against the two single calls; the queued chains rectify -> adaptor with no host wait between, against the adaptors'
restatements on the restated rectified images; misuse leaves the destination as it was.
tests/test_rectify_restatement.py pins the restatement itself."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptor_restatement as ar
import features_restatement as fr
import rectify_cases as rc
import rectify_restatement as rr
import stereo_dense_restatement as sd
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import _capi, adaptors, mapping, rectify

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = {"u8": abi.IMAGE_U8, "u16": abi.IMAGE_U16, "f32": abi.IMAGE_F32}
INFO_KEYS = ("num_pixels", "num_valid", "first_row", "last_row", "first_col", "last_col")
SENTINEL = 0xa5


@functools.lru_cache(maxsize=None)
def _want_map(name, rot, dst, wide=False):
    """the restated map of a named model on a target (computed once, shared; treat as read-only) with its arguments"""
    K, dist, R, shape = rc.model(name, rot)
    new_K = K if wide else rc.target_K(name, dst)
    uv, info = rr.build_map(K, dist, R, new_K, shape, dst)
    return uv, info, (K, dist, R, new_K, shape, dst)


def _set(r, args):
    K, dist, R, new_K, shape, dst = args
    return r.set_camera(K, dist, R, new_K, shape, dst)


def _bytes_2d(img):
    """the image's rows as bytes at their stride: (rows, stride) uint8"""
    rows, cols = img.shape
    stride = img.strides[0] if rows > 1 else cols * img.itemsize
    out = np.zeros((rows, stride), np.uint8)
    out[:, :cols * img.itemsize] = np.ascontiguousarray(img).view(np.uint8).reshape(rows, cols * img.itemsize)
    return out, stride


def _to_device(img):
    """(tensor kept alive, (pointer, row stride in bytes))"""
    import torch

    buf, stride = _bytes_2d(img)
    t = torch.from_numpy(buf).cuda() if buf.size else torch.zeros((1, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t, (t.data_ptr(), stride)


def _padded(img, pad, fill=7):
    if not pad:
        return img
    big = np.full((img.shape[0], img.shape[1] + pad), fill, img.dtype)
    big[:, :img.shape[1]] = img
    return big[:, :img.shape[1]]


def _case(kind, dst):
    """(name, rot) of the model a target shape is remapped under: the VGA source for the one large target, `small` otherwise;
    depth images under the identity rotation"""
    name = "vga_barrel" if dst[1] > 101 else "small"
    return name, ("tilted" if kind == "u8" else "identity")


# ---- the map --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rot", sorted(rc.ROTATIONS))
@pytest.mark.parametrize("name", sorted(rc.MODELS))
def test_map_and_counters_bit_for_bit(product, name, rot):
    r = product.ImageRectifier()
    targets = [((37, 53), False), ((67, 101), False)] + ([(rc.BEHIND_WIDE, True)] if name == "behind" else [])
    for dst, wide in targets:
        uv, info, args = _want_map(name, rot, dst, wide)
        got = _set(r, args)
        assert got == info and r.info == info, (name, rot, dst, got, info)
        assert np.array_equal(r.map(), uv), (name, rot, dst)
    if name == "behind":
        assert 0 < info["num_valid"] < info["num_pixels"]
    cam = r.camera()
    assert (cam.rows, cam.cols) == targets[-1][0] and cam.depth_scale == F(0.001)
    assert list(cam.camera_matrix) == [float(F(v)) for v in (args[3][0, 0], 0, args[3][0, 2], 0, args[3][1, 1], args[3][1, 2], 0, 0, 1)]


def test_map_of_the_full_vga_target_an_empty_target_and_an_empty_source(product):
    r = product.ImageRectifier()
    uv, info, args = _want_map("pincushion", "tilted", (480, 640))
    assert _set(r, args) == info and 0 < info["num_valid"] < info["num_pixels"]
    assert np.array_equal(r.map(), uv)
    K, dist, R, shape = rc.model("small")
    assert r.set_camera(K, dist, R, K, shape, (0, 0)) == dict(num_pixels=0, num_valid=0, first_row=-1, last_row=-1, first_col=-1, last_col=-1)
    assert r.map().shape == (0, 0, 2)
    assert r.rectify(rc.image(shape)).shape == (0, 0)  # a destination of zero pixels: accepted, nothing written
    info = r.set_camera(K, dist, R, K, (0, 0), (3, 5))
    assert info["num_valid"] == 0 and (r.map() == rr.INVALID).all()
    assert (r.rectify(np.zeros((0, 0), np.uint8), border=9) == 9).all()


# ---- the remap ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dst", rc.SHAPES, ids=["%dx%d" % s for s in rc.SHAPES])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_remap_over_the_shapes_and_memory_spaces(product, kind, dst):
    name, rot = _case(kind, dst)
    uv, info, args = _want_map(name, rot, dst)
    src = rc.image(args[4], kind)
    r = product.ImageRectifier()
    _set(r, args)
    for border in (0, 200):
        want = rr.remap(uv, src, border)
        got = r.rectify(src, border=border)  # host -> host
        assert got.dtype == src.dtype and got.tobytes() == want.tobytes(), (kind, dst, border, "host->host")
        if kind != "u8":
            break
    want = rr.remap(uv, src, 200)
    keep, pair = _to_device(src)
    for source, out in ((src, "device"), (pair, "device"), (pair, "host")):
        got = r.rectify(source, out=out, border=200, image_type=KINDS[kind])
        got = got.numpy() if isinstance(got, rectify.DeviceImage) else got
        assert got.tobytes() == want.tobytes(), (kind, dst, type(source), out)
    if info["num_pixels"] > 100:
        assert info["num_valid"] > info["num_pixels"] // 2


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_padded_rows_misaligned_destination_and_the_bytes_between_rows(product, kind):
    """source and destination rows at different, larger strides with a sentinel in the padding; the destination one ELEMENT past
    an aligned address (U8: the pointer is 1 mod 4, so no row starts on a word), in host and in device memory"""
    import torch

    esize = np.dtype(rc.image((1, 1), kind).dtype).itemsize
    r = product.ImageRectifier()
    for dst in ((37, 53), (67, 101), (3, 5)):
        name, rot = _case(kind, dst)
        uv, _, args = _want_map(name, rot, dst)
        _set(r, args)
        src = _padded(rc.image(args[4], kind), 5)
        want = rr.remap(uv, src, 200)
        keep, spair = _to_device(src)
        for pad in (0, 3, 8):
            stride = (dst[1] + pad) * esize
            raw = np.full(dst[0] * stride + 64, SENTINEL, np.uint8)
            # host: a view that starts one element into the buffer
            view = np.lib.stride_tricks.as_strided(raw[esize:].view(src.dtype), dst, (stride, esize))
            r.rectify(src, out=view, border=200)
            t = torch.from_numpy(np.full(raw.shape, SENTINEL, np.uint8)).cuda()
            torch.cuda.synchronize()
            base = t.data_ptr()
            assert base % 4 == 0
            for source in (src, spair):  # host and device sources into the device destination
                r.rectify(source, out=(base + esize, stride), border=200, image_type=KINDS[kind])
                torch.cuda.synchronize()
                dev = t.cpu().numpy()
                for buf, what in ((raw, "host"), (dev, "device")):
                    img = np.lib.stride_tricks.as_strided(buf[esize:].view(src.dtype), dst, (stride, esize))
                    assert img.tobytes() == want.tobytes(), (kind, dst, pad, what)
                    written = np.zeros(buf.shape, bool)
                    rows = np.lib.stride_tricks.as_strided(written[esize:], (dst[0], dst[1] * esize), (stride, 1))
                    rows[...] = True
                    assert (buf[~written] == SENTINEL).all(), (kind, dst, pad, what)


def test_nan_payloads_survive(product):
    uv, _, args = _want_map("small", "identity", (37, 53))
    src = rc.nan_payload_image(args[4])
    r = product.ImageRectifier()
    _set(r, args)
    want = rr.remap(uv, src)
    assert len(np.unique(want.view(np.uint32))) > 500
    assert r.rectify(src).tobytes() == want.tobytes()
    keep, pair = _to_device(src)
    assert r.rectify(pair, image_type=abi.IMAGE_F32).numpy().tobytes() == want.tobytes()


def test_one_handle_set_three_times(product):
    """growing then shrinking shapes: the map and the staging blocks are reused"""
    r = product.ImageRectifier()
    for name, rot, dst in (("small", "tilted", (3, 5)), ("vga_barrel", "tilted", (67, 101)), ("small", "identity", (37, 53))):
        uv, info, args = _want_map(name, rot, dst)
        assert _set(r, args) == info
        assert np.array_equal(r.map(), uv)
        for kind in (("u8", "u16") if rot == "identity" else ("u8",)):
            src = rc.image(args[4], kind)
            want = rr.remap(uv, src, 3)
            assert r.rectify(src, border=3).tobytes() == want.tobytes()
            assert r.rectify(src, out="device", border=3).numpy().tobytes() == want.tobytes()


# ---- the pair -------------------------------------------------------------------------------------------------------------

def _rig_rectifier(product, dst_shape=None):
    s = product.StereoRectifier()
    s.set_calibration(rc.RIG_K, rc.RIG_DISTORTION, rc.RIG_K, rc.RIG_DISTORTION, rc.RIG_R, rc.RIG_T, rc.rig()["shape"], dst_shape)
    return s


def test_pair_equals_the_two_single_calls(product):
    g = rc.rig()
    s = _rig_rectifier(product)
    assert s.R1.tobytes() == g["R1"].tobytes() and s.R2.tobytes() == g["R2"].tobytes() and s.baseline == g["baseline"]
    assert np.array_equal(s.left.map(), g["maps"][0]) and np.array_equal(s.right.map(), g["maps"][1])
    for border in (0, 200):
        wl, wr = rc.rig_rectified(border)
        singles = s.left.rectify(g["raw"][0], border=border), s.right.rectify(g["raw"][1], border=border)
        assert singles[0].tobytes() == wl.tobytes() and singles[1].tobytes() == wr.tobytes()
        dl, dr = s.rectify(*g["raw"], border=border)  # from the host
        assert dl.numpy().tobytes() == wl.tobytes() and dr.numpy().tobytes() == wr.tobytes()
        kl, lp = _to_device(_padded(g["raw"][0], 3))
        kr, rp = _to_device(_padded(g["raw"][1], 6))
        dl, dr = s.rectify(lp, rp, border=border)  # from device memory, two strides
        assert dl.numpy().tobytes() == wl.tobytes() and dr.numpy().tobytes() == wr.tobytes()
    # sources of different shapes are fine, targets of different shapes are not
    uv, _, args = _want_map("small", "tilted", g["shape"])
    _set(s.right, args)
    dl, dr = s.rectify(g["raw"][0], rc.image(args[4]))
    assert dl.numpy().tobytes() == rc.rig_rectified()[0].tobytes() and dr.numpy().tobytes() == rr.remap(uv, rc.image(args[4])).tobytes()
    _set(s.right, _want_map("small", "tilted", (37, 53))[2])
    before = dl.numpy().copy()
    with pytest.raises(RuntimeError, match="targets of different shape"):
        s.rectify(g["raw"][0], rc.image(args[4]), out=(dl, dr))
    assert dl.numpy().tobytes() == before.tobytes()


# ---- queued chains: no host wait between the rectifier and the adaptor ---------------------------------------------------------

def _camera9(cam):
    return tuple(float(v) for v in cam.camera_matrix)


def test_queued_image_feeds_the_feature_adaptor(product):
    g = rc.rig()
    s = _rig_rectifier(product)
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = adaptors.MeasurementAdaptorImageFeatures()
    ad.params.max_features = 0
    s.left.camera(ad.camera)
    keep, raw = _to_device(g["raw"][0])
    out = s.left.rectify(raw, order_on=scene, image_type=abi.IMAGE_U8)  # queued on the scene's stream
    ad.set_meas(scene)
    ad.set_raw_data(out.pair, intensity_type=abi.IMAGE_U8)
    res = ad.compute()
    want = fr.extract(rc.rig_rectified()[0], K=_camera9(ad.camera), fast_threshold=ad.params.fast_threshold, max_features=0)
    assert want["scene_size"] > 20
    assert res == {k: want[k] for k in ("status", "num_pixels", "num_candidates", "num_maxima", "num_selected", "num_with_depth", "scene_size")}
    pts, _ = scene.get()
    assert ar.same_bits(pts, want["points"])
    desc, inten = scene.features()
    assert desc.tobytes() == want["descriptors"].tobytes() and inten.tobytes() == want["intensity"].tobytes()
    assert np.array_equal(scene.global_indices(), want["global_indices"])
    assert np.array_equal(ad.keypoints()[:, :3], want["keypoints"])
    assert out.numpy().tobytes() == rc.rig_rectified()[0].tobytes()


def test_queued_pair_feeds_dense_stereo(product):
    """raw pair -> rectify_pair(order_on = scene) -> srrg2_adapt_stereo_dense(out = NULL, organised), settled by the first read
    of the scene: disparity, scene and counters are those of the dense restatement on the restated rectified pair"""
    import torch

    g = rc.rig()
    rows, cols = g["shape"]
    s = _rig_rectifier(product)
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = adaptors.MeasurementAdaptorStereoDense()
    s.camera(ad.camera)
    ad.stereo.baseline = s.baseline
    ad.stereo.min_disparity, ad.stereo.max_disparity = rc.RIG_RANGE["min_disparity"], rc.RIG_RANGE["max_disparity"]
    ad.set_meas(scene)
    want = sd.adapt(*rc.rig_rectified(), _camera9(ad.camera), float(F(s.baseline)), **rc.RIG_RANGE)
    assert want["num_consistent"] > 2000 and want["num_valid"] > 1000
    disp = torch.full((rows, cols), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for source in ("host", "device"):
        if source == "host":
            dl, dr = s.rectify(*g["raw"], order_on=scene)
        else:
            kl, lp = _to_device(g["raw"][0])
            kr, rp = _to_device(g["raw"][1])
            dl, dr = s.rectify(lp, rp, order_on=scene)
        ad.set_raw_data(dl.pair, dr.pair)
        assert ad.compute(False, (disp.data_ptr(), 4 * cols)) is None  # only queued
        assert scene.size() == rows * cols  # the first read settles the chain
        torch.cuda.synchronize()
        assert disp.cpu().numpy().tobytes() == want["disparity"].tobytes(), source
        pts, nrm = scene.get()
        assert ar.same_bits(pts, want["points"]) and ar.same_bits(nrm, want["normals"]), source
        assert ar.same_bits(scene.features()[1], want["intensity"]), source
        res = ad.compute(True, (disp.data_ptr(), 4 * cols))  # the same pair again, with the counters
        assert res == {k: want[k] for k in sd.COUNTERS}, (source, res)


def test_queued_depth_image_feeds_the_depth_adaptor(product):
    uv, _, args = _want_map("small", "identity", (67, 101))
    depth = rc.image(args[4], "u16")
    inten = rc.image(args[4], "u8")
    r = product.ImageRectifier()
    _set(r, args)
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = adaptors.MeasurementAdaptorDepthImage()
    r.camera(ad.params)
    kd, dp = _to_device(depth)
    od = r.rectify(dp, order_on=scene, image_type=abi.IMAGE_U16)
    oi = r.rectify(inten, order_on=scene, border=0)  # a host source, queued as well
    assert od.pair[1] % 2 == 0 and oi.pair[1] >= 101
    ad.set_meas(scene)
    ad.set_raw_data(od.pair, oi.pair, depth_type=abi.IMAGE_U16, intensity_type=abi.IMAGE_U8)
    assert ad.compute(want_result=False) is None
    want = ar.adapt_depth_image(rr.remap(uv, depth), _camera9(ad.params), intensity=rr.remap(uv, inten, 0))
    assert want["num_valid"] > 500
    assert scene.size() == 67 * 101
    pts, nrm = scene.get()
    assert ar.same_bits(pts, want["points"]) and ar.same_bits(nrm, want["normals"])
    assert ar.same_bits(scene.features()[1], want["intensity"])


def test_no_device_memory_leak(product):
    """a rectifier's map (2.5 MB at 480 x 640) and staging blocks go with the handle: 25 cycles of create / set / host-to-host
    rectify / destroy would hold 75 MB otherwise, against the 8 MB bound of tests/test_gpu_lifetime.py"""
    def _free_bytes():  # hipMemGetInfo of the HIP runtime the product library itself is linked against
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipDeviceSynchronize() == 0
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    _, _, args = _want_map("pincushion", "tilted", (480, 640))
    src = rc.image(args[4])

    def cycle():
        r = product.ImageRectifier()
        _set(r, args)
        r.rectify(src, border=1)
        r.close()

    for _ in range(3):
        cycle()  # allocator warm-up
    before = _free_bytes()
    for _ in range(25):
        cycle()
    after = _free_bytes()
    assert before - after < 8 << 20, (before, after)


# ---- misuse ---------------------------------------------------------------------------------------------------------------

def test_misuse_leaves_the_destination_untouched(product):
    import torch

    lib = _capi.lib()
    uv, _, args = _want_map("small", "tilted", (37, 53))
    src8, src16 = rc.image(args[4]), rc.image(args[4], "u16")
    r = product.ImageRectifier()
    unset = product.ImageRectifier()
    _set(r, args)
    other = product.ImageRectifier()
    _set(other, args)
    dst = np.full((37, 64), SENTINEL, np.uint8)
    dev = torch.full((37, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    two = mapping.Scene(product.scene_binding(0), 2)

    def image(h=r, order_on=None, sptr=src8.ctypes.data, type_=abi.IMAGE_U8, sstride=53, smem=abi.MEM_HOST, dptr=dst.ctypes.data,
              dstride=64, dmem=abi.MEM_HOST, border=0):
        return lib.srrg2_rectify_image(None if h is None else h._h, None if order_on is None else order_on._h, sptr, type_, sstride,
                                       smem, dptr, dstride, dmem, border)

    invalid = [dict(h=None), dict(h=unset), dict(sptr=None), dict(dptr=None), dict(sstride=52), dict(dstride=52), dict(sstride=-53),
               dict(smem=abi.MEM_DEVICE_KEPT), dict(smem=7), dict(dmem=abi.MEM_DEVICE_KEPT), dict(dmem=-1), dict(type_=abi.IMAGE_NONE),
               dict(type_=4), dict(border=-1), dict(border=256),
               dict(type_=abi.IMAGE_U16, sptr=src16.ctypes.data, sstride=105), dict(type_=abi.IMAGE_U16, sptr=src16.ctypes.data + 1, sstride=106),
               dict(type_=abi.IMAGE_U16, sptr=src16.ctypes.data, sstride=106, dstride=107),
               dict(type_=abi.IMAGE_F32, sstride=216, dstride=214), dict(type_=abi.IMAGE_F32, sstride=216, dstride=216, dptr=dst.ctypes.data + 2)]
    unsupported = [dict(type_=abi.IMAGE_U16, sptr=src16.ctypes.data, sstride=106, dstride=128),  # a depth image under a rotation
                   dict(type_=abi.IMAGE_F32, sstride=212, dstride=256)]
    for code, cases in ((-1, invalid), (-4, unsupported)):
        for kw in cases:
            assert image(**kw) == code, kw
            assert b"rectify_image" in lib.srrg2_amd_last_error(), kw
            assert (dst == SENTINEL).all(), kw
            if "dptr" not in kw and "dmem" not in kw:  # the same mistake with the destination in device memory
                assert image(dptr=dev.data_ptr(), dmem=abi.MEM_DEVICE, **kw) == code, kw
    torch.cuda.synchronize()
    assert (dev.cpu().numpy() == SENTINEL).all()

    def pair(hl=r, hr=other, mem=abi.MEM_HOST, lptr=src8.ctypes.data, rptr=src8.ctypes.data, lst=53, rst=53, dl=dst.ctypes.data,
             dr=dst.ctypes.data + 37 * 32, dls=64, drs=64, dmem=abi.MEM_HOST, border=0):
        return lib.srrg2_rectify_pair(None if hl is None else hl._h, None if hr is None else hr._h, None, lptr, lst, rptr, rst, mem, dl,
                                      dls, dr, drs, dmem, border)

    for kw in (dict(hl=None), dict(hr=None), dict(hr=unset), dict(hr=r), dict(mem=2), dict(dmem=5), dict(lptr=None), dict(rptr=None),
               dict(dl=None), dict(dr=None), dict(lst=52), dict(rst=0), dict(dls=52), dict(drs=52), dict(border=300)):
        assert pair(**kw) == -1, kw
        assert b"rectify_pair" in lib.srrg2_amd_last_error(), kw
        assert (dst == SENTINEL).all(), kw
    # get_map and camera
    small = np.full(10, 7, np.int32)
    assert lib.srrg2_rectifier_get_map(r._h, small.ctypes.data_as(C.POINTER(C.c_int32)), small.size) == -1 and (small == 7).all()
    assert lib.srrg2_rectifier_get_map(unset._h, small.ctypes.data_as(C.POINTER(C.c_int32)), small.size) == -1
    assert lib.srrg2_rectifier_get_map(r._h, None, 2 * 37 * 53) == -1
    assert lib.srrg2_rectifier_camera(unset._h, C.byref(abi.DepthAdaptorParams())) == -1
    assert lib.srrg2_rectifier_camera(r._h, None) == -1
    # a refused set leaves the handle's map as it was
    bad = rectify.default_rectifier_params()
    assert lib.srrg2_rectifier_set(r._h, C.byref(bad), None) == -1
    assert np.array_equal(r.map(), uv)
    # the same calls without the mistake
    assert image() == 0 and dst[:, :53].tobytes() == rr.remap(uv, src8, 0).tobytes() and (dst[:, 53:] == SENTINEL).all()
    assert pair(dr=dst.ctypes.data) == 0
    # order_on is accepted with a host destination (the call then waits) and a scene of any dim
    assert image(order_on=two) == 0


def test_destroy_right_after_a_queued_call(product):
    import torch

    uv, _, args = _want_map("vga_barrel", "tilted", (67, 101))
    src = rc.image(args[4])
    want = rr.remap(uv, src, 0)
    scene = mapping.Scene(product.scene_binding(0), 3)
    keep, pair = _to_device(src)
    outs = []
    for _ in range(3):
        r = product.ImageRectifier()
        _set(r, args)
        outs.append(r.rectify(pair, order_on=scene, image_type=abi.IMAGE_U8))
        r.close()  # waits for the queued work that reads its map
        del r
    torch.cuda.synchronize()
    for o in outs:
        assert o.numpy().tobytes() == want.tobytes()
    # a new map behind a queued call, and a call on the rectifier's own stream behind a queued one
    r = product.ImageRectifier()
    _set(r, args)
    first = r.rectify(pair, order_on=scene, image_type=abi.IMAGE_U8)
    second = r.rectify(src, out="host")
    uv2, _, args2 = _want_map("small", "tilted", (37, 53))
    third = r.rectify(pair, order_on=scene, image_type=abi.IMAGE_U8)
    _set(r, args2)
    assert second.tobytes() == want.tobytes() and first.numpy().tobytes() == want.tobytes() and third.numpy().tobytes() == want.tobytes()
    assert r.rectify(rc.image(args2[4])).tobytes() == rr.remap(uv2, rc.image(args2[4])).tobytes()
