"""GPU: the dense stereo adaptor (csrc/stereo_dense.hip) at working sizes, past the launch caps of its grid-stride kernels
(tests/stereo_dense_large_cases.py says where the caps come from), BIT FOR BIT against the numpy restatement with the helpers of
tests/test_gpu_stereo_dense.py: the whole disparity image, the counters and the scene organised with gaps 1/1 (points, normals,
intensity, global indices).  tests/test_stereo_dense_large_cases.py proves on the CPU that each case reaches the path it is here
for:

  second trip of k_sd_finish and k_sd_census, padded strides, staging of 530 KB     test_caps_bit_for_bit[host], [device]
  third trip of both; the split between the two images inside a trip of the census  test_three_trips_from_device_memory
  three trips of k_sd_cost (paths = 0)                                              test_cost_volume_in_three_trips
  NJ = 1 at VGA on structured content: 474 lines of 568, 568 lines of 474           test_vga_two_planes
  NJ = 2 on 354 x 504; NJ = 4 on lines of 58 and 136; the winner in the last slot   test_wide_ranges[wide], [deep], [*_far]
  rectify -> dense stereo, queued, at VGA                                           test_queued_vga_pair_feeds_dense_stereo

Not reached, on purpose: a cost volume beyond 2^31 bytes (the kernels index it in 64 bits, no restatement follows it in test
time); 1280 x 720 with 128 disparities (19 s of restatement); k_sd_count's cap, which every 120 x 160 case of
tests/test_gpu_stereo_dense.py crosses already; k_sd_paths, k_sd_best and k_sd_right have no capped launch.

The device's share of every test is milliseconds; the time is the CPU restatement's, computed once per case and parameter set
(stereo_dense_cases.want's cache) and shared by the tests of a session.  Seconds on one core of the development machine: caps 1.1,
caps3 2.1, cost 0.25, vga 2.7 per parameter set, wide 3.5, deep / wide_far / deep_far 0.2 each, the VGA rig 3.3 (two maps, two
remaps and the dense restatement).
"""
import numpy as np
import pytest

import adaptor_restatement as ar
import stereo_dense_large_cases as lc
import stereo_dense_restatement as sd
import test_gpu_rectify as tr
import test_gpu_stereo_dense as td
from srrg2_slam_interfaces_amd import adaptors, mapping

pytestmark = pytest.mark.gpu
F = np.float32


def _same_image(got, want, what):
    """two images equal bit for bit; a failure names the number of differing pixels and the first of them (the byte-string
    comparison of td._check says the same of a small image, and takes minutes to explain itself on two megabytes)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    kind = {1: np.uint8, 4: np.uint32}[got.dtype.itemsize]
    differ = np.flatnonzero(got.view(kind).reshape(-1) != want.view(kind).reshape(-1))
    assert differ.size == 0, (what, "%d pixels differ, the first at flat index %d" % (differ.size, differ[0]))


def _hold(scene, name, kw, device, pad=0, dpad=0):
    left, right = lc.pair(name)
    want = lc.want(name, **kw)
    what = (name, kw, device, pad, dpad)
    _, res, buf = td._run(scene, left, right, device=device, pad=pad, dpad=dpad, **kw)
    _same_image(buf[:, :left.shape[1]], want["disparity"], what)
    td._check(scene, res, buf, want, what)
    return res


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_caps_bit_for_bit(product, device):
    """548 x 972: the second trip of k_sd_finish (Z, flag bytes and the caller's disparity image at the caller's stride) and of
    k_sd_census; both images in rows at larger, unequal strides -- from host memory a staging of (rows - 1) * stride + cols bytes
    each --, a padded disparity stride whose padding stays as it was; then packed"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    (kw,) = lc.runs("caps")
    res = _hold(scene, "caps", kw, device, pad=5, dpad=3)
    assert res["num_pixels"] > lc.SD_FINISH_CAP and 2 * res["num_pixels"] > lc.SD_CENSUS_CAP
    _hold(scene, "caps", kw, device)
    scene.close()


def test_three_trips_from_device_memory(product):
    """1088 x 972: the third trip of k_sd_finish and k_sd_census; the census index passes from the left image to the right one
    inside the second trip"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    (kw,) = lc.runs("caps3")
    res = _hold(scene, "caps3", kw, True, dpad=1)
    assert res["num_pixels"] > 2 * lc.SD_FINISH_CAP and 2 * res["num_pixels"] > 2 * lc.SD_CENSUS_CAP
    scene.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_cost_volume_in_three_trips(product, device):
    """paths = 0 on 200 x 300 with 64 disparities: k_sd_cost writes 2 830 848 elements in three trips, and k_sd_best, k_sd_right
    and k_sd_finish read them all"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    (kw,) = lc.runs("cost")
    res = _hold(scene, "cost", kw, device)
    assert res["num_evaluated"] * 64 > 2 * lc.SD_COST_CAP
    scene.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_vga_two_planes(product, device):
    """the workload's own shape, two planes and their occlusion: the defaults, then whole disparities under the strictest
    left-right check"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    for kw in lc.runs("vga"):
        _hold(scene, "vga", kw, device, pad=3 if device else 0)
    scene.close()


@pytest.mark.parametrize("name", ["wide", "deep", "wide_far", "deep_far"])
def test_wide_ranges(product, name):
    """two and four disparities per lane on rectangles that are neither narrow nor short: 128 on 354 x 504, 256 with vertical
    lines of 58 and horizontal ones of 136; `*_far`: the winner in every lane's last slot.  From host and device memory"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    (kw,) = lc.runs(name)
    for device in (False, True):
        _hold(scene, name, kw, device, dpad=2 if device else 0)
    scene.close()


def test_one_handle_across_the_large_shapes(product):
    """the workspaces grow, are reused while larger than the pair needs, and serve the first pair again: a volume written by
    NJ = 4 read as NJ = 1, a census array of a million words under an image of 25 600 pixels"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    for name in ("cost", "caps", "deep_far", "cost", "deep"):
        (kw,) = lc.runs(name)
        _hold(scene, name, kw, name != "caps")
    scene.close()


def test_queued_vga_pair_feeds_dense_stereo(product):
    """raw VGA pair -> rectify_pair(order_on = scene) -> srrg2_adapt_stereo_dense(out = NULL, organised, d 1 .. 64), settled by
    the first read of the scene: the rectified pair, the disparity, the scene and the counters are those of the composition of
    the two restatements"""
    import torch

    g = lc.vga_rig()
    rows, cols = g["shape"]
    s = product.StereoRectifier()
    s.set_calibration(g["K"], g["distortion"], g["K"], g["distortion"], lc.VGA_RIG_R, lc.VGA_RIG_T, g["shape"])
    assert np.array_equal(s.left.map(), g["maps"][0]) and np.array_equal(s.right.map(), g["maps"][1])
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = adaptors.MeasurementAdaptorStereoDense()
    s.camera(ad.camera)
    ad.stereo.baseline = s.baseline
    ad.stereo.min_disparity, ad.stereo.max_disparity = lc.VGA_RIG_RANGE["min_disparity"], lc.VGA_RIG_RANGE["max_disparity"]
    ad.set_meas(scene)
    assert (tr._camera9(ad.camera), float(F(s.baseline))) == lc.vga_rig_camera()
    want = lc.want_vga_rig(tr._camera9(ad.camera), float(F(s.baseline)))
    assert want["num_consistent"] > 100000 and want["num_valid"] > 50000
    disp = torch.full((rows, cols), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for source in ("host", "device"):
        if source == "host":
            dl, dr = s.rectify(*g["raw"], order_on=scene)
        else:
            kl, lp = tr._to_device(g["raw"][0])
            kr, rp = tr._to_device(g["raw"][1])
            dl, dr = s.rectify(lp, rp, order_on=scene)
        ad.set_raw_data(dl.pair, dr.pair)
        assert ad.compute(False, (disp.data_ptr(), 4 * cols)) is None  # only queued
        assert scene.size() == rows * cols  # the first read settles the chain
        torch.cuda.synchronize()
        _same_image(dl.numpy(), g["rectified"][0], (source, "left"))
        _same_image(dr.numpy(), g["rectified"][1], (source, "right"))
        _same_image(disp.cpu().numpy(), want["disparity"], (source, "disparity"))
        td._check_scene(scene, want, source)
        res = ad.compute(True, (disp.data_ptr(), 4 * cols))  # the same pair again, with the counters
        assert res == {k: want[k] for k in sd.COUNTERS}, (source, res)
        assert ar.same_bits(scene.get()[0], want["points"]), source
    scene.close()
