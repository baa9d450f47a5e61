"""GPU: the image-feature and stereo adaptors (csrc/features.hip, csrc/stereo.hip) at camera resolutions, past the launch caps of
their grid-stride kernels (tests/image_large_cases.py says where the caps come from), BIT FOR BIT against the numpy restatements
with the helpers of tests/test_gpu_features.py and tests/test_gpu_stereo.py.  tests/test_image_large_cases.py proves on the CPU
that each case reaches the path it is here for:

  keypoints in trip 2 of k_feat_tie / k_feat_select / k_feat_scatter     test_features_bit_for_bit[vga], [odd]
  trips 3 and 4                                                          test_features_bit_for_bit[hd]
  the tie quota cut among the members past the cap                       test_tie_quota_cut_past_the_cap
  the depth gate at second-trip pixels                                   test_depth_gate_in_the_second_trip
  more left keypoints than k_stereo_count's grid has threads             test_stereo_bit_for_bit[odd_dense*]
  pitch != cols, partial tiles on both edges, hundreds of keypoint rows  the odd and hd cases of both

Not reached, on purpose: the 524 288-thread cap of blocks_for() in k_stereo_scatter (that many keypoints in one image; the row
table of csrc/desc_band.hip is launched without a cap) and the exclusive scan's second level (more than 4 194 304 pixels;
tests/test_gpu_scene_large.py drives it).

The device's share of every test is milliseconds; the time is the CPU restatements', computed once per case and parameter set in
image_large_cases and shared by the tests of a session (seconds on one core of the development machine: an extraction 0.3 to 0.9,
`odd` at threshold 0 2.6; match_banded 0.3 to 1.4).
"""
import ctypes as C

import numpy as np
import pytest

import adaptor_restatement as ar
import image_large_cases as lc
import test_gpu_features as tf
import test_gpu_stereo as ts
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping

pytestmark = pytest.mark.gpu
CAP = lc.FEAT_CAP
DEVICE = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
# name -> (fast_threshold, max_features) runs
FEATURE_RUNS = {"vga": ((20, 0), (20, 1000)), "odd": ((20, 0), (20, 1000), (0, 0)), "hd": ((20, 1000),)}


def _features(scene, name, threshold=20, max_features=0, depth_kind=None, device=False, pad=0):
    depth = None if depth_kind is None else lc.depth(name, depth_kind)
    ad, res = tf._extract(scene, lc.image(name), depth=depth, device=device, pad=pad, threshold=threshold, max_features=max_features)
    tf._check(scene, ad, res, lc.want_features(name, threshold, max_features, depth_kind),
              (name, threshold, max_features, depth_kind, device, pad))
    return ad, res


def _stereo(scene, name, kw, device=False, pad=0):
    ad, res = ts._run(scene, lc.image(name), lc.image(name, "right"), device=device, pad=pad, **kw)
    ts._check(scene, ad, res, lc.want_stereo(name, **kw), (name, kw, device, pad))
    return ad, res


@DEVICE
@pytest.mark.parametrize("name", sorted(FEATURE_RUNS))
def test_features_bit_for_bit(product, name, device):
    """keypoints in every trip of the grid-stride loops: points, intensities, descriptors, global indices, keypoint records and
    every counter (num_selected is summed over the trips); from device memory the capped run has rows at a larger stride"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    for threshold, max_features in FEATURE_RUNS[name]:
        _features(scene, name, threshold, max_features, device=device, pad=5 if device and max_features else 0)
        assert (scene.global_indices() >= CAP).any() and (scene.global_indices() < CAP).any()
    if name == "hd":
        assert set(lc.trip_of(scene.global_indices()).tolist()) == {0, 1, 2, 3}
    if name == "odd" and not device:  # rows at a larger stride from host memory too
        _features(scene, name, 20, 1000, pad=3)
    scene.close()


def test_keypoint_capacity_below_and_above_the_count(product):
    """keypoints_out takes what fits and no more, with thousands of keypoints on both sides of the cap"""
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    img, want = lc.image("vga"), lc.want_features("vga")
    n = want["scene_size"]
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = tf._adaptor()
    ad.camera.rows, ad.camera.cols = img.shape
    for capacity in (n - 700, n + 50):  # (the last 706 lie past the cap: the smaller capacity ends just inside them)
        buf = np.full((capacity + 1, 4), -7, np.int32)
        out = abi.FeatureResult()
        assert lib.srrg2_adapt_image_features(scene._h, C.c_void_p(img.ctypes.data), abi.IMAGE_U8, img.strides[0], None,
                                              abi.IMAGE_NONE, 0, abi.MEM_HOST, C.byref(ad.camera), C.byref(ad.params),
                                              buf.ctypes.data_as(C.POINTER(abi.Keypoint)), capacity, C.byref(out)) == 0
        got = min(capacity, n)
        assert np.array_equal(buf[:got, :3], want["keypoints"][:got]) and not buf[:got, 3].any() and (buf[got:] == -7).all()
        assert out.scene_size == out.num_selected == n
        assert np.array_equal(scene.global_indices(), want["global_indices"])
    scene.close()


@DEVICE
def test_tie_quota_cut_past_the_cap(product, device):
    """`tiled_large`: the cut class has 840 members below pixel FEAT_CAP and 80 past it.  `boundary` keeps them all; `past` ends
    the quota among the 80, whose ranks are the exclusive scan of k_feat_tie's flags across the trip boundary"""
    caps = lc.tiled_caps()
    scene = mapping.Scene(product.scene_binding(0), 3)
    _features(scene, "tiled_large", device=device)
    for which in ("boundary", "past"):
        ad, res = _features(scene, "tiled_large", 20, caps[which], device=device, pad=7 if which == "past" else 0)
        assert res["num_selected"] == caps[which] < res["num_maxima"]
        kp = ad.keypoints()
        assert (kp[:, 1] >= caps["cut"]).all()
        kept_past = int(((kp[:, 1] == caps["cut"]) & (kp[:, 0] >= CAP)).sum())
        assert kept_past == (caps["past_members"] if which == "boundary" else caps["past"] - caps["above"] - caps["below"])
    scene.close()


@DEVICE
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_depth_gate_in_the_second_trip(product, kind, device):
    """holes and out-of-range depths under second-trip keypoints; the kept points are the rows of srrg2_adapt_depth_image's
    organised output at those pixels, bit for bit"""
    name = "vga"
    b = product.scene_binding(0)
    scene, organised = mapping.Scene(b, 3), mapping.Scene(b, 3)
    ad, res = _features(scene, name, depth_kind=kind, device=device, pad=3 if device else 0)
    assert 0 < res["num_with_depth"] < res["num_selected"] == lc.want_features(name)["num_selected"]
    g = scene.global_indices()
    assert (g >= CAP).any() and (g < CAP).any()
    dp = adaptors.MeasurementAdaptorDepthImage(ad.camera)
    dp.params.normal_col_gap = dp.params.normal_row_gap = 0
    dp.params.compact = 0
    dp.set_meas(organised)
    dp.set_raw_data(lc.depth(name, kind))
    dp.compute()
    rows = organised.get()[0][g]
    assert np.isfinite(rows).all() and ar.same_bits(scene.get()[0], rows)
    scene.close(); organised.close()


@pytest.mark.parametrize("name,kw", lc.STEREO_CASES, ids=["vga", "odd_dense", "odd_dense_one_way", "hd_1000"])
def test_stereo_bit_for_bit(product, name, kw):
    """scene, matches, keypoints and all counters against match_banded, from host memory: two pipelines of FeatWork buffers and
    the second staging offset at camera sizes; `odd_dense*`: 21 407 left keypoints, k_stereo_count strides"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad, res = _stereo(scene, name, kw)
    if "fast_threshold" in kw:
        assert res["num_left"] > lc.STEREO_COUNT_CAP
    assert (scene.global_indices() >= CAP).any() and (scene.global_indices() < CAP).any()
    scene.close()


@pytest.mark.parametrize("name,kw", [lc.STEREO_CASES[0], lc.STEREO_CASES[1]], ids=["vga", "odd_dense"])
def test_stereo_from_device_memory_with_padded_strides(product, name, kw):
    """the two images at two different row strides, neither a multiple of 4 for `odd`: byte reads in k_feat_score_box"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    _stereo(scene, name, kw, device=True, pad=5)
    scene.close()


def test_stereo_record_capacities_below_the_count(product):
    """keypoints_out and matches_out smaller than the result, each by its own capacity"""
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    left, right = lc.image("vga"), lc.image("vga", "right")
    want = lc.want_stereo("vga")
    n = want["scene_size"]
    scene = mapping.Scene(product.scene_binding(0), 3)
    ad = ts._adaptor()
    ad.camera.rows, ad.camera.cols = left.shape
    for kcap, mcap in ((n - 300, 1000), (n + 9, n - 1)):
        kps = np.full((kcap + 1, 4), -7, np.int32)
        ms = np.full((mcap + 1, 4), -7, np.int32)
        out = abi.StereoResult()
        assert lib.srrg2_adapt_stereo_features(scene._h, C.c_void_p(left.ctypes.data), left.strides[0], C.c_void_p(right.ctypes.data),
                                               right.strides[0], abi.MEM_HOST, C.byref(ad.camera), C.byref(ad.params),
                                               C.byref(ad.stereo), kps.ctypes.data_as(C.POINTER(abi.Keypoint)), kcap,
                                               ms.ctypes.data_as(C.POINTER(abi.StereoMatch)), mcap, C.byref(out)) == 0
        gk, gm = min(kcap, n), min(mcap, n)
        assert np.array_equal(kps[:gk, :3], want["keypoints"][:gk]) and (kps[gk:] == -7).all()
        assert ms[:gm].tobytes() == want["matches"][:gm].tobytes() and (ms[gm:] == -7).all()
        assert out.scene_size == n and out.num_matched == want["num_matched"] and out.num_mutual == want["num_mutual"]
    scene.close()


def test_one_handle_across_the_large_shapes(product):
    """vga, odd, vga on one scene handle, features then stereo: the work buffers grow, are reused while larger than the image
    needs (odd has fewer pixels, at threshold 0 four times the keypoints), and serve the first image again"""
    scene = mapping.Scene(product.scene_binding(0), 3)
    for name, run in (("vga", (20, 0)), ("odd", (0, 0)), ("vga", (20, 1000)), ("odd", (20, 0)), ("vga", (20, 0))):
        _features(scene, name, *run)
    for name, kw in (lc.STEREO_CASES[0], lc.STEREO_CASES[1], lc.STEREO_CASES[0]):
        _stereo(scene, name, kw)
    _features(scene, "vga")  # (the stereo call left the feature buffers usable)
    scene.close()
