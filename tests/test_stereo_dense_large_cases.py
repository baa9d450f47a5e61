"""CPU: the pairs, caps and references of tests/stereo_dense_large_cases.py are what they claim to be -- before
tests/test_gpu_stereo_dense_large.py holds the device to them.  Crossing a launch cap exercises nothing unless pixels of the
processed rectangle lie behind it (540 x 972 crosses both caps and its last 592 pixels lie in the margin of 3 rows: the second
trip would write zeros only), so every case is pinned by what the restatement leaves behind each threshold.  Needs no GPU and no
library."""
import numpy as np
import pytest

import stereo_dense_cases as dc
import stereo_dense_large_cases as lc
import stereo_dense_restatement as sd


def test_constants_and_geometry():
    assert lc.SD_CENSUS_CAP == 1_048_576 and lc.SD_FINISH_CAP == 524_288 and lc.SD_COST_CAP == 1_048_576
    assert [lc.slots(nd) for nd in (1, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4]
    for name in lc.CASES:
        left, right = lc.pair(name)
        assert left.dtype == right.dtype == np.uint8 and left.shape == right.shape and left.flags.c_contiguous
        for kw in lc.runs(name):
            assert lc.geometry(name, kw) == lc.GEOMETRY[name], name
    # trips of the three grid-stride loops
    n = {name: lc.pair(name)[0].size for name in lc.CASES}
    assert (n["caps"], n["caps3"]) == (532_656, 1_057_536)
    assert -(-n["caps"] // lc.SD_FINISH_CAP) == 2 and -(-2 * n["caps"] // lc.SD_CENSUS_CAP) == 2
    assert -(-n["caps3"] // lc.SD_FINISH_CAP) == 3 and -(-2 * n["caps3"] // lc.SD_CENSUS_CAP) == 3
    assert lc.SD_CENSUS_CAP < n["caps3"] < 2 * lc.SD_CENSUS_CAP  # the split between the two images lies inside trip 2
    H, W, nd, _ = lc.GEOMETRY["cost"]
    assert H * W * nd == 2_830_848 and -(-H * W * nd // lc.SD_COST_CAP) == 3
    # the shapes that cross the caps and exercise nothing: their pixels past the thresholds lie below the rectangle
    for rows, at in ((540, lc.SD_FINISH_CAP), (1080, 2 * lc.SD_FINISH_CAP)):
        assert rows * 972 > at and at // 972 >= rows - 3


@pytest.mark.parametrize("name", ["caps", "caps3"])
def test_caps_leave_disparities_behind_every_threshold(name):
    """k_sd_finish: consistent pixels with a disparity, not all equal, in every trip; k_sd_census: defined census words of the
    right image (and for caps3 of the left one) in every trip past the first"""
    left, right = lc.pair(name)
    rows, cols = left.shape
    n = rows * cols
    (kw,) = lc.runs(name)
    w = lc.want(name, **kw)
    disp, ok = w["disparity"].reshape(-1), w["consistent"].reshape(-1)
    trips = 2 if name == "caps" else 3
    for t in range(trips):
        a, b = t * lc.SD_FINISH_CAP, min((t + 1) * lc.SD_FINISH_CAP, n)
        late = disp[a:b][ok[a:b]]
        print(name, "finish trip", t, "consistent", late.size, "distinct", len(np.unique(late)))
        assert late.size >= 1000 and (late != 0).all() and len(np.unique(late)) > 10
        # the points of the scene come from Z at those pixels
        assert np.isfinite(w["points"].reshape(n, 3)[a:b]).all(1).sum() >= 1000
    # most of the noise finds its shift
    assert w["num_consistent"] > 0.9 * w["num_evaluated"] and np.median(np.rint(disp[ok])) == lc.CASES[name][1]
    words = np.concatenate([sd.census(left).reshape(-1), sd.census(right).reshape(-1)])  # in the order of k_sd_census's index
    for t in range(1, trips):
        a, b = t * lc.SD_CENSUS_CAP, min((t + 1) * lc.SD_CENSUS_CAP, 2 * n)
        defined = words[a:b][words[a:b] != 0]
        print(name, "census trip", t, "words", b - a, "defined", defined.size)
        assert defined.size >= 5000 and len(np.unique(defined)) > 1000
        # ... that the result depends on: they belong to rows of the rectangle
        first_row = (a - n if a >= n else a) // cols
        assert 3 <= first_row < rows - 4
    if name == "caps3":  # trip 2 holds the end of the left image and the start of the right one
        assert words[lc.SD_CENSUS_CAP:n].any() and words[n:2 * lc.SD_CENSUS_CAP].any()


def test_cost_volume_elements_of_every_trip_belong_to_matched_pixels():
    """paths = 0: S = C, and on noise shifted by 20 the cost at d = 20 is 0 wherever the window lies in the copied columns --
    everywhere in the rectangle: the best disparity is the shift but for ties at cost 0"""
    (kw,) = lc.runs("cost")
    w = lc.want("cost", **kw)
    shift = lc.CASES["cost"][1]
    ev, best = w["evaluated"].reshape(-1), w["best"].reshape(-1)
    for t in range(3):
        a = t * lc.SD_COST_CAP
        pix = lc.volume_pixels("cost", kw, a, min(a + lc.SD_COST_CAP, 2_830_848))
        on = (best[pix] == shift).mean()
        print("cost trip", t, "pixels", pix.size, "best is the shift %.4f" % on)
        # (a pixel that is the darkest of its window has the census word 0, and so has now and then a right pixel at a smaller
        # d: cost 0 there too, and the smaller d wins -- under 1 % of the pixels)
        assert pix.size >= 8000 and ev[pix].all() and on >= 0.98
        assert w["consistent"].reshape(-1)[pix].sum() >= 8000
    assert w["num_evaluated"] == 194 * 228 and w["num_consistent"] > 0.95 * w["num_evaluated"]


def test_vga_is_structured_and_the_restatement_finds_it():
    """of the visible, consistent pixels at least 99.9 % round to the truth (a condition on the input); the occlusion leaves
    unique pixels that the left-right check turns down"""
    left, right, truth, visible = dc.two_plane(480, 640)
    assert np.array_equal(left, lc.pair("vga")[0]) and np.array_equal(right, lc.pair("vga")[1])
    rect = np.zeros((480, 640), bool)
    rect[3:477, 4 + 64:636] = True
    for kw in lc.runs("vga"):
        w = lc.want("vga", **kw)
        seen = visible & rect & w["consistent"]
        right_on = np.rint(w["disparity"][seen]) == truth[seen]
        print("vga", kw, "visible and consistent", int(seen.sum()), "on the truth %.4f %%" % (100.0 * right_on.mean()))
        assert seen.sum() > 0.9 * (visible & rect).sum() and right_on.mean() >= 0.999
        assert (w["unique"] & ~w["consistent"]).sum() >= 100
        assert w["num_evaluated"] == 474 * 568
        # both planes are there
        assert (np.rint(w["disparity"][seen]) == dc.FOREGROUND).sum() > 10000 and (np.rint(w["disparity"][seen]) == dc.BACKGROUND).sum() > 10000
    a, b = (lc.want("vga", **kw)["disparity"] for kw in lc.runs("vga"))
    assert not np.array_equal(a, b)  # the second parameter set decides something


@pytest.mark.parametrize("name", ["wide", "deep", "wide_far", "deep_far"])
def test_wide_ranges_land_in_their_slot_count(name):
    (kw,) = lc.runs(name)
    H, W, nd, nj = lc.geometry(name, kw)
    assert (H, W, nd, nj) == lc.GEOMETRY[name] and 64 * (nj // 2) < nd <= 64 * nj
    w = lc.want(name, **kw)
    shift = lc.CASES[name][1]
    ok = w["consistent"]
    print(name, {k: w[k] for k in sd.COUNTERS})
    assert w["num_evaluated"] == H * W and w["num_consistent"] > 0.9 * H * W
    assert np.median(w["best"][ok]) == shift
    # (z = 26.25 / 100 and / 200 lies before the depth gate of 0.4 m: the `*_far` cases are held by the disparity image and the
    # counters, their scene is the organised one without a point)
    assert w["num_valid"] == 0 if name.endswith("_far") else w["num_valid"] > 1000
    # the winner lies in the first slot, where the later slots hold the candidates it has to beat, or (`*_far`) in the last one
    assert (shift - kw["min_disparity"]) // lc.WAVE == (nj - 1 if name.endswith("_far") else 0)


def test_vga_rig_rectifies_to_a_pair_dense_stereo_can_use():
    g = lc.vga_rig()
    assert g["shape"] == (480, 640) and all(img.shape == (480, 640) and img.dtype == np.uint8 for img in g["raw"] + g["rectified"])
    assert not np.array_equal(g["raw"][0], g["ideal"][0])  # the lens and the tilt do something
    # the rectified left image is the ideal one again where the map is valid, up to the two interpolations
    close = np.abs(g["rectified"][0].astype(int) - g["ideal"][0].astype(int)) <= 48
    assert close[40:440, 60:580].mean() > 0.9
    w = lc.want_vga_rig()
    print("vga rig", {k: w[k] for k in sd.COUNTERS})
    assert w["num_evaluated"] == 474 * 568 and w["num_consistent"] > 100000 and w["num_valid"] > 50000
    d = np.rint(w["disparity"][w["consistent"]])
    assert (d == dc.BACKGROUND).sum() > 50000 and (d == dc.FOREGROUND).sum() > 10000
