"""CPU: the restatement of the scale-pyramid feature adaptor (tests/pyramid_restatement.py) against its own contract -- the
vectorised resampler against a per-pixel loop, the two properties the contract names, the level sizes and quotas, num_levels = 1
against the single-scale restatement, and the reason the pyramid exists: more correct matches under a change of scale.  Needs no GPU."""
import numpy as np
import pytest

import features_cases as fc
import features_restatement as fr
import pyramid_cases as pc
import pyramid_restatement as pr


@pytest.mark.parametrize("num,den", [(6, 5), (3, 2), (2, 1), (7, 5), (8, 7), (5, 3)])
def test_resampler_equals_the_per_pixel_loop(num, den):
    for rows, cols in ((33, 47), (40, 35)):
        img = fc.rectangles(rows, cols, 11 * num + den)
        got = pr.resample(img, num, den)
        assert got.shape == (rows * den // num, cols * den // num) and got.dtype == np.uint8
        assert np.array_equal(got, pr.resample_loop(img, num, den))


@pytest.mark.parametrize("num,den", pc.RATIOS)
def test_a_constant_image_stays_constant(num, den):
    for v in (0, 1, 127, 255):
        assert (pr.resample(np.full((37, 41), v, np.uint8), num, den) == v).all()


def test_two_to_one_is_the_rounded_mean_of_the_block():
    img = fc.rectangles(41, 53, 5)  # (odd sides: the last row and column are dropped)
    I = img.astype(np.int64)[:40, :52]
    want = (I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2
    assert np.array_equal(pr.resample(img, 2, 1), want)


def test_level_sizes_end_before_a_side_of_32():
    assert pr.level_sizes(48, 64, 4) == [(48, 64), (40, 53), (33, 44)]  # (the fourth would be 27 x 36)
    assert pr.level_sizes(67, 101, 4) == [(67, 101), (55, 84), (45, 70), (37, 58)]
    assert pr.level_sizes(67, 101, 4, 2, 1) == [(67, 101), (33, 50)]
    assert pr.level_sizes(33, 33, 2) == [(33, 33)] and pr.level_sizes(32, 40, 4) == [] and pr.level_sizes(0, 0, 4) == []
    assert len(pr.level_sizes(480, 640, 8)) == 8
    assert [im.shape for im in pr.build(fc.image(67, 101), 4)] == pr.level_sizes(67, 101, 4)


def test_quotas_sum_to_the_cap():
    for sizes in (pr.level_sizes(96, 128, 4), pr.level_sizes(480, 640, 8), pr.level_sizes(67, 101, 4, 2, 1), [(33, 33)]):
        areas = [r * c for r, c in sizes]
        for cap in (1, 2, 7, 50, 1000, 2 ** 31 - 1):
            q = pr.quotas(sizes, cap)
            assert sum(q) == cap and all(v >= 0 for v in q)
            assert all(q[l] == cap * areas[l] // sum(areas) for l in range(1, len(q)))
        assert pr.quotas(sizes, 0) == [0] * len(sizes)
    # areas 12288, 8480, 5808, 4015 of 30591: floors 2, 1, 1, 0 and the remainder 3 to level 0
    assert pr.quotas(pr.level_sizes(96, 128, 4), 7) == [5, 1, 1, 0]


def test_position_is_exact_at_level_0_and_a_block_centre_at_two_to_one():
    c = np.arange(50)
    assert np.array_equal(pr.position_q8(c, 0), 256 * c)
    assert np.array_equal(pr.position_q8(c, 1, 2, 1), 512 * c + 128)  # centre of columns 2c, 2c + 1
    assert np.array_equal(pr.position_q8(c, 2, 2, 1), 1024 * c + 384)


@pytest.mark.parametrize("depth", [None, "u16", "f32"])
def test_one_level_is_the_single_scale_restatement(depth):
    img = pc.image("67x101")
    d = None if depth is None else pc.depth_for("67x101", depth)
    for m in (0, 20):
        a = fr.extract(img, K=pc.CAMERA, max_features=m, depth=d)
        b = pr.extract_pyramid(img, K=pc.CAMERA, max_features=m, depth=d, num_levels=1)
        assert a["scene_size"] == b["scene_size"] > 5
        for k in ("points", "intensity", "descriptors", "global_indices"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert np.array_equal(a["keypoints"], b["keypoints"][:, :3])
        kp = b["keypoints"]
        assert not kp[:, 3].any() and np.array_equal(kp[:, 4], kp[:, 0]) and not kp[:, 7].any()
        assert np.array_equal(kp[:, 5], 256 * (kp[:, 0] % 101)) and np.array_equal(kp[:, 6], 256 * (kp[:, 0] // 101))
        for k in ("num_candidates", "num_maxima", "num_selected", "num_with_depth"):
            assert b[k] == [a[k]], k


def test_cases_put_keypoints_on_the_levels_they_name():
    assert pc.reference("48x64", 4, 6, 5)["num_with_depth"] == [14, 6, 0]
    assert pc.reference("67x101", 4, 6, 5)["num_with_depth"] == [41, 23, 11, 4]
    assert pc.reference("67x101", 4, 2, 1)["num_with_depth"] == [41, 0]
    assert pc.reference("quadrant", 2, 6, 5)["num_with_depth"] == [1]
    for case in pc.CASES:
        ref = pc.reference(*case)
        kp = ref["keypoints"]
        assert np.array_equal(np.bincount(kp[:, 3], minlength=ref["num_levels_built"]), ref["num_with_depth"])
        assert (np.diff(kp[:, 3]) >= 0).all()  # level-major
        for l in range(ref["num_levels_built"]):
            assert (np.diff(kp[kp[:, 3] == l, 4]) > 0).all()  # raster order within a level


def test_caps_of_each_kind():
    name, sizes = "96x128", pr.level_sizes(96, 128, 4)
    caps = pc.cap_settings(name)
    full = pc.reference(name, 4, 6, 5)
    zero = pc.reference(name, 4, 6, 5, caps["zero_quota"])
    assert zero["quota"][-1] == 0 and zero["num_selected"][-1] == 0 < full["num_maxima"][-1] == zero["num_maxima"][-1]
    assert zero["num_selected"] == [min(q, m) for q, m in zip(zero["quota"], zero["num_maxima"])]
    tie = pc.reference(name, 4, 6, 5, caps["tie"])
    assert tie["num_selected"] == [min(q, m) for q, m in zip(pr.quotas(sizes, caps["tie"]), full["num_maxima"])]
    above = pc.reference(name, 4, 6, 5, caps["above"])
    assert above["keypoints"].tobytes() == full["keypoints"].tobytes() and above["quota"] != full["quota"]


def test_upper_level_depth_holes_gate_upper_levels_only():
    for kind in ("u16", "f32"):
        d, punched = pc.upper_levels_depth("96x128", kind)
        full = pc.reference("96x128", 4, 6, 5)
        got = pr.extract_pyramid(pc.image("96x128"), K=pc.CAMERA, max_features=0, depth=d)
        assert len(punched) > 5 and got["num_with_depth"][0] == full["num_with_depth"][0]
        assert sum(got["num_with_depth"][1:]) < sum(full["num_with_depth"][1:]) and min(got["num_with_depth"][1:]) > 0


def test_a_pyramid_finds_more_correct_matches_under_a_change_of_scale():
    """B = A (120 x 160) resampled by s; mutual nearest neighbours within Hamming 64, correct within 3 s pixels.  Counts obtained
    (single scale -> 4 levels at 6/5): s = 7/5: 22 -> 86; s = 2/1: 4 -> 29."""
    found = {}
    for num, den in ((7, 5), (2, 1)):
        A, B = pc.scaled_pair(120, 160, 3, num, den)
        single, pyramid = pc.scale_counts(A, B, num, den)
        assert pyramid > single, (num, den, single, pyramid)
        found[(num, den)] = (single, pyramid)
    assert found == {(7, 5): (22, 86), (2, 1): (4, 29)}  # (integer arithmetic: the recorded counts are exact)
