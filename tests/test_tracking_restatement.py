"""CPU: the numpy restatement of the feature tracker (tests/tracking_restatement.py) against its own per-pair formulation on
every seeded case, its invariants, and that the cases of tests/tracking_cases.py exercise what they say they do."""
import numpy as np
import pytest

import tracking_cases as tc
import tracking_restatement as tr

ALL = list(tc.VARIANTS)
SMALL = [(n, k) for n, k in ALL if n not in ("large", "image_67x101") or k == 0]


def _want(name, k):
    c = tc.variants(name)[k]
    return c, tc.want(c)


@pytest.mark.parametrize("name,k", SMALL)
def test_matches_the_per_pair_formulation(name, k):
    c, w = _want(name, k)
    if name in ("large", "image_67x101"):  # (the scalar loop is slow: a seeded sixth of the landmarks)
        sel = np.arange(len(c["points"]))[::6]
        c = dict(c, points=c["points"][sel], moving_desc=c["moving_desc"][sel])
        w = tc.want(c)
    corr, counters = tr.track_per_pair(c["points"], c["moving_desc"], c["fixed_pixels"], c["fixed_desc"], c["pose"], c["K"], c["rows"],
                                       c["cols"], **c["params"])
    assert corr.tobytes() == w["correspondences"].tobytes(), c["name"]
    assert counters == {n: w[n] for n in tr.COUNTERS}, c["name"]


@pytest.mark.parametrize("name,k", ALL)
def test_invariants(name, k):
    c, w = _want(name, k)
    corr = w["correspondences"]
    assert w["num_moving"] >= w["num_in_view"] >= w["num_with_candidate"] >= w["num_accepted"] >= w["num_mutual"] == len(corr)
    assert (np.diff(corr["moving_idx"]) > 0).all()
    if c["params"]["cross_check"]:
        assert len(np.unique(corr["fixed_idx"])) == len(corr)  # one to one
    else:
        assert w["num_mutual"] == w["num_accepted"]
    d = w["details"]
    assert np.array_equal(corr["response"], d["distance"][corr["moving_idx"]].astype(np.float32))
    assert (corr["response"] <= c["params"]["max_distance"]).all()
    if c["params"]["search_radius"] == 0:
        pix = d["rv"][corr["moving_idx"]] * c["cols"] + d["cu"][corr["moving_idx"]]
        assert np.array_equal(pix, c["fixed_pixels"][corr["fixed_idx"]])


def test_the_cases_exercise_what_they_claim():
    for n in (1, 63, 64, 65, 200):
        c = tc.case("lane_stride_%d" % n)
        rows = c["fixed_pixels"] // c["cols"]
        assert int(((rows >= 24) & (rows <= 40)).sum()) == n
        d = tc.want(c)["details"]
        assert d["in_view"].all() and (d["rv"] == 32).all() and d["num_candidates"].max() >= 1
    c = tc.case("second_best")
    w = tc.want(c)
    d = w["details"]
    assert (d["num_candidates"] == 130).all() and (d["distance"] == 3).all() and (d["second"] == 7).all()
    assert [int(b) for b in d["best"]] == [5, 7, 9, 75, 128, 31]
    assert w["num_accepted"] == 6 and tc.want(tc.with_params(c, min_margin=5))["num_accepted"] == 0
    c = tc.case("ties")
    d = tc.want(c)["details"]
    assert list(d["num_candidates"]) == [2, 1, 1, 1, 2] and d["second"][0] == d["distance"][0] == 6 and d["best"][0] == 0
    assert list(d["mutual"]) == [True, True, False, True, True]  # (of the twins 1 and 2 the lower index keeps the keypoint)
    assert d["best"][4] == 4 and d["second"][4] - d["distance"][4] == 4
    assert list(tc.want(tc.with_params(c, min_margin=1))["details"]["accepted"]) == [False, True, True, True, True]
    assert list(tc.want(tc.with_params(c, min_margin=4))["details"]["accepted"]) == [False, True, True, True, True]
    assert list(tc.want(tc.with_params(c, min_margin=5))["details"]["accepted"]) == [False, True, True, True, False]
    c = tc.case("view_edges")
    d = tc.want(c)["details"]
    assert list(d["in_view"]) == [True, False, False, True, True, False, True, True, False, True, False] + [False] * 7
    assert d["cu"][0] == 0 and d["cu"][3] == 47 and d["rv"][4] == 0 and d["rv"][6] == 7
    c = tc.case("cross")
    on, off = tc.want(c), tc.want(tc.with_params(c, cross_check=False))
    assert on["details"]["rv"][0] == on["details"]["rv"][1] and on["details"]["cu"][0] == on["details"]["cu"][1]
    assert list(on["details"]["mutual"]) == [True, True, False, True, False, True] and off["num_mutual"] == 6
    assert on["details"]["best"][2] == on["details"]["best"][3]
    c = tc.case("gates")
    assert list(tc.want(tc.with_params(c, max_distance=0))["correspondences"]["moving_idx"]) == [0, 1, 2, 4]
    assert list(tc.want(tc.with_params(c, search_radius=0, max_distance=256))["correspondences"]["moving_idx"]) == [0, 2, 3, 4]
    c = tc.case("large")
    w = tc.want(c)
    assert len(c["points"]) > tc.SCAN_TILE and 0 < w["num_mutual"] < w["num_accepted"] < w["num_with_candidate"] < w["num_in_view"] < len(c["points"])
    assert w["correspondences"]["moving_idx"].max() >= tc.SCAN_TILE  # (pairs behind the scan's first tile)
    c = tc.case("borders")
    d = tc.want(c)["details"]
    assert d["in_view"].all() and (d["num_candidates"] >= 1).all()
    # keypoints in the first and the last image row, and landmarks whose row band reaches each of them (and is cut there)
    kp_rows, R, last = c["fixed_pixels"] // c["cols"], c["params"]["search_radius"], c["rows"] - 1
    assert (kp_rows == 0).any() and (kp_rows == last).any()
    assert (d["rv"] - R < 0).any() and (d["rv"] + R > last).any() and (d["rv"] == 0).any() and (d["rv"] == last).any()
    assert c["rows"] == 40 and [v["params"]["search_radius"] for v in tc.variants("borders")[2:]] == [255, 0, 39, 40]
    for name in ("image_48x64", "image_67x101"):
        w = tc.want(tc.case(name))
        assert w["num_mutual"] >= 5, name


def test_to_merger_flips_and_globalises():
    corr = np.array([(4, 0, 3.0), (1, 2, 7.0)], tr.CORR_DTYPE)
    out = tr.to_merger(corr, [10, 11, 12])
    assert list(out["fixed_idx"]) == [10, 12] and list(out["moving_idx"]) == [4, 1] and list(out["response"]) == [3.0, 7.0]
    from srrg2_slam_interfaces_amd import mapping

    assert mapping.to_merger(corr, [10, 11, 12]).tobytes() == out.tobytes()
