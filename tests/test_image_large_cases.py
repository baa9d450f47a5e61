"""CPU: the images, caps and references of tests/image_large_cases.py are what they claim to be -- before
tests/test_gpu_image_large.py holds the device to them.  Crossing a launch cap exercises nothing unless keypoints lie behind it (a
416 x 640 image crosses FEAT_CAP and its margin keeps every keypoint below it), so every case is pinned by where its keypoints
fall; the row-banded stereo restatement equals the all-pairs one bit for bit on every case the all-pairs one can take.  Needs no
GPU and no library."""
import numpy as np
import pytest

import features_cases as fc
import features_restatement as fr
import image_large_cases as lc
import stereo_cases as sc
import stereo_restatement as sr

CAP = lc.FEAT_CAP


def test_constants():
    assert CAP == 262_144 and lc.STEREO_COUNT_CAP == 16_384
    assert {n: lc.image(n).shape for n in lc.FEATURE_NAMES} == {"vga": (480, 640), "odd": (563, 509), "hd": (723, 1283),
                                                                "tiled_large": (576, 504)}
    # trips of the grid-stride loops
    assert {n: -(-lc.image(n).size // CAP) for n in lc.FEATURE_NAMES} == {"vga": 2, "odd": 2, "hd": 4, "tiled_large": 2}
    # the image that crosses the cap and exercises nothing: the last admissible pixel of 416 x 640 lies below the cap
    assert 416 * 640 > CAP and (416 - fr.MARGIN - 1) * 640 + (640 - fr.MARGIN - 1) < CAP
    # pitch != cols and partial tiles on both edges for odd and hd; vga is whole tiles
    assert lc.pitch_of(640) == 640 and 480 % lc.TILE_H == 0
    assert lc.pitch_of(509) == 512 and 563 % lc.TILE_H != 0 and lc.pitch_of(1283) == 1344 and 723 % lc.TILE_H != 0
    for name in lc.FEATURE_NAMES:
        assert lc.image(name).dtype == np.uint8 and lc.image(name).flags.c_contiguous


# (name, fast_threshold, max_features): the runs tests/test_gpu_image_large.py makes on the rectangle images
FEATURE_RUNS = [("vga", 20, 0), ("vga", 20, 1000), ("odd", 20, 0), ("odd", 20, 1000), ("odd", 0, 0), ("hd", 20, 1000)]


@pytest.mark.parametrize("name,threshold,max_features", FEATURE_RUNS)
def test_feature_cases_keep_keypoints_on_both_sides_of_the_cap(name, threshold, max_features):
    img = lc.image(name)
    assert img.size > CAP
    w = lc.want_features(name, threshold, max_features)
    g = w["global_indices"].astype(np.int64)
    per_trip = np.bincount(lc.trip_of(g), minlength=4)
    print(name, threshold, max_features, w["num_maxima"], per_trip)
    assert (np.diff(g) > 0).all() and w["scene_size"] == w["num_selected"] == len(g)
    assert per_trip[0] >= 100 and per_trip[1] >= 50  # below the cap, and at or past it
    if max_features:
        # the cap cuts, and keeps keypoints of the later trips (where the cut class lies is `tiled_large`'s business)
        assert w["num_selected"] == max_features < w["num_maxima"]
    if name == "hd":
        assert (per_trip >= 100).all()  # each of the four trips
    else:
        assert per_trip[2:].sum() == 0
    if (name, threshold) == ("odd", 0):
        assert len(g) > lc.STEREO_COUNT_CAP


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("name", lc.DEPTH_NAMES)
def test_depth_gate_drops_and_keeps_second_trip_keypoints(name, kind):
    d = lc.depth(name, kind)
    assert d.shape == lc.image(name).shape and d.dtype == (np.uint16 if kind == "u16" else np.float32)
    selected = lc.want_features(name)["global_indices"]  # without depth: every selected keypoint
    w = lc.want_features(name, depth_kind=kind)
    kept = w["global_indices"]
    assert w["num_selected"] == len(selected) and 0 < w["num_with_depth"] == len(kept) < w["num_selected"]
    dropped = np.setdiff1d(selected, kept)
    assert len(dropped) + len(kept) == len(selected)
    assert (dropped >= CAP).sum() >= 50 and (kept >= CAP).sum() >= 50 and (dropped < CAP).any() and (kept < CAP).any()
    # every way of failing the gate lies under some second-trip keypoint
    raw = d.reshape(-1)[dropped[dropped >= CAP]]
    if kind == "u16":
        assert {0, 200, 60000} <= set(raw.tolist())
    else:
        assert np.isnan(raw).any() and np.isinf(raw).any() and (raw == np.float32(0.1)).any() and (raw < 0).any()


def test_tiled_large_cuts_inside_the_members_past_the_cap():
    img = lc.image("tiled_large")
    assert img.size > CAP and np.array_equal(img[:96, :120], fc.tiled_image())
    caps = lc.tiled_caps()
    print(caps)
    full = lc.want_features("tiled_large")
    other, named = fc.tie_caps(img)
    assert named["boundary"] == caps["boundary"] and np.array_equal(other["keypoints"], full["keypoints"])
    pix, score = full["keypoints"][:, 0].astype(np.int64), full["keypoints"][:, 1]
    cut = caps["cut"]
    members = pix[score == cut]
    # the cut class straddles the cap
    assert caps["below"] == (members < CAP).sum() >= 100 and caps["past_members"] == (members >= CAP).sum() >= 10
    assert caps["boundary"] == caps["above"] + len(members) and caps["boundary"] < len(pix)  # the cap cuts at all
    assert caps["above"] + caps["below"] < caps["past"] < caps["boundary"]
    for which, quota in (("boundary", len(members)), ("past", caps["past"] - caps["above"])):
        w = lc.want_features("tiled_large", 20, caps[which])
        got, s = w["keypoints"][:, 0].astype(np.int64), w["keypoints"][:, 1]
        assert len(got) == caps[which] and s.min() == cut
        kept = got[s == cut]
        assert np.array_equal(kept, members[:quota])  # the first of the class in raster order
        rejected = members[quota:]
        if which == "boundary":
            assert len(rejected) == 0 and (kept >= CAP).sum() == caps["past_members"]
        else:  # kept and rejected members of the cut class both exist past the cap
            assert (kept >= CAP).sum() >= 10 and len(rejected) >= 10 and (rejected >= CAP).all()
        assert np.array_equal(got[s > cut], pix[score > cut])


def _same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert a == b, what


def test_match_banded_equals_the_all_pairs_restatement():
    """every array, every counter and every entry of `details`, on every case of stereo_cases.all_cases() and on the degenerate
    pairs -- the licence to use match_banded where the all-pairs table does not fit in memory"""
    cases = sc.all_cases() + [("blank", dict()), ("32x40", dict()), ("0x0", dict())]
    seen = dict(tied=0, long_band=0, unmatched=0, one_sided=0)
    for name, kw in cases:
        want = sc.want(name, **kw)
        got = lc.match_banded(*sc.named(name), sc.CAMERA, sc.BASELINE, extracted=(want["left"], want["right"]),
                              **dict(kw, max_features=kw.get("max_features", 0)))
        assert set(got) == set(want) and set(got["details"]) == set(want["details"])
        for k in want:
            if k in ("details", "left", "right"):
                continue
            _same(got[k], want[k], (name, kw, k))
        for k in want["details"]:
            _same(got["details"][k], want["details"][k], (name, kw, "details", k))
        d = want["details"]
        seen["tied"] += int(d["tied"].sum())
        seen["long_band"] += int((d["band_size"] > 64).sum())
        seen["unmatched"] += int((d["best"] < 0).sum())
        seen["one_sided"] += int((d["matched"] & ~d["mutual"]).sum())
    assert all(v > 0 for v in seen.values()), seen
    # ... and extracting by itself: the same defaults
    left, right = sc.named("48x64")
    a, b = lc.match_banded(left, right, sc.CAMERA, sc.BASELINE), sr.match(left, right, sc.CAMERA, sc.BASELINE)
    assert a["matches"].tobytes() == b["matches"].tobytes() and a["num_left"] == b["num_left"] > 0


# Row bands of more than 64 candidates (a second pass of the band search's wave) need the keypoints for it: `hd` under its cap of
# 1000 has fewer than two per row and cannot; `vga` and `odd` must.
@pytest.mark.parametrize("name,kw", lc.STEREO_CASES, ids=["vga", "odd_dense", "odd_dense_one_way", "hd_1000"])
def test_stereo_cases_discriminate(name, kw):
    left, right = lc.image(name), lc.image(name, "right")
    assert right.shape == left.shape and right.dtype == np.uint8
    r0, r1, d = sc.bands(left.shape[0])[0]
    assert r1 - r0 == sc.BAND_ROWS and np.array_equal(right[r0:r1, :-d], left[r0:r1, d:])
    w = lc.want_stereo(name, **kw)
    det = w["details"]
    print(name, kw, {k: w[k] for k in sr.COUNTERS}, int(det["band_size"].max()))
    if kw.get("fast_threshold", 20) == 0:
        assert w["num_left"] > lc.STEREO_COUNT_CAP  # k_stereo_count's second trip
        # ... and the counters would miss it: matched and mutual keypoints lie past the cap
        assert det["matched"][lc.STEREO_COUNT_CAP:].sum() >= 100 and det["mutual"][lc.STEREO_COUNT_CAP:].sum() >= 100
    if kw.get("cross_check", True):
        assert w["num_left"] > w["num_matched"] > w["num_mutual"] > w["num_in_range"] > 0
    else:  # (without the cross check every matched keypoint is mutual)
        assert w["num_left"] > w["num_matched"] == w["num_mutual"] > w["num_in_range"] > 0
    assert w["scene_size"] == w["num_in_range"] == len(w["matches"]) >= 400
    if name != "hd":
        assert (det["band_size"] > 64).any()
    # kept matches on both sides of the feature cap, for hd in every trip: the scatter and the records of a stereo call
    per_trip = np.bincount(lc.trip_of(w["global_indices"]), minlength=4)
    assert (per_trip[:4 if name == "hd" else 2] >= 20).all(), per_trip
    # the second image's own pipeline: keypoints of the right image past the cap too
    assert (w["right"]["global_indices"] >= CAP).sum() >= 50
    assert (det["tied"] & det["kept"]).any()  # the tie rule decides something


def test_band_tables_stay_small():
    """the largest table match_banded forms: one row's keypoints against one band, with their 32 descriptor bytes as int64"""
    w = lc.want_stereo("odd", **lc.DENSE)
    rows = w["details"]["left_pixel"] // lc.image("odd").shape[1]
    per_row = np.bincount(rows).max()
    assert per_row * int(w["details"]["band_size"].max()) * 32 * 8 < 100 * 2 ** 20  # bytes; the all-pairs table: 91 GiB
