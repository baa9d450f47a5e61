"""CPU: the stereo cases themselves (tests/stereo_cases.py) under the restatement (tests/stereo_restatement.py) -- that they
exercise every gate, the long row bands, the ties and both outcomes of the sub-pixel step, so that the GPU comparison
(tests/test_gpu_stereo.py) cannot pass vacuously; that the band-shifted pairs give back their disparities; and that the scene is
what the image-feature restatement gives under the depth image of the matches.  Needs no GPU and no library."""
import numpy as np

import adaptor_restatement as ar
import features_restatement as fr
import stereo_cases as sc
import stereo_restatement as sr

F = np.float32


def _all():
    return [(name, kw, sc.want(name, **kw)) for name, kw in sc.all_cases()]


def test_the_cases_exercise_every_path():
    seen = dict(mutual=0, disparity_gate=0, distance_gate=0, cross_check=0, depth_gate=0, long_band=0, tie=0, offset=0, flat=0)
    for name, kw, w in _all():
        d = w["details"]
        sub = kw.get("subpixel", True)
        seen["mutual"] = max(seen["mutual"], w["num_mutual"])
        seen["disparity_gate"] += int(((d["band_size"] > 0) & (d["num_candidates"] == 0)).sum())
        seen["distance_gate"] += int(((d["best"] >= 0) & ~d["matched"]).sum())
        seen["cross_check"] += int((d["matched"] & ~d["mutual"]).sum())
        seen["depth_gate"] += int((d["mutual"] & ~d["kept"]).sum())
        if kw.get("fast_threshold", 20) == 0 and kw.get("row_tolerance", 1) >= 2:
            seen["long_band"] += int((d["band_size"] > 64).sum())
        seen["tie"] += int((d["tied"] & d["kept"]).sum())
        if sub:
            seen["offset"] += int((d["kept"] & (d["disparity"] != np.round(d["disparity"]))).sum())
            seen["flat"] += int((d["kept"] & (d["curvature"] <= 0)).sum())
    assert seen["mutual"] >= 20, seen
    for what in ("disparity_gate", "distance_gate", "cross_check", "depth_gate", "long_band", "tie", "offset", "flat"):
        assert seen[what] > 0, (what, seen)


def test_a_tie_goes_to_the_smaller_pixel_index():
    """the tiled pair: the partner repeats every 24 columns with the same descriptor; of the two candidates at distance 0 the one
    further left (the larger disparity) is taken"""
    w = sc.want("tiled", max_disparity=40, cross_check=False)
    d = w["details"]
    tied = d["tied"] & d["kept"] & (d["distance"] == 0)
    assert tied.sum() >= 10
    cols = sc.named("tiled")[0].shape[1]
    disp = d["left_pixel"][tied] % cols - d["right_pixel"][d["best"][tied]] % cols
    assert (disp == sc.TILED_DISPARITY + 24).all()
    # ... and with the second candidate outside the disparity gate the first one is found
    d2 = sc.want("tiled", max_disparity=20)["details"]
    both = tied & d2["kept"]
    assert both.sum() >= 10
    assert (d2["left_pixel"][both] % cols - d2["right_pixel"][d2["best"][both]] % cols == sc.TILED_DISPARITY).all()


def test_the_one_column_gate_is_used_in_both_directions():
    """min_disparity == max_disparity: with the cross check there are mutual matches (right -> left finds the column c + d),
    and left keypoints whose best is taken by another left keypoint (right -> left decides, not left -> right alone); every
    candidate lies in exactly that column, and without the cross check exactly the rejected ones come back"""
    on, off = (sc.want(sc.ONE_COLUMN_PAIR, **kw) for kw in sc.ONE_COLUMN)
    assert sc.ONE_COLUMN[0]["cross_check"] and not sc.ONE_COLUMN[1]["cross_check"]
    d = on["details"]
    rejected = d["matched"] & ~d["mutual"]
    assert on["num_mutual"] >= 1 and rejected.sum() >= 1, (on["num_mutual"], int(rejected.sum()))
    cols = sc.named(sc.ONE_COLUMN_PAIR)[0].shape[1]
    has = d["best"] >= 0
    assert (d["left_pixel"][has] % cols - d["right_pixel"][d["best"][has]] % cols == sc.ONE_COLUMN_DISPARITY).all()
    assert off["num_matched"] == on["num_matched"] and off["num_mutual"] == on["num_mutual"] + int(rejected.sum())


def test_interior_matches_recover_the_band_disparity():
    """a left keypoint whose 31 x 31 window lies in one band and whose partner lies inside the right image's margin: distance 0,
    the band's disparity -- exactly without the sub-pixel step, within half a pixel with it"""
    checked = 0
    for name, _, _ in sc.pairs():
        left, _ = sc.named(name)
        rows, cols = left.shape
        for kw in (dict(), dict(subpixel=False), dict(row_tolerance=0), dict(cross_check=False)):
            w = sc.want(name, **kw)
            d = w["details"]
            right_pixels = set(int(p) for p in d["right_pixel"])
            for i in range(len(d["best"])):
                r, c = divmod(int(d["left_pixel"][i]), cols)
                band, interior = sc.band_of(rows, r)
                if not interior or c - band < 16:
                    continue
                assert r * cols + c - band in right_pixels, (name, kw, r, c)  # the partner is a keypoint of the right image
                assert d["distance"][i] == 0 and d["matched"][i] and d["mutual"][i], (name, kw, r, c)
                got = c - int(d["right_pixel"][d["best"][i]]) % cols
                assert got == band, (name, kw, r, c, got, band)
                if kw.get("subpixel", True):
                    assert abs(float(d["disparity"][i]) - band) <= 0.5
                    assert d["costs"][i][1] == 0
                else:
                    assert d["disparity"][i] == F(band)
                assert d["z"][i] == F(sc.CAMERA[0]) * F(sc.BASELINE) / d["disparity"][i]
                assert bool(d["kept"][i]) == (0.4 <= float(d["z"][i]) <= 8.0)
                checked += 1
    assert checked >= 100


def test_the_scene_is_the_feature_scene_under_the_depth_image_of_the_matches():
    """(6) of the contract: extract() on the left image with an F32 depth image holding z at the matched pixels and 0 elsewhere
    gives the stereo scene, bit for bit"""
    for name, kw, w in _all():
        left, _ = sc.named(name)
        rows, cols = left.shape
        depth = sr.depth_image_of(w["matches"], rows, cols, sc.CAMERA, sc.BASELINE)
        fkw = {k: kw[k] for k in ("fast_threshold", "oriented") if k in kw}
        e = fr.extract(left, K=sc.CAMERA, max_features=0, depth=depth, **fkw)
        assert e["scene_size"] == w["scene_size"], (name, kw)
        assert ar.same_bits(e["points"], w["points"]), (name, kw)
        assert np.array_equal(e["global_indices"], w["global_indices"]) and np.array_equal(e["keypoints"], w["keypoints"])
        assert e["descriptors"].tobytes() == w["descriptors"].tobytes() and e["intensity"].tobytes() == w["intensity"].tobytes()


def test_counters_and_degenerate_pairs():
    for name, kw, w in _all():
        assert w["num_left"] >= w["num_matched"] >= w["num_mutual"] >= w["num_in_range"] == w["scene_size"] == len(w["matches"])
        if not kw.get("cross_check", True):
            assert w["num_matched"] == w["num_mutual"]
        assert (np.diff(w["global_indices"]) > 0).all() and (w["matches"]["disparity"] > 0).all()
        assert np.array_equal(w["matches"]["left_pixel"], w["global_indices"])
    blank = sc.want("blank")
    assert blank["num_left"] > 0 and blank["num_right"] == 0 and blank["num_matched"] == 0 and blank["scene_size"] == 0
    assert blank["status"] == 0
    small = sc.want("32x40")
    assert small["num_left"] == small["num_right"] == small["scene_size"] == 0 and small["status"] == 0
    none = sc.want("0x0")
    assert none["status"] == 1 and none["num_pixels"] == 0 and none["scene_size"] == 0


def test_the_cap_cuts_each_image_on_its_own():
    """a cap inside a class of equal scores (features_cases.tie_caps on the left image of the tiled pair): both images keep
    exactly that many keypoints, and fewer matches survive than without the cap"""
    import features_cases as fc

    left, _ = sc.named("tiled")
    _, caps = fc.tie_caps(left)
    w = sc.want("tiled", max_features=caps["inside"], max_disparity=20)
    assert w["num_left"] == caps["inside"] and w["num_right"] == caps["inside"]
    assert 0 < w["scene_size"] < sc.want("tiled", max_disparity=20)["scene_size"]
