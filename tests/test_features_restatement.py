"""CPU: the numpy restatement of the image-feature contract (tests/features_restatement.py) against the facts DESIGN.md section 4
"Image features" states, and the case file's promises (tests/features_cases.py).  Needs neither the library nor a GPU."""
import zlib

import numpy as np

import features_cases as fc
import features_restatement as fr


def test_pattern_generator():
    p, draws = fr.base_pattern(return_draws=True)
    assert draws == 260 and p.shape == (256, 4)
    assert p[:3].tolist() == [[-4, 2, 8, 1], [-4, -4, 9, -1], [-2, -3, -3, 1]]
    assert p[-1].tolist() == [7, 0, 2, -6]
    assert zlib.crc32(p.astype(np.int8).tobytes()) == 2693931087
    assert ((p[:, 0] ** 2 + p[:, 1] ** 2) <= 169).all() and ((p[:, 2] ** 2 + p[:, 3] ** 2) <= 169).all()
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()


def test_cos_sin_table_is_double_precision_rounding():
    t = fr.cos_sin_table()
    k = np.arange(32)
    assert np.array_equal(t[:, 0], np.round(16384.0 * np.cos(2.0 * np.pi * k / 32.0)).astype(np.int64))
    assert np.array_equal(t[:, 1], np.round(16384.0 * np.sin(2.0 * np.pi * k / 32.0)).astype(np.int64))
    assert sorted(set(np.abs(t).reshape(-1).tolist())) == [0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384]


def test_rotated_patterns_stay_within_twelve_and_collapse_where_stated():
    collapsed = {}
    for k in range(32):
        r = fr.rotated_pattern(k)
        assert np.abs(r).max() <= 12, k
        collapsed[k] = int(((r[:, 0] == r[:, 2]) & (r[:, 1] == r[:, 3])).sum())
    assert np.array_equal(fr.rotated_pattern(0), fr.base_pattern())
    assert {k for k, n in collapsed.items() if n} == {4, 12, 20, 28} and all(collapsed[k] == 2 for k in (4, 12, 20, 28))


def test_disc_has_709_pixels():
    d = fr.disc_offsets()
    assert d.shape == (709, 2) and len({tuple(v) for v in d.tolist()}) == 709
    assert (d[:, 0] ** 2 + d[:, 1] ** 2).max() == 225


def test_score_is_the_largest_passing_threshold():
    """the segment test written out literally, on a few pixels: passes at t iff score > t"""
    I = fc.image(48, 64).astype(np.int32)
    score = fr.fast_score(I.astype(np.uint8))
    assert score[:3].max() == 0 and score[-3:].max() == 0 and score[:, :3].max() == 0 and score[:, -3:].max() == 0
    rng = np.random.default_rng(3)
    for _ in range(60):
        r, c = int(rng.integers(3, 45)), int(rng.integers(3, 61))
        ring = np.array([I[r + dy, c + dx] for dx, dy in fr.CIRCLE])

        def passes(t):
            for sign in (1, -1):
                flags = sign * (ring - I[r, c]) > t
                if any(all(flags[(k + j) % 16] for j in range(9)) for k in range(16)):
                    return True
            return False

        s = int(score[r, c])
        assert not passes(s) and (s == 0 or passes(s - 1)), (r, c, s)


def test_hand_made_quadrant_image():
    o = fr.extract(fc.quadrant_image(), max_features=0)
    assert o["keypoints"].tolist() == [[544, 100, 4]]
    assert o["num_pixels"] == 33 * 33 and o["num_candidates"] == o["num_maxima"] == o["num_selected"] == o["scene_size"] == 1
    assert o["points"].tolist() == [[16.0, 16.0, 1.0]] and o["intensity"].tolist() == [200.0]
    assert o["descriptors"].shape == (1, 32) and o["global_indices"].tolist() == [544]
    m = fr.extract(fc.quadrant_image(mirrored=True), max_features=0)
    assert m["keypoints"].shape == (0, 3) and m["num_maxima"] == 0 and m["scene_size"] == 0
    assert fr.extract(np.zeros((32, 40), np.uint8))["scene_size"] == 0
    empty = fr.extract(np.zeros((0, 0), np.uint8))
    assert empty["status"] == 1 and empty["num_pixels"] == 0 and empty["descriptors"].shape == (0, 32)


def test_cap_on_the_tiled_image():
    img = fc.tiled_image()
    full, caps = fc.tie_caps(img)
    scores = full["keypoints"][:, 1]
    n = len(scores)
    classes, counts = np.unique(scores, return_counts=True)
    assert n == 121 and len(classes) == 11 and counts.min() == 6 and counts.max() == 24  # many equal scores
    for name, m in caps.items():
        o = fr.extract(img, max_features=m)
        kept = o["keypoints"]
        assert len(kept) == min(m, n) == o["num_selected"] and o["num_maxima"] == n, name
        assert np.all(np.diff(kept[:, 0]) > 0)  # pixel order
        if m >= n:
            assert np.array_equal(kept, full["keypoints"])
            continue
        # the definition, by sorting: higher scores first, of equal scores the earlier pixel
        order = np.lexsort((full["keypoints"][:, 0], -scores))[:m]
        assert np.array_equal(kept, full["keypoints"][np.sort(order)]), name
        assert np.array_equal(o["descriptors"], full["descriptors"][np.sort(order)])
    cut = scores[np.lexsort((full["keypoints"][:, 0], -scores))[caps["inside"] - 1]]
    assert (scores == cut).sum() > ((fr.extract(img, max_features=caps["inside"])["keypoints"][:, 1]) == cut).sum() > 0


def test_case_images_cover_every_orientation_bin():
    bins, total = set(), 0
    for name, img in fc.images():
        o = fr.extract(img, max_features=0)
        bins |= set(o["keypoints"][:, 2].tolist())
        total += o["scene_size"]
        assert o["scene_size"] > 0, name
    assert bins == set(range(32)) and total > 400
    big = fr.extract(fc.image(120, 160), max_features=128)
    assert big["scene_size"] == 128 and big["num_maxima"] > 128  # past one workgroup of waves, over several tile rows


def test_crops_share_keypoints_with_identical_descriptors():
    (oa, A), (ob, B) = fc.crops()
    a, b = fr.extract(A, max_features=0), fr.extract(B, max_features=0)
    cols = A.shape[1]
    where = {(int(p) // cols + oa[0], int(p) % cols + oa[1]): i for i, p in enumerate(a["global_indices"])}
    common = 0
    for j, p in enumerate(b["global_indices"]):
        i = where.get((int(p) // cols + ob[0], int(p) % cols + ob[1]))
        if i is None:
            continue
        common += 1
        assert np.array_equal(a["keypoints"][i, 1:], b["keypoints"][j, 1:]) and np.array_equal(a["descriptors"][i], b["descriptors"][j])
    assert common >= 60


def test_depth_gates_use_the_keypoints_own_pixel():
    img = fc.image(96, 128)
    for kind in ("u16", "f32"):
        d = fc.depth_for(img, kind)
        o = fr.extract(img, K=fc.CAMERA, max_features=0, depth=d)
        assert 0 < o["num_with_depth"] < o["num_selected"]
        import adaptor_restatement as ar

        ref = ar.adapt_depth_image(d, fc.CAMERA, col_gap=0, row_gap=0)
        assert ref["depth_valid"][o["global_indices"]].all()
        assert ar.same_bits(o["points"], ref["points"][o["global_indices"]])
    assert (fr.extract(img, K=fc.CAMERA, max_features=0)["points"][:, 2] == 1.0).all()
