"""GPU: the feature tracker (srrg2_scene_track_features, csrc/tracking.hip) against the numpy restatement of its contract
(tests/tracking_restatement.py), BIT FOR BIT: the records (the float response's bits included) and every counter, on the seeded
cases of tests/tracking_cases.py (tests/test_tracking_restatement.py pins what they exercise); capacity, empty scenes, every
refusal with its code and untouched outputs; and one tracker frame end to end: extract -> clip -> track -> aligner with given
correspondences (against the oracle) -> merge (against the oracle).

Not reachable through the public API, hence not driven here: fixed global indices that do NOT ascend -- every producer of
global indices (the clippers, the adaptors, voxelize, estimate_normals) emits them ascending; the out-of-range half of the same
device check is driven (a measurement clipped from a larger image than the tracker is told)."""
import ctypes as C

import numpy as np
import pytest

import features_cases as fc
import tracking_cases as tc
import tracking_restatement as tr
from helpers import assert_same_run
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -4, -5
_SCENES = {}


def _fixed_scene(b, rows, cols, pixels, desc, points=None):
    """a measurement at arbitrary pixels without an image: a full scene of rows * cols points, NaN everywhere but at the chosen
    pixels, with descriptors, ball-clipped with the identity: the clip keeps the features and its global indices are the pixels"""
    n = rows * cols
    P = np.full((n, 3), np.nan, F)
    P[pixels] = np.stack([(pixels % cols) * 0.01, (pixels // cols) * 0.01, np.ones(len(pixels))], -1) if points is None else points
    D = np.zeros((n, 32), np.uint8)
    D[pixels] = desc
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    full.set(P)
    full.set_features(D)
    clip = mapping.SceneClipperBall(b, 1e6)
    clip.set_full_scene(full)
    clip.set_clipped_scene_in_robot(clipped)
    clip.set_robot_in_local_map(np.eye(3, 4, dtype=F))
    clip.compute()
    full.close()
    assert np.array_equal(clipped.global_indices(), pixels) and clipped.has_features()[0]
    return clipped


def _moving_scene(b, points, desc):
    s = mapping.Scene(b, 3)
    s.set(points)
    if len(points):
        s.set_features(desc)
    return s


def _scenes(product, name):
    """(binding, moving, fixed) of a case, built once and shared by its variants (the tracker leaves both as they are)"""
    if name not in _SCENES:
        b = product.scene_binding(0)
        c = tc.case(name)
        _SCENES[name] = (b, _moving_scene(b, c["points"], c["moving_desc"]),
                         _fixed_scene(b, c["rows"], c["cols"], c["fixed_pixels"].astype(np.int64), c["fixed_desc"]))
    return _SCENES[name]


def _params(c):
    p = mapping.default_track_params()
    for i, v in enumerate(c["K"]):
        p.camera_matrix[i] = v
    p.image_rows, p.image_cols = c["rows"], c["cols"]
    p.depth_min, p.depth_max = c["params"]["depth_min"], c["params"]["depth_max"]
    p.search_radius, p.max_distance, p.min_margin = (c["params"][k] for k in ("search_radius", "max_distance", "min_margin"))
    p.cross_check = int(c["params"]["cross_check"])
    return p


def _tracker(b, c, moving, fixed):
    ft = mapping.FeatureTracker(b, _params(c))
    ft.set_moving(moving)
    ft.set_fixed(fixed)
    ft.set_moving_in_sensor(c["pose"])
    return ft


def _same(got, result, want, what):
    assert result == {k: (0 if k == "reserved" else want[k]) for k in result}, (what, result)
    assert got.dtype == tr.CORR_DTYPE and got.tobytes() == want["correspondences"].tobytes(), what


@pytest.mark.parametrize("name,k", tc.VARIANTS)
def test_bit_for_bit_against_the_restatement(product, name, k):
    c = tc.variants(name)[k]
    b, moving, fixed = _scenes(product, name)
    ft = _tracker(b, c, moving, fixed)
    got = ft.compute()
    _same(got, ft.result, tc.want(c), c["name"])


def test_stability_and_untouched_scenes(product):
    c = tc.case("large")
    b, moving, fixed = _scenes(product, "large")
    ft = _tracker(b, c, moving, fixed)
    first, r1 = ft.compute().tobytes(), dict(ft.result)
    second, r2 = ft.compute().tobytes(), dict(ft.result)
    assert first == second and r1 == r2 and r1["num_correspondences"] > 0
    assert np.array_equal(fixed.global_indices(), c["fixed_pixels"]) and moving.size() == len(c["points"])
    assert moving.features()[0].tobytes() == c["moving_desc"].tobytes()


def _raw(b, moving, fixed, T, p, buf, cap, out):
    return b.fn("track_features")(moving, fixed, None if T is None else T.ctypes.data_as(C.POINTER(C.c_float)),
                                  None if p is None else C.byref(p), None if buf is None else C.c_void_p(buf.ctypes.data), C.c_int(cap),
                                  None if out is None else C.byref(out))


def test_capacity_null_buffer_and_null_result(product):
    c = tc.case("image_48x64")
    b, moving, fixed = _scenes(product, "image_48x64")
    w = tc.want(c)
    n = w["num_correspondences"]
    assert n >= 5
    ft = _tracker(b, c, moving, fixed)
    got = ft.compute(capacity=n - 3)  # below the count: the first records, the count unlimited
    assert got.tobytes() == w["correspondences"][:n - 3].tobytes() and ft.result["num_correspondences"] == n
    assert len(ft.compute(capacity=0)) == 0 and ft.result["num_correspondences"] == n  # capacity 0: a null buffer
    p, T = _params(c), np.ascontiguousarray(c["pose"], F)
    guard = np.full(3 * (n + 2), 0x5A5A5A5A, np.uint32)
    out = abi.TrackResult()
    b.check(_raw(b, moving._h, fixed._h, T, p, guard, n - 1, out))  # nothing behind min(capacity, count) records is written
    assert guard[:3 * (n - 1)].tobytes() == w["correspondences"][:n - 1].tobytes() and (guard[3 * (n - 1):] == 0x5A5A5A5A).all()
    b.check(_raw(b, moving._h, fixed._h, T, p, None, 5, out))  # a null buffer with room announced
    assert out.num_correspondences == n
    buf = np.zeros(n, tr.CORR_DTYPE)
    b.check(_raw(b, moving._h, fixed._h, T, p, buf, n, None))  # a null result
    assert buf.tobytes() == w["correspondences"].tobytes()
    assert ft.compute(want_result=False).tobytes() == w["correspondences"].tobytes() + bytes(12 * (moving.size() - n))


def test_empty_scenes(product):
    c = tc.case("ties")
    b, moving, fixed = _scenes(product, "ties")
    empty = mapping.Scene(b, 3)
    empty.set(np.zeros((0, 3), F))
    ft = _tracker(b, c, empty, fixed)
    assert len(ft.compute()) == 0
    assert ft.result == dict(num_moving=0, num_fixed=len(c["fixed_pixels"]), num_in_view=0, num_with_candidate=0, num_accepted=0,
                             num_mutual=0, num_correspondences=0, reserved=0)
    ft = _tracker(b, c, moving, empty)
    assert len(ft.compute()) == 0
    w = tr.track(c["points"], c["moving_desc"], np.zeros(0, np.int64), np.zeros((0, 32), np.uint8), c["pose"], c["K"], c["rows"],
                 c["cols"], **c["params"])
    assert w["num_in_view"] == len(c["points"])
    _same(ft.compute(), ft.result, w, "empty fixed")


def test_every_refusal_leaves_the_outputs_alone(product):
    c = tc.case("ties")
    b, moving, fixed = _scenes(product, "ties")
    T = np.ascontiguousarray(c["pose"], F)
    other = mapping.Scene(b, 2)
    other.set(np.zeros((3, 2), F))
    bare = _moving_scene(b, c["points"], None)
    bare.set_features(None, np.ones(len(c["points"]), F))  # intensity only: no descriptors
    unindexed = _moving_scene(b, c["points"], c["moving_desc"])  # Scene.set leaves no global indices
    big = _fixed_scene(b, c["rows"] + 2, c["cols"], np.r_[c["fixed_pixels"], (c["rows"] + 1) * c["cols"] + 3].astype(np.int64),
                       np.r_[c["fixed_desc"], c["fixed_desc"][:1]])  # the last pixel lies outside the tracker's image

    def mutated(**kw):
        p = _params(c)
        for k, v in kw.items():
            if k.startswith("K"):
                p.camera_matrix[int(k[1:])] = v
            else:
                setattr(p, k, v)
        return p

    def bad_pose(v):
        X = T.copy()
        X[1, 2] = v
        return X

    good = _params(c)
    calls = [(E_INVALID, None, fixed._h, T, good, 8), (E_INVALID, moving._h, None, T, good, 8), (E_INVALID, moving._h, fixed._h, None, good, 8),
             (E_INVALID, moving._h, fixed._h, T, None, 8), (E_INVALID, moving._h, moving._h, T, good, 8),
             (E_INVALID, other._h, fixed._h, T, good, 8), (E_INVALID, moving._h, other._h, T, good, 8),
             (E_INVALID, moving._h, fixed._h, T, good, -1), (E_INVALID, moving._h, fixed._h, bad_pose(np.nan), good, 8),
             (E_INVALID, moving._h, fixed._h, bad_pose(np.inf), good, 8), (E_UNSUPPORTED, moving._h, fixed._h, T, mutated(K1=0.5), 8),
             (E_STATE, bare._h, fixed._h, T, good, 8), (E_STATE, moving._h, bare._h, T, good, 8), (E_STATE, moving._h, unindexed._h, T, good, 8),
             (E_INVALID, moving._h, big._h, T, good, 8)]
    for kw in (dict(image_rows=0), dict(image_cols=-1), dict(image_rows=65536, image_cols=65536), dict(K0=0.0), dict(K4=float("nan")),
               dict(K0=float("inf")), dict(depth_min=0.0), dict(depth_min=float("nan")), dict(depth_min=2.0, depth_max=1.0),
               dict(depth_max=float("nan")), dict(search_radius=-1), dict(search_radius=256), dict(max_distance=-1), dict(max_distance=257),
               dict(min_margin=-1), dict(min_margin=257), dict(cross_check=2), dict(cross_check=-1), dict(reserved=1)):
        calls.append((E_INVALID, moving._h, fixed._h, T, mutated(**kw), 8))
    for code, m, f, X, p, cap in calls:
        guard = np.full(3 * 8, 0x5A5A5A5A, np.uint32)
        out = abi.TrackResult(*([-7] * 8))
        rc = _raw(b, m, f, X, p, guard, cap, out)
        assert rc == code, (rc, code, b.err())
        assert (guard == 0x5A5A5A5A).all() and out.as_dict() == dict.fromkeys(out.as_dict(), -7), code
    ft = _tracker(b, c, moving, fixed)  # the scenes still work
    _same(ft.compute(), ft.result, tc.want(c), "after the refusals")


def test_a_keypoint_with_a_non_finite_point_still_matches(product):
    """an image adaptor without a depth image and with cx = inf leaves keypoints whose points are not finite"""
    c = tc.case("image_48x64")
    b, moving, _ = _scenes(product, "image_48x64")
    meas = mapping.Scene(b, 3)
    ad = adaptors.MeasurementAdaptorImageFeatures()
    ad.set_camera_matrix((60.0, 0.0, np.inf, 0.0, 60.0, 23.5, 0.0, 0.0, 1.0))
    ad.params.max_features = 0
    ad.set_meas(meas)
    ad.set_raw_data(fc.image(48, 64))
    ad.compute()
    assert not np.isfinite(meas.get()[0]).all(axis=1).any()
    assert np.array_equal(meas.global_indices(), c["fixed_pixels"]) and meas.features()[0].tobytes() == c["fixed_desc"].tobytes()
    ft = _tracker(b, c, moving, meas)
    got = ft.compute()
    assert len(got) >= 5
    _same(got, ft.result, tc.want(c), "non-finite keypoint points")


def test_tracker_frame_end_to_end(oracle, product):
    rows, cols = 67, 101
    K = (80.0, 0.0, 50.0, 0.0, 80.0, 33.0, 0.0, 0.0, 1.0)
    img, depth = fc.image(rows, cols), fc.depth_for(fc.image(rows, cols), "u16")
    b = product.scene_binding(0)

    def extract():
        s = mapping.Scene(b, 3)
        ad = adaptors.MeasurementAdaptorImageFeatures()
        ad.set_camera_matrix(K)
        ad.params.max_features = 0
        ad.set_meas(s)
        ad.set_raw_data(img, depth)
        ad.compute()
        return s

    A, meas = extract(), extract()  # frame A becomes the map, the same image again the measurement
    pa, pix_a = A.get()[0], A.global_indices().astype(np.int64)
    da, ia = A.features()
    n = len(pa)
    assert n >= 30
    W = syn.se3(np.array([0.4, -0.2, 0.3]), np.deg2rad([4.0, -7.0, 11.0]))  # the sensor in the map
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)  # (the map's order is not the image's)
    map_pts = (pa.astype(np.float64) @ W[:, :3].T + W[:, 3]).astype(F)[perm]
    world = mapping.Scene(b, 3)
    world.set(map_pts)
    world.set_features(da[perm], ia[perm])
    clipped = mapping.Scene(b, 3)
    clip = mapping.SceneClipperBall(b, 100.0)
    clip.set_full_scene(world)
    clip.set_clipped_scene_in_robot(clipped)
    clip.set_robot_in_local_map(np.eye(3, 4, dtype=F))
    clip.compute()
    g = clipped.global_indices()
    guess = syn.se3_mul(syn.se3(np.array([0.02, -0.015, 0.01]), np.deg2rad([0.3, -0.2, 0.4])), syn.se3_inv(W))  # a little off
    p = mapping.default_track_params()
    for i, v in enumerate(K):
        p.camera_matrix[i] = v
    p.image_rows, p.image_cols, p.search_radius, p.max_distance, p.min_margin = rows, cols, 8, 32, 1
    ft = mapping.FeatureTracker(b, p)
    ft.set_fixed(meas)
    ft.set_moving(clipped)
    ft.set_moving_in_sensor(guess[:3])
    corr = ft.compute()
    assert len(corr) >= n // 2, ft.result
    # every pair is a true pair: the landmark that came from pixel q is matched to the keypoint at pixel q
    assert np.array_equal(pix_a[perm[g[corr["moving_idx"]]]], meas.global_indices()[corr["fixed_idx"]])
    # the aligner on these pairs: the HIP library against the oracle
    kind = abi.SE3_QUAT_RIGHT
    cfg = abi.default_slice_config(kind)
    cfg.kind, cfg.finder = abi.SLICE_P2P, abi.FINDER_CORRESPONDENCES
    fixed_pts, moving_pts = meas.get()[0], clipped.get()[0]
    runs = []
    for al in (oracle.OracleAligner(kind), product.MultiAligner(kind)):
        al.set_params(max_iterations=8)
        si = al.add_slice(cfg)
        al.set_fixed(si, fixed_pts, None)
        al.set_moving(si, moving_pts, None)
        al.set_correspondences(si, corr)
        al.set_moving_in_fixed(syn.identity(al.dim))
        assert al.compute() == abi.SUCCESS
        runs.append(al)
    assert_same_run(*runs)
    assert np.max(np.abs(runs[1].moving_in_fixed() - syn.se3_inv(W)[:3])) < 1e-3
    # the merge of the flipped pairs: the HIP library against the oracle
    flipped = mapping.to_merger(corr, g)
    assert flipped.tobytes() == tr.to_merger(corr, g).tobytes()
    results = []
    for side in (oracle.scene_binding(), b):
        scene, m = (mapping.Scene(side, 3), mapping.Scene(side, 3)) if side is not b else (world, meas)
        if side is not b:
            scene.set(map_pts)
            m.set(fixed_pts)
        mg = mapping.MergerCorrespondenceHomo(side)
        mg.set_scene(scene)
        mg.set_measurement(m)
        mg.set_measurement_in_scene(W[:3])
        mg.set_correspondences(flipped)
        results.append(mg.compute())
    assert results[0] == results[1] and results[1]["num_merged"] > 0, results
