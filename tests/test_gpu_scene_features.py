"""-m gpu: scenes that carry a 256-bit descriptor and an intensity per point (srrg2_scene_set_features): the features travel
with the point through clip, merge and append, and the descriptor database adds and matches a scene on the device.

The oracle (oracle/o_scene.c) knows no features and needs none: neither gate of the merge reads anything but coordinates and
the response, so the expected features come from the oracle BY PROVENANCE (tests/scene_provenance.py: a second oracle merge
with tagged normals tells which measurement point every output point carries; tests/test_scene_provenance.py checks that
helper on the CPU).  Coordinates and normals stay bit for bit the oracle's, as in tests/test_gpu_scene_merge.py."""
import ctypes as C

import numpy as np
import pytest

import hbst_restatement as hr
import scene_provenance as prov
from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn
from test_gpu_scene import _same_scene
from test_gpu_scene_merge import _corr, _flip, _merge, _pose, _to_meas

pytestmark = pytest.mark.gpu
f32 = np.float32
E_INVALID, E_STATE = -1, -5
FIELDS = ["descriptors", "intensity", "both"]


def _features(rng, n, fields):
    """(descriptors or None, intensity or None) for n points; the intensities include NaN, inf and -0.0 (compared as bytes)"""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8) if fields in ("descriptors", "both") else None
    i = None
    if fields in ("intensity", "both"):
        i = rng.uniform(-1, 1, n).astype(f32)
        i[::97], i[1::97], i[2::97] = np.nan, np.inf, -0.0
    return d, i


def _same_features(scene, want_d, want_i):
    d, i = scene.features()
    assert scene.has_features() == (want_d is not None, want_i is not None)
    assert (d is None) == (want_d is None) and (i is None) == (want_i is None)
    if d is not None:
        assert d.shape == want_d.shape and d.tobytes() == np.ascontiguousarray(want_d).tobytes()
    if i is not None:
        assert i.shape == want_i.shape and i.tobytes() == np.ascontiguousarray(want_i, f32).tobytes()


def _carried(src, scene_f, meas_f):
    return tuple(None if m is None else prov.carried(src, s, m) for s, m in zip(scene_f, meas_f))


def _clip(b, full, pose, range_max, clipped=None):
    clipped = clipped or mapping.Scene(b, full.dim)
    cl = mapping.SceneClipperBall(b, range_max=range_max)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    cl.compute()
    return cl.global_indices(), clipped


def _check_clip(b, full, pose, range_max, min_kept=20):
    """the clipped scene's features are those of the points it kept"""
    g, clipped = _clip(b, full, pose, range_max)
    assert min_kept < len(g) < full.size()
    d, i = full.features()
    _same_features(clipped, None if d is None else d[g], None if i is None else i[g])
    return clipped


def _hit_case(seed, dim, ns=5000, nm=4000):
    """a scene, a measurement and correspondences in which 300 scene points are hit 2 .. 5 times with mixed gate outcomes (a
    third of the responses above the gate, a fifth of the measurement points too far), the rest once; NaN points on both sides"""
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-3, 3, (ns, dim)).astype(f32)
    T = _pose(dim)
    times = rng.integers(2, 6, 300)
    s_multi = np.repeat(rng.permutation(ns)[:300], times)
    s_single = rng.permutation(np.setdiff1d(np.arange(ns), s_multi))[:2000]
    fixed = np.concatenate([s_multi, s_single])
    fixed = fixed[rng.permutation(len(fixed))]
    moving = rng.permutation(nm)[:len(fixed)]
    assert len(fixed) < nm
    noise = rng.normal(scale=0.05, size=(len(fixed), dim))
    far = rng.random(len(fixed)) < 0.2
    noise[far] *= 30.0
    mp = _to_meas(T, rng.uniform(-3, 3, (nm, dim)))
    mp[moving] = _to_meas(T, sp[fixed].astype(np.float64) + noise)
    mp[moving[7]] = np.nan
    mp[np.setdiff1d(np.arange(nm), moving)[:5]] = np.inf  # invalid points nobody hits: never appended
    sp[fixed[3]] = np.nan
    resp = rng.uniform(0, 75, len(fixed))
    counts = np.bincount(fixed, minlength=ns)
    assert set(np.unique(counts[counts > 1])) == {2, 3, 4, 5}
    return sp, mp, T, _corr(fixed, moving, resp), rng


# ---- 1. merge with explicit correspondences -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["target_not_reached", "target_reached", "no_correspondences"])
@pytest.mark.parametrize("fields", FIELDS)
@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("dim", [3, 2])
def test_merge_moves_the_features_with_the_points(oracle, product, dim, normals, fields, mode):
    sp, mp, T, corr, rng = _hit_case(200 + dim, dim)
    sn = rng.normal(size=sp.shape).astype(f32) if normals else None
    mn = rng.normal(size=mp.shape).astype(f32) if normals else None
    corr = None if mode == "no_correspondences" else corr
    params = mapping.MergerParams(50.0, 0.25, 100 if mode == "target_reached" else 10 ** 9)
    sf, mf = _features(rng, len(sp), fields), _features(rng, len(mp), fields)
    ob, b = oracle.scene_binding(), product.scene_binding(0)
    o_scene, o_meas, scene, meas = (mapping.Scene(x, dim) for x in (ob, ob, b, b))
    for s, m in ((o_scene, o_meas), (scene, meas)):
        s.set(sp, sn); m.set(mp, mn)
    scene.set_features(*sf)
    meas.set_features(*mf)
    _same_features(scene, *sf)
    ref = _merge(ob, o_scene, o_meas, T, corr, params)
    got = _merge(b, scene, meas, T, corr, params)
    assert got == ref and got["status"] == mapping.MERGER_SUCCESS
    _same_scene(o_scene, scene)  # coordinates and normals: bit for bit the oracle's, as without features
    src, coords, res = prov.provenance(oracle, dim, sp, mp, T, corr, params)
    assert res == ref and coords.tobytes() == scene.get()[0].tobytes()
    _same_features(scene, *_carried(src, sf, mf))
    if mode == "no_correspondences":
        assert got["num_added"] == np.isfinite(mp).all(axis=1).sum() and np.all(src[:len(sp)] < 0)
    else:
        assert got["num_merged"] > 500 and (got["num_added"] > 0) == (mode == "target_not_reached")
        # scene points hit several times: the last correspondence that PASSED decides, not the last one listed
        last = dict(zip(corr["fixed_idx"].tolist(), corr["moving_idx"].tolist()))
        multi = np.flatnonzero(np.bincount(corr["fixed_idx"], minlength=len(sp)) > 1)
        assert sum(src[s] >= 0 and src[s] != last[s] for s in multi) > 10 and sum(src[s] == last[s] for s in multi) > 10
    _same_features(meas, *mf)  # the measurement is only read
    _check_clip(b, scene, _pose(dim), 2.0)
    # a second merge into the merged scene: correspondences onto old and appended points
    n = scene.size()
    c2 = _corr(rng.integers(0, n, 3000), rng.integers(0, len(mp), 3000), rng.uniform(0, 60, 3000))
    before_p, before_f = scene.get()[0], scene.features()
    src2, coords2, _ = prov.provenance(oracle, dim, before_p, mp, T, c2, params)
    _merge(b, scene, meas, T, c2, params)
    assert coords2.tobytes() == scene.get()[0].tobytes()
    _same_features(scene, *_carried(src2, before_f, mf))


@pytest.mark.parametrize("fields", FIELDS)
@pytest.mark.parametrize("dim", [3, 2])
def test_an_empty_scene_adopts_the_measurements_fields(oracle, product, dim, fields):
    sp, mp, T, corr, rng = _hit_case(210 + dim, dim, ns=600, nm=3000)
    mf = _features(rng, len(mp), fields)
    b = product.scene_binding(0)
    scene, meas = mapping.Scene(b, dim), mapping.Scene(b, dim)
    meas.set(mp)
    meas.set_features(*mf)
    assert scene.has_features() == (False, False)
    params = mapping.default_merger_params()
    got = _merge(b, scene, meas, T, None, params)
    src, coords, res = prov.provenance(oracle, dim, np.zeros((0, dim), f32), mp, T, None, params)
    assert got == res and coords.tobytes() == scene.get()[0].tobytes()
    _same_features(scene, *_carried(src, tuple(None if f is None else f[:0] for f in mf), mf))


# ---- 2. the tracker's cycle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("fields", ["both", "descriptors"])
@pytest.mark.parametrize("dim", [3, 2])
def test_tracker_cycle_carries_the_features(oracle, product, dim, fields, prune):
    """clip -> align -> merge_from_aligner over three frames, everything on the device.  Per frame the provenance comes from the
    oracle's merge fed with the aligner's correspondences flipped and mapped through the clip's global indices
    (tracker_slice_processor_impl.cpp:160-186); a host-side twin applies it to the features, and the scene must equal the twin."""
    rng = np.random.default_rng(300 + dim)
    if dim == 3:
        kind, ident = abi.SE3_QUAT_RIGHT, syn.identity(3)
        poses = [syn.se3(np.array([0.05 * k, -0.03 * k, 0.01 * k]), np.deg2rad(np.array([0.6 * k, -0.4 * k, 0.8 * k]))) for k in range(4)]
        frames = []
        for k in range(4):
            P, N = syn.scene_3d(30_000, 300 + k)
            Xi = syn.se3_inv(poses[k])
            frames.append((np.ascontiguousarray(P @ Xi[:, :3].T + Xi[:, 3], f32), np.ascontiguousarray(N @ Xi[:, :3].T, f32)))
        cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 2e-5 if prune else 0.05)
    else:
        kind, ident = abi.SE2_RIGHT, syn.identity(2)
        poses = [syn.se2(0.08 * k, 0.03 * k, np.deg2rad(2.0 * k)) for k in range(4)]
        frames = [tuple(np.ascontiguousarray(a, f32) for a in syn.scan_2d(poses[k], beams=2000, sigma=0.005, seed=10 + k))
                  for k in range(4)]
        cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.5, abi.ROBUST_CAUCHY, 2e-5 if prune else 0.05)
    for fr in frames:  # invalid measurement points keep their index and never enter the scene
        fr[0][11::503] = np.nan
    feats = [_features(rng, len(fr[0]), fields) for fr in frames]
    params = mapping.MergerParams(50.0, 0.01, 10 ** 9)
    b = product.scene_binding(0)
    al = product.MultiAligner(kind)
    si = al.add_slice(cfg)
    al.set_params(keep_only_inlier_correspondences=prune)
    scene, clipped, meas = mapping.Scene(b, dim), mapping.Scene(b, dim), mapping.Scene(b, dim)
    mg = mapping.MergerCorrespondenceHomo(b, params)
    mg.set_scene(scene); mg.set_measurement(meas)
    # frame 0 starts the local map
    meas.set(*frames[0])
    meas.set_features(*feats[0])
    mg.set_measurement_in_scene(ident)
    mg.compute()
    src, coords, _ = prov.provenance(oracle, dim, np.zeros((0, dim), f32), frames[0][0], ident, None, params)
    twin = _carried(src, tuple(None if f is None else f[:0] for f in feats[0]), feats[0])
    assert coords.tobytes() == scene.get()[0].tobytes()
    _same_features(scene, *twin)
    robot_in_map = ident.astype(f32)
    for k in range(1, 4):
        meas.set(*frames[k])
        assert meas.has_features() == (False, False)  # srrg2_scene_set replaces the content
        meas.set_features(*feats[k])
        g, _ = _clip(b, scene, robot_in_map, 6.0, clipped)
        _same_features(clipped, *(None if f is None else f[g] for f in twin))
        cp, cn, n = clipped.device_arrays()
        al.set_cloud_device("set_moving", si, cp, 16, cn, 16, n)
        mp_, mn_, m = meas.device_arrays()
        al.set_cloud_device("set_fixed", si, mp_, 16, mn_, 16, m)
        al.set_moving_in_fixed(ident)
        al.compute()
        assert al.status() == abi.SUCCESS
        X = al.moving_in_fixed().astype(np.float64)
        if dim == 3:
            robot_in_map = (np.vstack([robot_in_map, [0, 0, 0, 1]]).astype(np.float64) @ np.linalg.inv(np.vstack([X, [0, 0, 0, 1]])))[:3].astype(f32)
        else:
            robot_in_map = (robot_in_map.astype(np.float64) @ np.linalg.inv(X)).astype(f32)
        flipped = _flip(al.correspondences(si), g)
        before = scene.get()[0]
        src, coords, ref = prov.provenance(oracle, dim, before, frames[k][0], robot_in_map, flipped, params)
        mg.set_measurement_in_scene(robot_in_map)
        got = mg.compute_from_aligner(al, si, clipped)
        assert got == ref and got["num_merged"] > 500 and got["scene_size"] == len(src)
        if prune:
            stats = al.iteration_stats()[-1]
            assert got["num_correspondences"] == stats["num_inliers"] < stats["num_correspondences"]
        assert coords.tobytes() == scene.get()[0].tobytes()
        twin = _carried(src, twin, feats[k])
        _same_features(scene, *twin)
        assert (src[:len(before)] >= 0).sum() > 500


# ---- 3. sizes past every launch cap, growth of the capacity ---------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_merge_with_features_past_every_launch_cap(oracle, product, dim):
    """the shape of test_gpu_scene_merge.test_merge_past_every_launch_cap: 700 k measurement points, 1.0 M correspondences of
    which 705 k hit a scene point more than once (one hub 5 000 times), shuffled; every grid-stride loop takes several trips
    in its feature-carrying instantiation, the append included; then a clip of the 650 k-point result"""
    rng = np.random.default_rng(40 + dim)
    ns, nm = 400_000, 700_000
    sp = rng.uniform(-50, 50, (ns, dim)).astype(f32)
    sn = rng.normal(size=(ns, dim)).astype(f32)
    T = (syn.se3(np.array([0.3, -0.2, 0.1]), np.deg2rad(np.array([1.0, 2.0, -3.0]))) if dim == 3
         else syn.se2(0.3, -0.2, np.deg2rad(-3.0))).astype(f32)
    fixed = np.concatenate([1 + rng.permutation(299_999), np.zeros(5000, np.int64), rng.integers(300_000, ns, 700_000)])
    moving = rng.integers(0, nm, len(fixed))
    order = rng.permutation(len(fixed))
    fixed, moving = fixed[order], moving[order]
    src_pt = rng.integers(0, ns, nm)
    src_pt[moving] = fixed
    mp = _to_meas(T, sp[src_pt].astype(np.float64) + rng.normal(scale=0.1, size=(nm, dim)))
    mp[::9973] = np.nan
    mn = rng.normal(size=(nm, dim)).astype(f32)
    arr = _corr(fixed, moving, rng.uniform(0, 60, len(fixed)))
    sf, mf = _features(rng, ns, "both"), _features(rng, nm, "both")
    ob, b = oracle.scene_binding(), product.scene_binding(0)
    for target in (10 ** 9, 1000):
        o_scene, o_meas, scene, meas = (mapping.Scene(x, dim) for x in (ob, ob, b, b))
        for s, m in ((o_scene, o_meas), (scene, meas)):
            s.set(sp, sn); m.set(mp, mn)
        scene.set_features(*sf)
        meas.set_features(*mf)
        params = mapping.MergerParams(50.0, 0.25, target)
        ref = _merge(ob, o_scene, o_meas, T, arr, params)
        got = _merge(b, scene, meas, T, arr, params)
        assert got == ref
        _same_scene(o_scene, scene)
        src, coords, res = prov.provenance(oracle, dim, sp, mp, T, arr, params)
        assert res == ref
        _same_features(scene, *_carried(src, sf, mf))
        if target == 1000:
            assert got["num_added"] == 0
        else:
            assert got["num_merged"] > 50_000 and got["num_added"] > 16_384 and got["scene_size"] > 524_288
            # (a ball that leaves out only the corners of the +-50 box: the scatter's loop over the scene takes several trips and
            # more than 2048 x 256 points are kept)
            clipped = _check_clip(b, scene, _pose(dim), 70.0 if dim == 3 else 65.0, min_kept=524_288)
            assert clipped.size() == len(clipped.global_indices())


@pytest.mark.parametrize("fields", FIELDS)
@pytest.mark.parametrize("dim", [3, 2])
def test_growth_keeps_the_old_points_features(oracle, product, dim, fields):
    """the shape of test_merge_growth_keeps_the_old_points: merges that each outgrow the scene's capacity, then one whose
    correspondences hit points of all three generations"""
    rng = np.random.default_rng(50 + dim)
    T = _pose(dim)
    sp = rng.uniform(-5, 5, (1000, dim)).astype(f32)
    b = product.scene_binding(0)
    scene, meas = mapping.Scene(b, dim), mapping.Scene(b, dim)
    scene.set(sp)
    twin = _features(rng, 1000, fields)
    scene.set_features(*twin)
    params = mapping.MergerParams(50.0, 0.25, 10 ** 9)
    sizes = [1000]
    for step, nm in enumerate((5000, 20_000, 30_000)):
        c = _corr(rng.integers(0, sizes[-1], 4000), rng.permutation(nm)[:4000], rng.uniform(0, 60, 4000))
        if step == 2:
            c["fixed_idx"][:3] = [0, 1500, sizes[-1] - 1]
            c["response"][:3] = 1.0
        current = scene.get()[0]
        mp = _to_meas(T, rng.uniform(-5, 5, (nm, dim)))
        mp[c["moving_idx"]] = _to_meas(T, current[c["fixed_idx"]].astype(np.float64) + rng.normal(scale=0.05, size=(4000, dim)))
        mf = _features(rng, nm, fields)
        meas.set(mp)
        meas.set_features(*mf)
        src, coords, ref = prov.provenance(oracle, dim, current, mp, T, c, params)
        got = _merge(b, scene, meas, T, c, params)
        assert got == ref and got["num_merged"] > 2000 and got["num_added"] > 0
        assert coords.tobytes() == scene.get()[0].tobytes()
        twin = _carried(src, twin, mf)
        _same_features(scene, *twin)
        sizes.append(got["scene_size"])
    assert sizes[1] > 1000 * 1.5 + 1024 and all(sizes[i + 1] > sizes[i] * 1.5 + 1024 for i in (1, 2)), sizes
    _check_clip(b, scene, _pose(dim), 3.0)


# ---- 4. the descriptor database fed from a scene --------------------------------------------------------------------------
def _same_match(a, b):
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.num_matches, b.num_matches)
    assert np.array_equal(a.map_counts, b.map_counts) and len(a.correspondences) == len(b.correspondences)
    for x, y in zip(a.correspondences, b.correspondences):
        assert x.tobytes() == y.tobytes()


def _scene_with(b, dim, pts, desc):
    s = mapping.Scene(b, dim)
    s.set(pts)
    s.set_features(desc)
    return s


@pytest.mark.parametrize("dim", [3, 2])
def test_database_add_and_match_from_a_scene(product, dim):
    """two databases: one fed with scenes on the device, one with scene.features() and the finite-coordinate mask on the host"""
    rng = np.random.default_rng(400 + dim)
    b = product.scene_binding(0)
    dev, host = product.DescriptorDatabase(0), product.DescriptorDatabase(0)
    D = hr.random_descriptors(rng, 6000)
    maps = []
    sizes = (1500, 2500, 0, 700, 600_000, 900)
    for k, n in enumerate(sizes):
        own = rng.integers(0, len(D), n)
        pts = rng.uniform(-5, 5, (n, dim)).astype(f32)
        if k == 3:
            pts[:] = np.nan  # an all-invalid scene: not added
        else:
            pts[rng.random(n) < 0.05] = np.nan
            pts[rng.random(n) < 0.02, dim - 1] = np.inf
        desc = np.concatenate([np.stack([hr.flip_bits(rng, D[i], int(rng.integers(0, 5))) for i in own[:3000]]),
                               D[own[3000:]]]) if n else np.zeros((0, 32), np.uint8)
        scene = _scene_with(b, dim, pts, desc)
        d, _ = scene.features()
        valid = np.isfinite(pts).all(axis=1)
        # the match before the add, as the detector does it
        for kw in (dict(), dict(max_distance=12.5, min_age=1, min_matches=40), dict(query_index=1, min_age=0, min_matches=0)):
            _same_match(dev.match_scene(scene, **kw), host.match(d, valid, **kw))
        i_dev, i_host = dev.add_scene(scene), host.add(d, valid)
        assert i_dev == i_host and (i_dev == -1) == (k in (2, 3)) and dev.size() == host.size()
        maps.append((scene, pts, desc))
    # (a map of 600 k points, ~93 % of them valid: more than 2048 x 256, so the staging kernels' loops take several trips)
    assert dev.size()[0] == 4 and dev.size()[1] > 524_288 + 4000
    # a scene changed after it was added: the database kept its copy
    scene, pts, desc = maps[0]
    query = _scene_with(b, dim, pts, desc)
    want = host.match(desc, np.isfinite(pts).all(axis=1), min_matches=100)
    assert 0 in want.indices.tolist()
    scene.set_features(hr.random_descriptors(rng, len(pts)))
    scene.set(rng.uniform(-5, 5, (10, dim)).astype(f32))
    _same_match(dev.match_scene(query, min_matches=100), want)
    # a query with fixed_idx past the invalid points: indices are the scene's, never compacted
    got = dev.match_scene(query, min_matches=100)
    c0 = got.correspondences[got.indices.tolist().index(0)]
    valid0 = np.flatnonzero(np.isfinite(pts).all(axis=1))
    assert set(c0["fixed_idx"].tolist()) <= set(valid0.tolist()) and c0["fixed_idx"].max() > len(valid0)
    # an empty query and an all-invalid one
    for q_pts in (np.zeros((0, dim), f32), np.full((50, dim), np.nan, f32)):
        q = _scene_with(b, dim, q_pts, hr.random_descriptors(rng, len(q_pts)) if len(q_pts) else np.zeros((0, 32), np.uint8))
        res = dev.match_scene(q)
        _same_match(res, host.match(q.features()[0], np.zeros(len(q_pts), np.uint8)))
        assert len(res) == 0 and dev.add_scene(q) == -1


# ---- 5. the HBST detector with scenes as input ----------------------------------------------------------------------------
def test_hbst_detector_with_scenes_equals_host_arrays(product):
    from test_hbst_detector_end_to_end import _detector, _world

    maps, q = _world(33)
    q["points"][q["valid"] == 0] = np.nan  # a scene's validity IS its coordinates
    maps[1]["points"][::41] = np.nan
    b = product.scene_binding(0)
    host, dev = _detector(product), _detector(product)
    scenes = []
    for m in maps:
        valid = np.isfinite(m["points"]).all(axis=1).astype(np.uint8)
        s = _scene_with(b, 3, m["points"], m["descriptors"])
        scenes.append(s)
        assert host.compute(m["graph_id"], m["points"], None, m["descriptors"], valid) == dev.compute(m["graph_id"], s) == []
        assert host.add_previous_query() == dev.add_previous_query() >= 0
    qs = _scene_with(b, 3, q["points"], q["descriptors"])
    want = host.compute(q["graph_id"], q["points"], None, q["descriptors"], q["valid"])
    got = dev.compute(q["graph_id"], qs)
    assert dev.indices() == host.indices() == [0, 1, 2, 3]
    _same_match(dev.last_match, host.last_match)
    assert dev.drops == host.drops and len(got) == len(want) == 2
    for a, w in zip(got, want):
        assert (a["source"], a["target"]) == (w["source"], w["target"])
        for key in ("measurement", "information", "pose_in_target", "correspondences"):
            assert a[key].tobytes() == w[key].tobytes(), key
        assert (a["num_inliers"], a["num_correspondences"], a["chi_inliers"]) == \
               (w["num_inliers"], w["num_correspondences"], w["chi_inliers"])
    assert dev.add_previous_query() == host.add_previous_query() == 5
    assert dev.add_previous_query() == -1  # registered already


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _raw_set_features(b, scene, d, ds, i, is_, n, mem=abi.MEM_HOST):
    return b.lib.srrg2_scene_set_features(scene._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int(ds),
                                          None if i is None else i.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(is_),
                                          C.c_int(n), C.c_int(mem))


@pytest.mark.parametrize("dim", [3, 2])
def test_refusals_leave_the_handles_unchanged(oracle, product, dim):
    sp, mp, T, corr, rng = _hit_case(600 + dim, dim, ns=3000, nm=4000)
    b = product.scene_binding(0)
    sf, mf = _features(rng, len(sp), "both"), _features(rng, len(mp), "both")
    scene, meas = mapping.Scene(b, dim), mapping.Scene(b, dim)
    scene.set(sp); meas.set(mp)
    scene.set_features(*sf); meas.set_features(*mf)
    d, i = sf
    # size mismatch, bad strides, bad mem: SRRG2_E_INVALID, the features stay
    assert _raw_set_features(b, scene, d, 32, i, 4, len(sp) - 1) == E_INVALID
    assert _raw_set_features(b, scene, d, 31, None, 4, len(sp)) == E_INVALID
    assert _raw_set_features(b, scene, None, 32, i, 2, len(sp)) == E_INVALID
    assert _raw_set_features(b, scene, None, 32, i, 6, len(sp)) == E_INVALID
    assert _raw_set_features(b, scene, d, 32, i, 4, len(sp), mem=7) == E_INVALID
    with pytest.raises(ValueError):
        scene.set_features(d[:-1])
    _same_features(scene, *sf)
    # feature presence that disagrees: SRRG2_E_STATE from both merges, nothing moved
    params = mapping.MergerParams(50.0, 0.25, 10 ** 9)
    before = scene.get()
    for keep in ((None, mf[1]), (mf[0], None), (None, None)):
        meas.set_features(*keep)
        out = mapping.MergeResult()
        Tc = np.ascontiguousarray(T, f32)
        rc = b.lib.srrg2_scene_merge(scene._h, meas._h, Tc.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(corr.ctypes.data),
                                     C.c_int(len(corr)), C.byref(params), C.byref(out))
        assert rc == E_STATE and b"disagree" in b.err()
        assert scene.size() == len(sp) and scene.get()[0].tobytes() == before[0].tobytes()
        _same_features(scene, *sf)
        _same_features(meas, *keep)
    bare = mapping.Scene(b, dim)
    bare.set(sp)
    meas.set_features(*mf)
    with pytest.raises(RuntimeError, match="disagree"):
        _merge(b, bare, meas, T, corr, params)
    assert bare.has_features() == (False, False) and bare.get()[0].tobytes() == before[0].tobytes()
    # ... and the valid call that follows gives the result of fresh handles
    got = _merge(b, scene, meas, T, corr, params)
    src, coords, ref = prov.provenance(oracle, dim, sp, mp, T, corr, params)
    assert got == ref and coords.tobytes() == scene.get()[0].tobytes()
    _same_features(scene, *_carried(src, sf, mf))
    # the database: a scene without descriptors (SRRG2_E_STATE), the database untouched
    db, fresh = product.DescriptorDatabase(0), product.DescriptorDatabase(0)
    lib = db._lib
    assert db.add_scene(meas) == 0 and fresh.add(mf[0], np.isfinite(mp).all(axis=1)) == 0
    first = db.match_scene(meas, query_index=5)
    only_intensity = mapping.Scene(b, dim)
    only_intensity.set(mp)
    only_intensity.set_features(None, mf[1])
    idx, K = C.c_int(7), C.c_int(7)
    for s in (bare, only_intensity):
        assert lib.srrg2_descriptor_db_add_scene(db._h, s._h, C.byref(idx)) == E_STATE
        assert lib.srrg2_descriptor_db_match_scene(db._h, s._h, 5, 25.0, 0, 0, C.byref(K)) == E_STATE
    assert lib.srrg2_descriptor_db_add_scene(db._h, None, C.byref(idx)) == E_INVALID
    assert lib.srrg2_descriptor_db_match_scene(db._h, meas._h, -1, 25.0, 0, 0, C.byref(K)) == E_INVALID
    assert lib.srrg2_descriptor_db_match_scene(db._h, meas._h, 5, float("nan"), 0, 0, C.byref(K)) == E_INVALID
    assert db.size() == fresh.size() == (1, int(np.isfinite(mp).all(axis=1).sum()))
    _same_match(db.match_scene(meas, query_index=5), first)
    _same_match(first, fresh.match(mf[0], np.isfinite(mp).all(axis=1), query_index=5))


def test_a_scene_on_another_device_is_refused(product):
    """SRRG2_E_INVALID for a scene that lives on another device than the database.  On a host with one device such a scene
    cannot exist: creating it is refused, which is all there is to check there."""
    from srrg2_slam_interfaces_amd import _capi

    rng = np.random.default_rng(7)
    db = product.DescriptorDatabase(0)
    if _capi.device_count() < 2:
        with pytest.raises(RuntimeError, match="bad device index"):
            mapping.Scene(product.scene_binding(1), 3)
        return
    pts, desc = rng.uniform(-1, 1, (100, 3)).astype(f32), hr.random_descriptors(rng, 100)
    other = _scene_with(product.scene_binding(1), 3, pts, desc)
    idx, K = C.c_int(7), C.c_int(7)
    assert db._lib.srrg2_descriptor_db_add_scene(db._h, other._h, C.byref(idx)) == E_INVALID
    assert db._lib.srrg2_descriptor_db_match_scene(db._h, other._h, 0, 25.0, 0, 0, C.byref(K)) == E_INVALID
    assert db.size() == (0, 0)
    assert db.add_scene(_scene_with(product.scene_binding(0), 3, pts, desc)) == 0


# ---- set_features layouts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_set_features_strided_and_device_input(product, mem):
    """interleaved records (descriptor at an odd byte offset, intensity behind it): what a PointIntensityDescriptor3f vector
    looks like through the C ABI; device_features() hands back what get_features() copies"""
    lib = product.scene_binding(0).lib
    rng = np.random.default_rng(70)
    n, stride = 20_000, 52
    b = product.scene_binding(0)
    pts = rng.uniform(-1, 1, (n, 3)).astype(f32)
    d, i = _features(rng, n, "both")
    rec = np.full((n, stride), 0xAB, np.uint8)
    rec[:, 12:16] = i.view(np.uint8).reshape(n, 4)
    rec[:, 17:49] = d
    scene = mapping.Scene(b, 3)
    scene.set(pts)
    dptr = None
    try:
        base, kind = rec.ctypes.data, abi.MEM_HOST
        if mem == "device":
            p = C.c_void_p()
            assert lib.srrg2_amd_device_malloc(C.c_size_t(rec.nbytes), C.byref(p)) == 0
            dptr = p.value
            assert lib.srrg2_amd_memcpy(C.c_void_p(dptr), C.c_void_p(rec.ctypes.data), C.c_size_t(rec.nbytes), C.c_int(1), None) == 0
            base, kind = dptr, abi.MEM_DEVICE
        b.check(lib.srrg2_scene_set_features(scene._h, C.cast(base + 17, C.POINTER(C.c_uint8)), C.c_int(stride),
                                             C.cast(base + 12, C.POINTER(C.c_float)), C.c_int(stride), C.c_int(n), C.c_int(kind)))
    finally:
        if dptr is not None:
            lib.srrg2_amd_device_free(C.c_void_p(dptr))
    _same_features(scene, d, i)
    dp, ip, m = scene.device_features()
    assert m == n and dp is not None and ip is not None
    back_d, back_i = np.zeros((n, 32), np.uint8), np.zeros(n, f32)
    for dst, src in ((back_d, dp), (back_i, ip)):
        assert lib.srrg2_amd_memcpy(C.c_void_p(dst.ctypes.data), C.cast(src, C.c_void_p), C.c_size_t(dst.nbytes), C.c_int(0), None) == 0
    assert back_d.tobytes() == d.tobytes() and back_i.tobytes() == i.tobytes()
    scene.set_features(None, None)  # both null: dropped
    assert scene.has_features() == (False, False) and scene.features() == (None, None)
    assert scene.device_features()[:2] == (None, None)


# ---- 7. scenes without features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_scenes_without_features_report_none(product, dim):
    sp, mp, T, corr, rng = _hit_case(700 + dim, dim, ns=3000, nm=4000)
    b = product.scene_binding(0)
    scene, meas = mapping.Scene(b, dim), mapping.Scene(b, dim)
    assert scene.has_features() == (False, False)
    scene.set(sp, rng.normal(size=sp.shape).astype(f32)); meas.set(mp)
    assert scene.has_features() == meas.has_features() == (False, False)
    _, clipped = _clip(b, scene, _pose(dim), 2.0)
    assert clipped.size() > 20 and clipped.has_features() == (False, False)
    _merge(b, scene, meas, T, corr, mapping.MergerParams(50.0, 0.25, 10 ** 9))
    assert scene.size() > len(sp) and scene.has_features() == meas.has_features() == (False, False)
    assert scene.features() == (None, None) and scene.device_features()[:2] == (None, None)
    # a clipped scene that carried features drops them when it next receives a feature-less clip
    scene.set_features(*_features(rng, scene.size(), "both"))
    _clip(b, scene, _pose(dim), 2.0, clipped)
    assert clipped.has_features() == (True, True)
    scene.set(sp)
    _clip(b, scene, _pose(dim), 2.0, clipped)
    assert clipped.has_features() == (False, False)
