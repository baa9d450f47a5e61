"""CPU: the clouds and references of tests/scene_large_cases.py are what they claim to be -- before tests/test_gpu_scene_large.py
holds the device to them.  The scan cases' intended masks are the oracle's clip; the clipper cases cross the launch cap in what
they keep; the vectorised voxelize equals the loop restatement bit for bit; the normals clouds, at a twentieth of the size, give
every class of point."""
import numpy as np
import pytest

import clip_projective_restatement as cr
import clip_scan_restatement as cs
import normals_restatement as nr
import scene_large_cases as lc
import voxel_cases as vc
import voxel_restatement as vr
from srrg2_slam_interfaces_amd import mapping

F = np.float32
T, CAP = lc.T, lc.CAP


def test_constants():
    assert T == 2048 and CAP == 524_288 and lc.N_CAP == CAP + 2 * T + 1
    assert lc.SCAN_SIZES == (4_194_304, 4_194_305, 8_390_657)
    # trips of the one workgroup over the tile sums: exactly one; a second for one sum; a third for two
    assert [(-(-n // T), -(-(-(-n // T)) // T)) for n in lc.SCAN_SIZES] == [(2048, 1), (2049, 2), (4098, 3)]


@pytest.mark.parametrize("n", lc.SCAN_SIZES)
@pytest.mark.parametrize("dim", [3, 2])
def test_scan_case_mask_is_the_oracles_clip(oracle, dim, n):
    c = lc.scan_case(n, dim)
    mask, pts, R = c["mask"], c["points"], c["range_max"]
    # the structure per tile
    per_tile = np.add.reduceat(mask.astype(np.int64), np.arange(0, n, T))
    assert per_tile[0] == T and per_tile[1] == 0 and mask[n - 1] and not mask[n - 2] and np.isnan(pts[n - 2]).all()
    marked = [t for t in lc.SCAN_MARKED_TILES if (t + 1) * T <= n]
    assert len(marked) == (2 if n < 2 * T * T else 4)
    got = per_tile[marked]
    assert len(set(got.tolist())) == len(marked) and (got > 0).all() and (got < T).all()
    rest = np.delete(per_tile[:n // T], [0, 1] + marked)
    assert rest.min() < 0.1 * T and rest.max() > 0.5 * T and len(np.unique(rest)) > 500  # varying density
    # the margin: float64 distances from the robot
    d = np.linalg.norm(pts.astype(np.float64) - c["centre"].astype(np.float64), axis=1)
    assert d[mask].max() <= 0.5 * R and np.nanmin(d[~mask]) >= 2.0 * R and np.isnan(d).sum() == 1
    # ... and the oracle keeps exactly the mask, and nothing from the far pose
    b = oracle.scene_binding()
    full, clipped = mapping.Scene(b, dim), mapping.Scene(b, dim)
    full.set(pts, c["normals"])
    cl = mapping.SceneClipperBall(b, range_max=R)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(c["pose"])
    cl.compute()
    assert np.array_equal(cl.global_indices(), np.flatnonzero(mask))
    cl.set_robot_in_local_map(c["pose_far"])
    cl.compute()
    assert clipped.size() == 0
    full.close(); clipped.close()


def _crosses_the_cap(g):
    return len(g) > T and g[-1] >= CAP and (g < CAP).any()


@pytest.mark.parametrize("dim", [3, 2])
def test_clip_case(oracle, dim):
    c = lc.clip_case(dim)
    pts, n = c["points"], lc.N_CAP
    assert pts.shape == (n, dim) and c["descriptors"].shape == (n, 32) and c["intensity"].shape == (n,)
    bad = ~np.isfinite(pts).all(1)
    assert 0.0005 * n < bad.sum() < 0.002 * n and bad[CAP:].any() and bad[:CAP].any()
    b = oracle.scene_binding()
    full, clipped = mapping.Scene(b, dim), mapping.Scene(b, dim)
    full.set(pts, c["normals"])
    for pose in lc.ball_poses(dim):
        cl = mapping.SceneClipperBall(b, range_max=lc.BALL_RANGE[dim])
        cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
        cl.compute()
        g = cl.global_indices()
        assert _crosses_the_cap(g) and len(g) < n // 2
    full.close(); clipped.close()
    if dim == 3:
        for pose, sensor, margin in lc.PROJECTIVE_RUNS:
            r = cr.clip_projective(pts, pose, lc.CAMERA_K, lc.CAMERA_ROWS, lc.CAMERA_COLS, sensor_in_robot=sensor, occlusion_margin=margin)
            assert _crosses_the_cap(r["global_indices"])
            assert 0 < r["num_kept"] <= r["num_in_view"] < r["num_valid"] < n and (margin < 0 or r["num_kept"] < r["num_in_view"])
    else:
        paths = []
        for beams, a0, inc, pose, sensor, margin in lc.SCAN_RUNS:
            r = cs.clip_scan(pts, pose, a0, inc, beams, *lc.SCAN_CLIP_RANGES, sensor_in_robot=sensor, occlusion_margin=margin)
            assert _crosses_the_cap(r["global_indices"])
            assert 0 < r["num_kept"] <= r["num_in_view"] < r["num_valid"] < n and (margin < 0 or r["num_kept"] < r["num_in_view"])
            if margin >= 0:
                paths.append(lc.scan_minimum_in_lds(n, beams))
        assert sorted(paths) == [False, True]  # both kernels of the per-beam minimum


def _same_voxels(a, b, what):
    assert a["result"] == b["result"], (what, a["result"], b["result"])
    for k in ("points", "normals", "descriptors", "intensity", "global_indices", "counts"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert vr.same_bits(a[k], b[k]), (what, k)


def _both(pts, leaf, dim, what, **kw):
    a, b = lc.voxelize_vectorised(pts, leaf, dim=dim, **kw), vr.voxelize(pts, leaf, dim=dim, **kw)
    _same_voxels(a, b, (what, dim, kw.get("mode"), kw.get("min_points"), kw.get("normals") is not None))
    return a


@pytest.mark.parametrize("dim", [2, 3])
def test_vectorised_voxelize_equals_the_loop_restatement(dim):
    rng = np.random.default_rng(40 + dim)
    n = 20_000
    pts = rng.uniform(-3.0 if dim == 3 else -20.0, 3.0 if dim == 3 else 20.0, (n, dim)).astype(F)
    nrm = rng.normal(size=(n, dim))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    bad = rng.choice(n, n // 50, replace=False)
    pts[bad, rng.integers(0, dim, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    pts[rng.choice(n, n // 40)] = pts[rng.choice(n, n // 40)]  # exact duplicates
    some = rng.choice(n, n // 20, replace=False)
    nrm[some, rng.integers(0, dim, len(some))] = rng.choice(np.array([np.nan, np.inf, 2.0, -7.5, 1e30], F), len(some))
    desc, inten = lc.features(n, 1)
    seen = set()
    for mode in (vr.CENTROID, vr.FIRST):
        for normals in (None, nrm):
            for min_points in (1, 2, 3):
                r = _both(pts, 0.3, dim, "random", mode=mode, min_points=min_points, normals=normals, descriptors=desc, intensity=inten,
                          origin=(0.1, -0.2, 0.05))
                res = r["result"]
                assert res["num_finite"] < n and res["max_points_per_voxel"] > 3 and 0 < res["num_voxels"] <= res["num_occupied"]
                seen.add(res["num_voxels"])
    assert len(seen) == 3
    # the clouds of the through-the-stack case, an empty cloud, one without a finite point, one point
    for cloud in vc.clouds(dim):
        for mode in (vr.CENTROID, vr.FIRST):
            _both(cloud, vc.leaf_and_radius(dim)[0], dim, "voxel_cases", mode=mode)
    _both(np.zeros((0, dim), F), 0.5, dim, "empty", normals=np.zeros((0, dim), F))
    _both(np.full((5, dim), np.nan, F), 0.5, dim, "nothing finite", normals=np.ones((5, dim), F))
    _both(np.array([[1.0000001, 1e-30, -123456.79][:dim]], F), 0.3, dim, "one point")
    # the large cases' construction at a size the loop takes
    c = lc.voxel_many_cells(dim, n=20_001)
    desc, inten = lc.features(20_001, 2)
    for mode, normals, min_points in ((vr.CENTROID, c["normals"], 1), (vr.CENTROID, c["normals"], 2), (vr.FIRST, None, 2), (vr.FIRST, c["normals"], 3)):
        _both(c["points"], c["leaf"], dim, "many cells", mode=mode, normals=normals, min_points=min_points, descriptors=desc, intensity=inten)
    if dim == 3:
        _both(lc.voxel_lattice(20_001)[0], 1.0, 3, "lattice", mode=vr.FIRST)


@pytest.mark.parametrize("dim", [3, 2])
def test_voxel_many_cells_has_more_cells_than_the_cap(dim):
    c = lc.voxel_many_cells(dim)
    pts, n, fin = c["points"], lc.N_CAP, c["finite"]
    assert pts.shape == (n, dim) and np.array_equal(np.isfinite(pts).all(1), fin) and 0 < (~fin).sum() < n // 1000
    # every finite point in the cell it was meant for, a tenth of a leaf from every face
    t = pts[fin].astype(np.float64) / np.float64(F(c["leaf"]))
    assert np.array_equal(np.floor(t), c["cells"][fin]) and (t - np.floor(t)).min() > 0.09 and (t - np.floor(t)).max() < 0.91
    mode, min_points = (vr.CENTROID, 1) if dim == 3 else (vr.FIRST, 2)
    r = lc.voxelize_vectorised(pts, c["leaf"], dim=dim, mode=mode, min_points=min_points, normals=c["normals"] if dim == 3 else None)
    res = r["result"]
    assert res["num_occupied"] == c["num_cells"] > CAP and res["max_points_per_voxel"] == 3 and res["num_finite"] == int(fin.sum())
    if min_points == 1:
        assert res["num_voxels"] == res["num_occupied"] and 0 < res["num_with_normal"] < res["num_voxels"]
        assert (r["global_indices"] >= CAP).sum() > T
        assert [int((r["counts"] == k).sum()) for k in (1, 2, 3)] == [c["num_cells"] - c["num_twos"] - c["num_threes"], c["num_twos"], c["num_threes"]]
    else:
        assert T < res["num_voxels"] == c["num_twos"] + c["num_threes"]  # most cells are flagged 0
    assert (np.diff(r["global_indices"]) > 0).all()


def test_voxel_lattice_is_exact_and_every_point_owns_its_cell():
    pts, cells = lc.voxel_lattice()
    n = T * T + T + 1
    assert pts.shape == (n, 3) and np.array_equal(pts.astype(np.float64), cells + 0.5)  # exactly representable, mid-cell
    r = lc.voxelize_vectorised(pts, 1.0, dim=3, mode=vr.FIRST)
    assert r["result"] == {"num_points": n, "num_finite": n, "num_occupied": n, "num_voxels": n, "num_with_normal": 0,
                           "max_points_per_voxel": 1}
    assert np.array_equal(r["global_indices"], np.arange(n)) and vr.same_bits(r["points"], pts) and (r["counts"] == 1).all()
    assert vr.key_layout(pts, 1.0, (0, 0, 0), 3) is not None


def _every_class(res, live):
    """"substantial": most of the points that take part get a normal"""
    assert res["num_with_normal"] > 0.5 * live and res["num_too_few"] > 0 and res["num_degenerate"] + res["num_too_curved"] > 0


def test_normals_clouds_at_a_small_size_give_every_class():
    c = lc.normals_curve(n=20_001)
    pts = c["points"]
    assert pts.shape == (20_001, 2) and 0 < (~np.isfinite(pts).all(1)).sum() <= 20
    r = nr.estimate_normals(pts, c["radius"], dim=2, viewpoint=None, drop=True, max_curvature=lc.NORMALS_MAX_CURVATURE)
    print(r["result"], np.median(r["count"][r["cls"] == nr.CLS_NORMAL]))
    _every_class(r["result"], 20_001)
    assert r["result"]["num_degenerate"] > 0 and r["result"]["num_too_curved"] > 0
    assert 5 <= np.median(r["count"][r["cls"] == nr.CLS_NORMAL]) <= 9  # (the point itself counts)
    c = lc.normals_behind_a_dead_head(head=10_000, m=10_000)
    pts = c["points"]
    assert pts.shape == (20_000, 3) and not np.isfinite(pts[:10_000]).all(1).any() and np.isfinite(pts[10_000:]).all()
    for drop, vp in ((True, None), (False, lc.NORMALS_VIEW)):
        r = nr.estimate_normals(pts, c["radius"], dim=3, viewpoint=vp, drop=drop, max_curvature=lc.NORMALS_MAX_CURVATURE)
        print(r["result"])
        _every_class(r["result"], 10_000)
        assert r["result"]["num_finite"] == 10_000 and r["kept"][0] >= (10_000 if drop else 0)


def test_the_full_size_normals_clouds_are_past_the_cap():
    c = lc.normals_curve()
    fin = np.isfinite(c["points"]).all(1)
    assert len(fin) == lc.N_CAP and fin.sum() > CAP and 0.0005 * len(fin) < (~fin).sum() < 0.002 * len(fin)
    c = lc.normals_behind_a_dead_head()
    fin = np.isfinite(c["points"]).all(1)
    assert len(fin) == CAP + 40_000 and not fin[:CAP].any() and fin[CAP:].all()
