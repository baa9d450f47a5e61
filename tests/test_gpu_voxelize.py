"""GPU: srrg2_scene_voxelize (csrc/voxel.hip) against the numpy restatement of its contract (tests/voxel_restatement.py), BIT FOR
BIT: points, normals, descriptors, intensities, global indices, counts and the result struct; refusals leave `dst` as it was and
every call leaves `src` as it was; and through the stack: set -> voxelize -> estimate normals -> align equals the oracle's run on
the restatement-made decimated cloud."""
import ctypes as C

import numpy as np
import pytest

import voxel_restatement as vr
from helpers import assert_same_run
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID, E_UNSUPPORTED = -1, -4
MODES = {"centroid": vr.CENTROID, "first": vr.FIRST}


def _features(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F)


def _snapshot(scene):
    c, m = scene.get()
    d, i = scene.features()
    _, nrm_ptr, _ = scene.device_arrays()
    return (scene.size(), c.tobytes(), m.tobytes(), None if d is None else d.tobytes(), None if i is None else i.tobytes(),
            scene.global_indices().tobytes(), scene.has_features(), nrm_ptr is not None)


def _check(product, pts, leaf, dim, mode="centroid", normals=None, features=False, origin=(0.0, 0.0, 0.0), min_points=1, dst=None,
           tag=""):
    """one call against the restatement: everything the call writes, and that it leaves the source alone"""
    b = product.scene_binding(0)
    src = mapping.Scene(b, dim)
    src.set(pts, normals)
    desc = inten = None
    if features:
        desc, inten = _features(len(pts), 3)
        src.set_features(desc, inten)
    before = _snapshot(src)
    dst = mapping.Scene(b, dim) if dst is None else dst
    res, counts = src.voxelize(dst, leaf, origin=origin, mode=mode, min_points=min_points, return_counts=True)
    r = vr.voxelize(pts, leaf, dim=dim, origin=origin, mode=MODES[mode], min_points=min_points, normals=normals, descriptors=desc,
                    intensity=inten)
    assert res == r["result"], (tag, res, r["result"])
    assert _snapshot(src) == before, tag
    m = r["result"]["num_voxels"]
    assert dst.size() == m
    c, nrm = dst.get()
    bad = np.flatnonzero((c.view(np.uint32) != r["points"].view(np.uint32)).any(1)) if c.shape == r["points"].shape else None
    assert vr.same_bits(c, r["points"]), (tag, bad[:10] if bad is not None else c.shape)
    assert np.array_equal(dst.global_indices(), r["global_indices"]), tag
    assert np.array_equal(counts, r["counts"]), tag
    _, nptr, _ = dst.device_arrays()
    assert (nptr is not None) == (normals is not None), tag
    if normals is not None:
        assert vr.same_bits(nrm, r["normals"]), (tag, np.flatnonzero((nrm.view(np.uint32) != r["normals"].view(np.uint32)).any(1))[:10])
    else:
        assert not nrm.any(), tag
    assert dst.has_features() == (features, features), tag
    if features:
        d, i = dst.features()
        assert vr.same_bits(d, r["descriptors"]) and vr.same_bits(i, r["intensity"]), tag
    return r


def _cloud(n, dim, seed, extent=1.0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-extent, extent, (n, dim)).astype(F)
    nrm = rng.normal(size=(n, dim))
    return pts, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 257])
def test_small_sizes(product, n, dim):
    pts, nrm = _cloud(n, dim, 10 + n)
    leaf = 0.5 if dim == 3 else 0.25  # (a few points per cell at the larger sizes, lone ones too)
    for mode in ("centroid", "first"):
        for features in (False, True):
            for with_normals in (False, True):
                r = _check(product, pts, leaf, dim, mode, nrm if with_normals else None, features, tag=(n, dim, mode, features, with_normals))
    if n >= 63:
        assert r["result"]["num_voxels"] < n and r["result"]["max_points_per_voxel"] > 1


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["centroid", "first"])
def test_one_crowded_cell(product, dim, mode):
    """6 000 points inside ONE cell, 50 scattered around it: the cell's run spans ~94 waves of the reduction, all but the
    pieces at its two ends add into the accumulators with 64-bit atomics"""
    rng = np.random.default_rng(9)
    inner = (2.0 + 0.98 * rng.random((6000, dim))).astype(F)
    outer = (2.5 + rng.uniform(-1.6, 1.6, (50, dim))).astype(F)
    outer = outer[((outer < 2.0) | (outer >= 3.0)).any(1)]
    pts = np.concatenate([inner, outer])[rng.permutation(6000 + len(outer))]
    nrm = _cloud(len(pts), dim, 4)[1]
    r = _check(product, pts, 1.0, dim, mode, nrm, features=True, tag=("crowded", dim, mode))
    assert r["result"]["max_points_per_voxel"] == 6000 and r["result"]["num_voxels"] > 10


@pytest.mark.parametrize("dim", [2, 3])
def test_every_point_its_own_cell(product, dim):
    m = 40 if dim == 2 else 12
    g = (np.arange(m, dtype=np.float64) + 0.3) * 0.5
    pts = np.stack([a.ravel() for a in np.meshgrid(*([g] * dim), indexing="ij")], 1).astype(F)
    pts = pts[np.random.default_rng(2).permutation(len(pts))]
    nrm = _cloud(len(pts), dim, 6)[1]
    for mode in ("centroid", "first"):
        r = _check(product, pts, 0.5, dim, mode, nrm, features=True, tag=("own cell", dim, mode))
        assert vr.same_bits(r["points"], pts) and np.array_equal(r["global_indices"], np.arange(len(pts)))
    assert vr.same_bits(_check(product, pts, 0.5, dim, "first", nrm)["normals"], nrm)


@pytest.mark.parametrize("lead", [0, 1, 62])
def test_runs_that_straddle_wave_edges(product, lead):
    """a 1-D row of cells whose populations are `lead` ones, then 1, 63, 64, 65, 130, 1, 200, 3: in the sorted order the runs lie
    back to back in this order (the cell index ascends), so with lead = 0 / 1 / 62 their heads fall on lanes 0, 1, 63 and on
    everything in between, runs end exactly on a wave's last lane, and the 130 and 200 runs cross one or two edges"""
    runs = [1] * lead + [1, 63, 64, 65, 130, 1, 200, 3]
    rng = np.random.default_rng(lead)
    cell = np.repeat(np.arange(len(runs)), runs)
    x = (cell + rng.uniform(0.01, 0.99, len(cell))) * 0.25
    pts = np.stack([x, rng.uniform(0.01, 0.24, len(cell)), rng.uniform(0.01, 0.24, len(cell))], 1).astype(F)
    assert np.array_equal(np.floor(pts[:, 0].astype(np.float64) / 0.25), cell)
    order = rng.permutation(len(pts))  # scene order is not cell order
    pts, cell = pts[order], cell[order]
    nrm = _cloud(len(pts), 3, 8)[1]
    for dim in (2, 3):
        for mode in ("centroid", "first"):
            r = _check(product, pts[:, :dim], 0.25, dim, mode, nrm[:, :dim], features=True, tag=("straddle", lead, dim, mode))
            assert np.array_equal(r["counts"], np.asarray(runs)[cell[r["global_indices"]]])
            assert sorted(r["counts"].tolist()) == sorted(runs)


@pytest.mark.parametrize("dim", [2, 3])
def test_faces(product, dim):
    """a lattice whose spacing is the leaf: every point on a cell corner, wherever the lattice lies; with the origin moved by half
    a leaf every point is in the middle of its cell.  Twice as fine: 2^dim points per cell, on faces and corners"""
    leaf = 0.25
    for spacing in (leaf, leaf / 2):
        g = np.arange(8, dtype=np.float64) * spacing
        P = np.stack([a.ravel() for a in np.meshgrid(*([g] * dim), indexing="ij")], 1) - 0.5
        for shift in (0.0, 1e4, -3e4):
            pts = (P + shift).astype(F)
            assert np.array_equal(np.diff(np.unique(pts[:, 0])), np.full(7, F(spacing)))
            for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125)):
                r = _check(product, pts, leaf, dim, "centroid", origin=origin, tag=("faces", dim, spacing, shift, origin))
                if spacing == leaf:
                    assert r["result"]["num_voxels"] == len(pts)
                elif origin[0] == 0.0:
                    assert (r["counts"] == 2 ** dim).all()


@pytest.mark.parametrize("dim,mode,min_points", [(3, "centroid", 1), (3, "centroid", 2), (2, "centroid", 3), (3, "first", 2), (2, "first", 1)])
def test_random_cloud_with_bad_values(product, dim, mode, min_points):
    n = 20_000
    pts, nrm = _cloud(n, dim, 77, extent=3.0 if dim == 3 else 20.0)
    rng = np.random.default_rng(5)
    bad = rng.choice(n, n // 50, replace=False)
    pts[bad, rng.integers(0, dim, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    src = rng.choice(n, n // 40)
    pts[rng.choice(n, n // 40)] = pts[src]  # exact duplicates
    some = rng.choice(n, n // 20, replace=False)
    nrm[some, rng.integers(0, dim, len(some))] = rng.choice(np.array([np.nan, np.inf, 2.0, -7.5, 1e30], F), len(some))
    r = _check(product, pts, 0.3, dim, mode, nrm, features=True, min_points=min_points, tag=("random", dim, mode, min_points))
    res = r["result"]
    print(dim, mode, min_points, res)
    assert res["num_finite"] < n and res["max_points_per_voxel"] > 3 and res["num_with_normal"] > 0
    if min_points > 1:
        assert res["num_voxels"] < res["num_occupied"]
    if mode == "centroid":
        assert res["num_with_normal"] <= res["num_voxels"]


def test_far_apart_clusters_and_a_reused_destination(product):
    """cells are keyed relative to the lowest occupied one: a cloud 10^7 leaves from the origin, and two clusters 10^6 leaves apart
    on every axis, are fine; one `dst` takes results of different sizes and field sets one after the other"""
    dst = mapping.Scene(product.scene_binding(0), 3)
    a, na = _cloud(3000, 3, 1)
    _check(product, (a + F(1.25e6)).astype(F), 0.125, 3, "centroid", na, features=True, dst=dst, tag="offset")
    b = np.concatenate([a, (a + np.asarray([1.25e5, -1.25e5, 1.25e5], F)).astype(F)])
    _check(product, b, 0.125, 3, "centroid", dst=dst, tag="two clusters")
    _check(product, a[:10], 0.5, 3, "first", na[:10], dst=dst, tag="small")
    _check(product, np.zeros((0, 3), F), 0.5, 3, "first", dst=dst, tag="empty")


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals(product, dim):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    b = product.scene_binding(0)
    pts, nrm = _cloud(500, dim, 3)
    src, dst, other = mapping.Scene(b, dim), mapping.Scene(b, dim), mapping.Scene(b, 5 - dim)
    desc, inten = _features(500, 1)
    src.set(pts, nrm)
    src.set_features(desc, inten)
    keep, knrm = _cloud(300, dim, 4)
    full = mapping.Scene(b, dim)
    full.set(keep, knrm)
    full.set_features(*_features(300, 2))
    assert full.voxelize(dst, 0.3)["num_voxels"] > 50  # dst holds points, normals, features and global indices
    before_dst, before_src = _snapshot(dst), _snapshot(src)

    def call(s=src._h, d=dst._h, null_params=False, **kw):
        p = mapping.default_voxel_params()
        p.leaf_size = 0.2
        for k, v in kw.items():
            if k in ("origin", "reserved"):
                for j, x in enumerate(v):
                    getattr(p, k)[j] = x
            else:
                setattr(p, k, v)
        return lib.srrg2_scene_voxelize(s, None if null_params else C.byref(p), d, None, None)

    assert call(s=None) == E_INVALID and call(d=None) == E_INVALID and call(null_params=True) == E_INVALID
    assert call(d=src._h) == E_INVALID  # src == dst
    assert call(d=other._h) == E_INVALID  # different dims
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(leaf_size=bad) == E_INVALID
    for bad in (float("nan"), float("inf")):
        for axis in range(3):
            o = [0.0, 0.0, 0.0]
            o[axis] = bad
            assert call(origin=o) == E_INVALID
    assert call(mode=2) == E_INVALID and call(mode=-1) == E_INVALID
    assert call(min_points_per_voxel=0) == E_INVALID and call(min_points_per_voxel=-3) == E_INVALID
    assert call(reserved=[1, 0]) == E_INVALID and call(reserved=[0, 7]) == E_INVALID
    if _capi.device_count() > 1:
        far = mapping.Scene(product.scene_binding(1), dim)
        assert call(d=far._h) == E_INVALID  # different devices
    assert _snapshot(dst) == before_dst and _snapshot(src) == before_src
    # the extent: two points 2^31 leaves apart on one axis
    wide = mapping.Scene(b, dim)
    two = np.zeros((2, dim), F)
    two[1, dim - 1] = 2.0 ** 31 * 0.25
    assert vr.key_layout(two, 0.25, (0, 0, 0), dim) is None
    wide.set(two)
    before_wide = _snapshot(wide)
    assert call(s=wide._h, leaf_size=0.25) == E_UNSUPPORTED
    assert b"63-bit" in lib.srrg2_amd_last_error()
    assert _snapshot(dst) == before_dst and _snapshot(wide) == before_wide
    two[1, dim - 1] = (2.0 ** 30 - 64) * 0.25  # ... and the widest the key holds
    assert vr.key_layout(two, 0.25, (0, 0, 0), dim) is not None
    _check(product, two, 0.25, dim, tag="widest")
    assert call() == 0 and dst.size() > 0 and _snapshot(src) == before_src


@pytest.mark.parametrize("dim", [2, 3])
def test_through_the_stack_equals_the_oracle(product, oracle, dim):
    """two clouds without normals: Scene.set -> voxelize -> estimate_normals(drop) -> set_moving / set_fixed on device arrays ->
    point-to-plane compute(); the oracle aligns the clouds the two restatements make"""
    import normals_restatement as nr
    import voxel_cases as vc

    kind = abi.SE3_QUAT_RIGHT if dim == 3 else abi.SE2_RIGHT
    leaf, radius = vc.leaf_and_radius(dim)
    b = product.scene_binding(0)
    want, scenes = [], []
    for cloud in vc.clouds(dim):
        v, n = vc.restated(cloud, dim)
        assert len(cloud) // 5 < v["result"]["num_voxels"] < 4 * len(cloud) // 5 and n["result"]["scene_size"] > 0.8 * v["result"]["num_voxels"]
        full, dec = mapping.Scene(b, dim), mapping.Scene(b, dim)
        full.set(cloud)
        assert full.voxelize(dec, leaf) == v["result"]
        assert dec.estimate_normals(radius, viewpoint=vc.VIEW, drop=True) == n["result"]
        assert nr.same_bits(dec.get()[0], n["points_out"]) and nr.same_bits(dec.get()[1], n["normals_out"])
        want.append(n)
        scenes.append(dec)
    ref = vc.oracle_run(oracle, dim, fixed=want[1], moving=want[0])
    al = product.MultiAligner(kind, device=0)
    si = al.add_slice(vc.config(dim))
    mp, mn, m = scenes[0].device_arrays()
    fp, fn, f = scenes[1].device_arrays()
    al.set_cloud_device("set_fixed", si, fp, 16, fn, 16, f, kept=True)
    al.set_cloud_device("set_moving", si, mp, 16, mn, 16, m, kept=True)
    al.set_moving_in_fixed(syn.identity(dim))
    al.compute()
    assert al.status() == abi.SUCCESS
    assert_same_run(ref, al)
    print(dim, m, f, al.iteration_stats()[-1]["num_correspondences"])
    assert al.iteration_stats()[-1]["num_correspondences"] > m // 2


def test_decimated_map_into_the_clipper_and_the_merger(product):
    """voxelize a map with features, clip_ball the result: the clipped scene's global indices composed with the decimated scene's
    name the right source points, and the descriptors follow; then a measurement merges into the decimated map"""
    dim = 3
    b = product.scene_binding(0)
    pts, nrm = _cloud(8000, dim, 12, extent=2.0)
    desc, inten = _features(len(pts), 5)
    src, dec, clipped = (mapping.Scene(b, dim) for _ in range(3))
    src.set(pts, nrm)
    src.set_features(desc, inten)
    res = src.voxelize(dec, 0.2)
    r = vr.voxelize(pts, 0.2, normals=nrm, descriptors=desc, intensity=inten)
    assert res == r["result"] and 500 < res["num_voxels"] < 7000
    cl = mapping.SceneClipperBall(b, range_max=1.5)
    cl.set_full_scene(dec); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(np.asarray(syn.identity(dim), F)); cl.compute()
    g = clipped.global_indices()
    inside = np.flatnonzero(((r["points"].astype(F) ** 2).sum(1, dtype=F)) <= F(1.5) * F(1.5))
    assert 50 < len(g) < res["num_voxels"] and abs(len(g) - len(inside)) <= 2  # (the clipper's own order of operations decides ties)
    back = dec.global_indices()[g]  # clipped -> decimated -> source
    assert np.array_equal(back, r["global_indices"][g])
    d, i = clipped.features()
    assert vr.same_bits(d, desc[back]) and vr.same_bits(i, inten[back])
    assert vr.same_bits(clipped.get()[0], r["points"][g])  # (identity pose: the clipper moves nothing)
    # the decimated map takes a merge like any scene: a measurement of its own points, one correspondence each
    meas = mapping.Scene(b, dim)
    meas.set(r["points"][:100], r["normals"][:100])
    meas.set_features(desc[:100], inten[:100])
    mg = mapping.MergerCorrespondenceHomo(b)
    mg.set_scene(dec); mg.set_measurement(meas); mg.set_measurement_in_scene(np.asarray(syn.identity(dim), F))
    corr = np.zeros(100, dtype=[("fixed_idx", "<i4"), ("moving_idx", "<i4"), ("response", "<f4")])
    corr["fixed_idx"], corr["moving_idx"], corr["response"] = np.arange(100), np.arange(100), 0.0
    mg.set_correspondences(corr)
    out = mg.compute()
    assert out["num_merged"] == 100 and out["scene_size"] == res["num_voxels"]
    assert vr.same_bits(dec.features()[0][:100], desc[:100])
