"""GPU: srrg2_scene_estimate_normals (csrc/normals.hip) against the numpy restatement of its contract
(tests/normals_restatement.py), BIT FOR BIT: normals, curvature, counts, surviving order, global indices, moved descriptors and
intensities; refusals leave the scene as it was; and through the stack: set -> estimate normals -> clip -> align -> merge equals the
oracle's run on restatement-made normals."""
import ctypes as C

import numpy as np
import pytest

import normals_restatement as nr
from helpers import assert_same_run, cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID, E_UNSUPPORTED = -1, -4
VIEW = (0.3, -0.2, 5.0)


def _features(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F)


def _snapshot(scene):
    c, m = scene.get()
    d, i = scene.features()
    return (scene.size(), c.tobytes(), m.tobytes(), None if d is None else d.tobytes(), None if i is None else i.tobytes(),
            scene.global_indices().tobytes())


def _check(product, pts, radius, dim, drop, viewpoint, features=False, tag="", **kw):
    """one call on a fresh scene against the restatement: everything the call writes"""
    b = product.scene_binding(0)
    s = mapping.Scene(b, dim)
    s.set(pts)
    desc = inten = None
    if features:
        desc, inten = _features(len(pts), 3)
        s.set_features(desc, inten)
    res, curv = s.estimate_normals(radius, viewpoint=viewpoint, drop=drop, return_curvature=True, **kw)
    r = nr.estimate_normals(pts, radius, dim=dim, viewpoint=viewpoint, drop=drop, **kw)
    assert res == r["result"], (tag, res, r["result"])
    assert nr.same_bits(curv, r["curvature"]), tag
    c, m = s.get()
    assert s.size() == len(r["kept"])
    assert nr.same_bits(c, r["points_out"]), tag
    assert nr.same_bits(m, r["normals_out"]), (tag, np.flatnonzero((m.view(np.uint32) != r["normals_out"].view(np.uint32)).any(1))[:10])
    if drop:
        assert np.array_equal(s.global_indices(), r["kept"]), tag
    if features:
        d, i = s.features()
        assert nr.same_bits(d, desc[r["kept"]]) and nr.same_bits(i, inten[r["kept"]]), tag
    return r


def _cloud(n, dim, seed):
    """points of the CPU test's surfaces, ~10 neighbours at any n >= 64"""
    kinds = ["plane", "sphere", "cylinder", "crossing"] if dim == 3 else ["line", "circle", "crossing"]
    per = max(1, n // len(kinds))
    radius = (0.09 if dim == 3 else 0.006) * (5000.0 / max(per, 1)) ** (1.0 / (dim - 1)) * 0.6
    radius = float(min(radius, 0.5))
    parts = [nr.surface(k, per if j else n - per * (len(kinds) - 1), seed + j, radius, dim) for j, k in enumerate(kinds)]
    return np.concatenate(parts)[np.random.default_rng(seed).permutation(n)], radius


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [0, 1, 4, 63, 64, 65, 257])
def test_small_sizes(product, n, dim):
    pts, radius = _cloud(260, dim, 10)[0][:n], 0.2
    for drop in (False, True):
        for vp in (VIEW, None):
            _check(product, pts, radius, dim, drop, vp, features=drop, tag=(n, dim, drop, vp))


@pytest.mark.parametrize("dim,drop,vp", [(3, True, VIEW), (3, False, None), (2, True, None), (2, False, VIEW)])
def test_random_cloud_with_bad_values(product, dim, drop, vp):
    n = 20_000
    pts, radius = _cloud(n, dim, 77)
    rng = np.random.default_rng(5)
    bad = rng.choice(n, n // 50, replace=False)
    pts[bad, rng.integers(0, dim, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    src = rng.choice(n, n // 40)
    pts[rng.choice(n, n // 40)] = pts[src]  # exact duplicates
    r = _check(product, pts, radius, dim, drop, vp, features=True, max_curvature=0.2, tag=("random", dim))
    res = r["result"]
    print(dim, res)
    assert res["num_finite"] < n and res["num_with_normal"] > n // 2 and res["num_too_few"] > 0


@pytest.mark.parametrize("dim", [2, 3])
def test_one_crowded_cell(product, dim):
    """6 000 points inside ONE cell, 50 around it.  The neighbourhood kernel stages candidates in LDS tiles of 64 points
    (SRRG2_NRM_TILE in csrc/normals.hip): the cell takes 94 tiles, and its 6 000 queries spread over 94 workgroups"""
    rng = np.random.default_rng(9)
    radius = 1.0
    inner = (2.0 + 0.98 * rng.random((6000, dim))).astype(F)
    outer = (2.5 + rng.uniform(-1.6, 1.6, (50, dim))).astype(F)
    pts = np.concatenate([np.zeros((1, dim), F), inner, outer])  # (the origin pins the cells: the crowd fills cell (2, 2[, 2]))
    r = _check(product, pts, radius, dim, True, None, tag=("crowded", dim))
    assert r["count"].max() > 3000


@pytest.mark.parametrize("dim", [2, 3])
def test_cell_borders_and_distance_exactly_the_radius(product, dim):
    """a lattice with spacing exactly the radius, shifted so that the box minimum is no lattice point: axis neighbours are
    members (inclusive), diagonal ones are not, wherever the cell borders fall"""
    m, radius = 9, 0.25
    g = np.arange(m, dtype=np.float64) * radius
    P = np.stack([a.ravel() for a in np.meshgrid(*([g] * dim), indexing="ij")], 1)
    pts = np.concatenate([P + 0.0625, np.full((1, dim), -1.03125)]).astype(F)  # (+ one point far off the lattice)
    for shift in (0.0, 1e4, -3e4):
        q = (pts + F(shift)).astype(F)
        if shift:
            # membership must be unambiguous on the restatement's side: no pair at d2 == r2 unless it is a lattice step
            assert np.array_equal(np.diff(np.unique(q[:-1, 0])), np.full(m - 1, F(radius)))
        r = _check(product, q, radius, dim, False, None, min_neighbours=dim + 1, tag=("lattice", dim, shift))
        idx = np.stack([a.ravel() for a in np.meshgrid(*([np.arange(m)] * dim), indexing="ij")], 1)
        expect = 1 + sum((idx[:, d] > 0).astype(int) + (idx[:, d] < m - 1).astype(int) for d in range(dim))
        assert np.array_equal(r["count"][:-1], expect)


@pytest.mark.parametrize("offset", [1e4, -3e4])
def test_large_offsets(product, offset):
    """coordinates far from the origin: the moments are taken about the query"""
    pts, radius = _cloud(3000, 3, 31)[0], 0.2
    q = (pts + F(offset)).astype(F)
    # unambiguous membership: no pair of the shifted cloud sits at exactly the radius
    r2 = F(radius) * F(radius)
    for _, _, d in nr.member_pairs(q, radius * 1.001, 3):
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        assert not (d2 == r2).any()
    r = _check(product, q, radius, 3, True, (offset, offset, offset + 5), tag=("offset", offset))
    assert r["result"]["num_with_normal"] > 1000


def _inverse(X, dim):
    """the inverse of an estimate as the ABI takes transforms: 3x3 (SE2) or 3x4 (SE3), float32"""
    H = np.eye(dim + 1)
    H[:dim, :] = np.asarray(X, np.float64).reshape(-1, dim + 1)[:dim, :]
    return np.ascontiguousarray(np.linalg.inv(H)[:3, :], F)


def _clusters(dim, sep):
    a = nr.surface("plane" if dim == 3 else "line", 2000, 1, 0.1, dim)
    b = nr.surface("sphere" if dim == 3 else "circle", 2000, 2, 0.1, dim)
    return np.concatenate([a, (b + np.asarray(sep, F)[:dim]).astype(F)])


def test_far_apart_clusters(product):
    radius = 0.125
    far = 1e7 * radius
    for dim, vp in ((3, None), (2, VIEW)):
        pts = _clusters(dim, (far, 0, 0))
        r = _check(product, pts, radius, dim, True, vp, tag=("far", dim))
        assert r["result"]["num_with_normal"] > 1000
    # beyond the key range: 10^7 radii apart along all three axes (3 x 24 bits), 2^31 radii along one (2-D)
    from srrg2_slam_interfaces_amd import _capi

    for dim, sep, rad in ((3, (far, far, far), radius), (2, (4e6, 0, 0), 1e-3)):
        s = mapping.Scene(product.scene_binding(0), dim)
        s.set(_clusters(dim, sep))
        before = _snapshot(s)
        p = abi.NormalsParams()
        _capi.lib().srrg2_normals_default_params(C.byref(p), dim)
        p.radius = rad
        out = abi.NormalsResult()
        assert _capi.lib().srrg2_scene_estimate_normals(s._h, C.byref(p), None, C.byref(out)) == E_UNSUPPORTED
        assert _snapshot(s) == before


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_leave_the_scene_untouched(product, dim):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    pts, radius = _cloud(500, dim, 3)
    s = mapping.Scene(product.scene_binding(0), dim)
    desc, inten = _features(500, 1)
    nrm = np.random.default_rng(2).normal(size=(500, dim)).astype(F)
    s.set(pts, nrm)
    s.set_features(desc, inten)
    s.estimate_normals(0.3, drop=True)  # (global indices to keep)
    before = _snapshot(s)
    assert before[0] > 100

    def call(handle=s._h, null_params=False, **kw):
        p = abi.NormalsParams()
        lib.srrg2_normals_default_params(C.byref(p), dim)
        p.radius = 0.3
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.srrg2_scene_estimate_normals(handle, None if null_params else C.byref(p), None, None)

    assert call(handle=None) == E_INVALID and call(null_params=True) == E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e20, 1e-24):  # (the last two: radius*radius is inf / 0 in float32)
        assert call(radius=bad) == E_INVALID
    assert call(min_neighbours=dim) == E_INVALID and call(min_neighbours=-1) == E_INVALID
    assert call(max_curvature=float("nan")) == E_INVALID
    assert call(drop_points_without_normal=2) == E_INVALID and call(drop_points_without_normal=-1) == E_INVALID
    assert _snapshot(s) == before
    assert call(min_neighbours=dim + 1) == 0


@pytest.mark.parametrize("dim", [2, 3])
def test_a_reused_handle_reaches_a_fixed_point(product, dim):
    """one scene, frame after frame: set -> estimate_normals(drop) thirty times, with features.  Every frame matches the
    restatement, and from the third frame on the scene's arrays alternate between the same two allocations: nothing grows"""
    s = mapping.Scene(product.scene_binding(0), dim)
    clouds = [_cloud(3000, dim, 40 + k) for k in range(3)]
    want = [nr.estimate_normals(p, r, dim=dim, viewpoint=VIEW, drop=True) for p, r in clouds]
    desc, inten = _features(3000, 6)
    seen = []
    for frame in range(30):
        (pts, radius), r = clouds[frame % 3], want[frame % 3]
        s.set(pts)
        s.set_features(desc, inten)
        assert s.estimate_normals(radius, viewpoint=VIEW, drop=True) == r["result"]
        assert nr.same_bits(s.get()[0], r["points_out"]) and nr.same_bits(s.get()[1], r["normals_out"])
        d, i = s.features()
        assert nr.same_bits(d, desc[r["kept"]]) and nr.same_bits(i, inten[r["kept"]])
        assert np.array_equal(s.global_indices(), r["kept"])
        cp, cn, _ = s.device_arrays()
        dp, ip, _ = s.device_features()
        seen.append(tuple(C.cast(x, C.c_void_p).value for x in (cp, cn, dp, ip)))
    for k in range(4):
        assert len({t[k] for t in seen[2:]}) <= 2, (k, [hex(t[k]) for t in seen])
    # viewpoint: a NaN in the third component means "no viewpoint" for a 2-D scene as well
    if dim == 2:
        pts, radius = clouds[0]
        s.set(pts)
        s.estimate_normals(radius, viewpoint=(0.3, -0.2, np.nan), drop=False)
        assert nr.same_bits(s.get()[1], nr.estimate_normals(pts, radius, dim=2, viewpoint=None, drop=False)["normals"])


def test_queued_call_without_outputs(product):
    """drop = 0 and no outputs: the call returns without waiting; the next scene call settles it -- same bits"""
    pts, radius = _cloud(5000, 3, 8)
    s = mapping.Scene(product.scene_binding(0), 3)
    s.set(pts)
    assert s.estimate_normals(radius, drop=False, want_result=False) is None
    r = nr.estimate_normals(pts, radius, drop=False)
    assert nr.same_bits(s.get()[1], r["normals"])
    # ... and an extent it cannot refuse from there leaves NaN normals, never stale ones
    s.set(_clusters(3, (1.25e6, 1.25e6, 1.25e6)), np.ones((4000, 3), F))
    assert s.estimate_normals(0.125, drop=False, want_result=False) is None
    assert np.isnan(s.get()[1]).all() and s.size() == 4000


def test_after_an_adaptor_write_still_pending(product):
    """srrg2_adapt_depth_image, organised, out == NULL leaves its write queued: estimate_normals settles it by itself"""
    import adaptor_restatement as ar

    rows, cols = 48, 64
    rng = np.random.default_rng(4)
    depth = (1.5 + 0.002 * np.arange(cols)[None, :] + 0.003 * np.arange(rows)[:, None] + 0.0005 * rng.random((rows, cols))).astype(F)
    depth[rng.random((rows, cols)) < 0.05] = 0.0
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], F)
    p = adaptors.default_depth_params()
    for k, v in enumerate(K.reshape(9)):
        p.camera_matrix[k] = float(v)
    p.rows, p.cols, p.compact = rows, cols, 0
    meas = mapping.Scene(product.scene_binding(0), 3)
    ad = adaptors.MeasurementAdaptorDepthImage(p)
    ad.set_meas(meas); ad.set_raw_data(depth); ad.compute(False)
    res = meas.estimate_normals(0.12, drop=True)
    want = ar.adapt_depth_image(depth, K, depth_scale=p.depth_scale, depth_min=p.depth_min, depth_max=p.depth_max, col_gap=1, row_gap=1,
                                max_distance_squared=p.normal_max_distance_squared, drop_points_without_normal=True, compact=False)
    r = nr.estimate_normals(want["points"], 0.12, drop=True)
    assert res == r["result"] and res["num_with_normal"] > 1000
    assert nr.same_bits(meas.get()[0], r["points_out"]) and nr.same_bits(meas.get()[1], r["normals_out"])
    assert np.array_equal(meas.global_indices(), r["kept"])


@pytest.mark.parametrize("dim", [2, 3])
def test_through_the_stack_equals_the_oracle(product, oracle, dim):
    """two clouds without normals: Scene.set -> estimate_normals(drop) -> clip_ball -> set_moving / set_fixed on device arrays
    (kept) -> point-to-plane compute() -> merge_from_aligner into the estimated map; the oracle runs the same on restatement-made
    normals"""
    kind = abi.SE3_QUAT_RIGHT if dim == 3 else abi.SE2_RIGHT
    n, radius = 5000, (0.09 if dim == 3 else 0.012)
    rng = np.random.default_rng(12)
    if dim == 3:
        map_pts = np.concatenate([nr.surface("plane", n // 2, 1, radius), nr.surface("crossing", n - n // 2, 2, radius)])
        X = np.eye(4)
        X[:3, :] = np.asarray(syn.se3((0.02, -0.015, 0.01), np.deg2rad([0.5, -0.4, 0.8])), np.float64)[:3, :]
    else:
        map_pts = np.concatenate([nr.surface("crossing", n // 2, 1, radius, 2), nr.surface("circle", n - n // 2, 2, radius, 2)])
        X = np.asarray(syn.se2(0.004, -0.003, np.deg2rad(0.4)), np.float64)
    meas_pts = ((map_pts.astype(np.float64) @ X[:dim, :dim].T + X[:dim, dim]) + rng.normal(scale=0.002 * radius, size=map_pts.shape)).astype(F)
    view = (0.0, 0.0, 3.0)
    rm, rs = (nr.estimate_normals(p, radius, dim=dim, viewpoint=view, drop=True) for p in (map_pts, meas_pts))
    assert min(rm["result"]["scene_size"], rs["result"]["scene_size"]) > 0.9 * n
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 4 * radius, robust=abi.ROBUST_CAUCHY)
    I = syn.identity(dim)
    runs = {}
    for side in ("oracle", "gpu"):
        b = oracle.scene_binding() if side == "oracle" else product.scene_binding(0)
        scene, meas, clipped = (mapping.Scene(b, dim) for _ in range(3))
        if side == "oracle":
            scene.set(rm["points_out"], rm["normals_out"]); meas.set(rs["points_out"], rs["normals_out"])
        else:
            scene.set(map_pts); meas.set(meas_pts)
            assert scene.estimate_normals(radius, viewpoint=view, drop=True) == rm["result"]
            assert meas.estimate_normals(radius, viewpoint=view, drop=True) == rs["result"]
        cl = mapping.SceneClipperBall(b, range_max=100.0)
        cl.set_full_scene(scene); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(np.asarray(I, F)); cl.compute()
        al = oracle.OracleAligner(kind) if side == "oracle" else product.MultiAligner(kind, device=0)
        si = al.add_slice(cfg)
        if side == "oracle":
            al.set_fixed(si, *meas.get()); al.set_moving(si, *clipped.get())
        else:
            cp, cn, k = clipped.device_arrays()
            mp, mn, m = meas.device_arrays()
            assert mn is not None and cn is not None and m == rs["result"]["scene_size"]
            al.set_cloud_device("set_moving", si, cp, 16, cn, 16, k, kept=True)
            al.set_cloud_device("set_fixed", si, mp, 16, mn, 16, m, kept=True)
        al.set_moving_in_fixed(I)
        al.compute()
        assert al.status() == abi.SUCCESS
        mg = mapping.MergerCorrespondenceHomo(b)
        mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(_inverse(al.moving_in_fixed(), dim))
        if side == "gpu":
            out = mg.compute_from_aligner(al, si, clipped)
        else:
            c = al.correspondences(si)
            g = clipped.global_indices()
            flipped = np.zeros(len(c), dtype=c.dtype)
            flipped["fixed_idx"], flipped["moving_idx"], flipped["response"] = g[c["moving_idx"]], c["fixed_idx"], c["response"]
            mg.set_correspondences(flipped)
            out = mg.compute()
        runs[side] = (out, scene.get(), al)
    (outr, (pr, nrr), alr), (outg, (pg, ng), alg) = runs["oracle"], runs["gpu"]
    assert_same_run(alr, alg)
    print(dim, alg.iteration_stats()[-1]["num_correspondences"], outg)
    assert alg.iteration_stats()[-1]["num_correspondences"] > n // 2
    assert outr == outg and outg["num_merged"] > 100
    assert nr.same_bits(pr, pg) and nr.same_bits(nrr, ng)
