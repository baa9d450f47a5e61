"""CPU: the scene oracle (oracle/o_scene.c) against an independent numpy restatement of
MergerCorrespondenceHomo_::compute() (S/mapping/merger_correspondence_homo_impl.cpp:11-125) and of the ball clipper,
in 3-D and 2-D (SE(2): the 2-D laser tracker's MergerCorrespondencePointNormal2f), with and without normals."""
import numpy as np
import pytest

from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn

f32 = np.float32


def _dim_of(T):
    """SE(3) rows of [R|t] are 3x4, SE(2) ones 3x3"""
    return 3 if np.shape(T)[1] == 4 else 2


def _xform(T, p):
    """3-D: ((r0 x + r1 y) + r2 z) + t; 2-D: (r0 x + r1 y) + t -- in float32, the order of o_scene.c"""
    T = np.asarray(T, f32)
    if _dim_of(T) == 2:
        x, y = f32(p[0]), f32(p[1])
        return np.array([f32(f32(T[r, 0] * x) + f32(T[r, 1] * y)) + T[r, 2] for r in range(2)], f32)
    x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
    return np.array([f32(f32(f32(T[r, 0] * x) + f32(T[r, 1] * y)) + f32(T[r, 2] * z)) + T[r, 3] for r in range(3)], f32)


def _rot(T, n):
    T = np.asarray(T, f32)
    if _dim_of(T) == 2:
        x, y = f32(n[0]), f32(n[1])
        return np.array([f32(T[r, 0] * x) + f32(T[r, 1] * y) for r in range(2)], f32)
    x, y, z = f32(n[0]), f32(n[1]), f32(n[2])
    return np.array([f32(f32(T[r, 0] * x) + f32(T[r, 1] * y)) + f32(T[r, 2] * z) for r in range(3)], f32)


def _sqnorm(d):
    """(dx dx + dy dy) + dz dz; in 2-D z is 0 on both sides, and adding 0 changes no comparison"""
    s = f32(f32(d[0] * d[0]) + f32(d[1] * d[1]))
    return f32(s + f32(d[2] * d[2])) if len(d) == 3 else s


def _valid(p):
    """Valid <=> finite coordinates (x, y in 2-D; x, y, z in 3-D)"""
    return bool(np.all(np.isfinite(p)))


def merge_reference(scene_p, scene_n, meas_p, meas_n, T, corr, params):
    """pure-python walk of the reference loop; corr = list of (fixed_idx, moving_idx, response) or None.
    scene_n / meas_n None: a cloud without normals (its normals read as zero, a measurement without them writes zeros)."""
    dim = _dim_of(T)
    zero = np.zeros(dim, f32)
    sp = [np.asarray(p, f32).copy() for p in scene_p]
    sn = [zero.copy() for _ in scene_p] if scene_n is None else [np.asarray(n, f32).copy() for n in scene_n]
    mnrm = (lambda i: zero.copy()) if meas_n is None else (lambda i: np.asarray(meas_n[i], f32).copy())
    added = merged_n = 0
    with np.errstate(invalid="ignore", over="ignore"):
        if corr is None:
            for i, p in enumerate(meas_p):
                if _valid(p):
                    sp.append(_xform(T, p)); sn.append(_rot(T, mnrm(i))); added += 1
        else:
            merged = set()
            for (s, m, resp) in corr:
                if not (f32(resp) < f32(params.maximum_response)):
                    continue
                q = _xform(T, meas_p[m])
                d2 = _sqnorm(q - sp[s])
                if not (d2 < f32(params.maximum_distance_geometry_squared)):
                    continue
                sn[s] = mnrm(m)  # :71 copied as it is: the normal is NOT rotated into the scene
                sp[s] = ((q + sp[s]) * f32(0.5)).astype(f32)
                merged.add(m)
            merged_n = len(merged)
            if merged_n < params.target_number_of_merges:
                for i, p in enumerate(meas_p):
                    if i in merged or not _valid(p):
                        continue
                    sp.append(_xform(T, p)); sn.append(_rot(T, mnrm(i))); added += 1
    return np.array(sp, f32).reshape(-1, dim), np.array(sn, f32).reshape(-1, dim), merged_n, added


def clip_reference(sp, sn, pose, range_max):
    """the ball clipper: keep Valid points whose squared distance to the robot is <= range^2, in scene order, expressed in the
    robot frame; normals rotated (zero when the scene has none).  Returns (global indices, points, normals)."""
    from oracle import pyoracle

    dim = _dim_of(pose)
    L = pyoracle.se3_inverse(pose) if dim == 3 else pyoracle.se2_inverse(pose)
    r2 = f32(f32(range_max) * f32(range_max))
    keep, pts, nrm = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(sp)):
            if not _valid(sp[i]):
                continue
            q = _xform(L, sp[i])
            if _sqnorm(q) <= r2:
                keep.append(i); pts.append(q); nrm.append(np.zeros(dim, f32) if sn is None else _rot(L, sn[i]))
    return (np.array(keep, np.int32), np.array(pts, f32).reshape(-1, dim), np.array(nrm, f32).reshape(-1, dim))


def _clouds(seed, ns=300, nm=200):
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-2, 2, (ns, 3)).astype(f32)
    sn = rng.normal(size=(ns, 3)).astype(f32)
    T = syn.se3(np.array([0.1, -0.05, 0.02]), np.deg2rad(np.array([2.0, -1.0, 3.0]))).astype(f32)
    # measurement: noisy copies of some scene points expressed in the measurement frame + fresh points
    Ti = syn.se3_inv(T.astype(np.float64))
    idx = rng.integers(0, ns, nm)
    mp = (sp[idx].astype(np.float64) + rng.normal(scale=0.05, size=(nm, 3))) @ Ti[:, :3].T + Ti[:, 3]
    mp = mp.astype(f32)
    mn = rng.normal(size=(nm, 3)).astype(f32)
    mp[5] = np.nan  # invalid measurement point
    corr = [(int(idx[m]), m, float(rng.uniform(0, 80))) for m in range(nm) if m % 3 != 0]  # duplicates of fixed_idx included
    return sp, sn, mp, mn, T, corr


def _clouds_nd(seed, dim, ns=300, nm=200, normals=True):
    """_clouds in either dimension: a scene, a measurement of noisy scene points in the measurement frame (one of them
    NaN), correspondences with duplicates of fixed_idx, and the scene point of the first correspondence made NaN (hit, but
    never merged).  normals=False: neither cloud has normals."""
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-2, 2, (ns, dim)).astype(f32)
    sn = rng.normal(size=(ns, dim)).astype(f32)
    if dim == 3:
        T = syn.se3(np.array([0.1, -0.05, 0.02]), np.deg2rad(np.array([2.0, -1.0, 3.0]))).astype(f32)
        Ti = syn.se3_inv(T.astype(np.float64))
    else:
        T = syn.se2(0.1, -0.05, np.deg2rad(3.0)).astype(f32)
        Ti = np.linalg.inv(T.astype(np.float64))[:2]
    idx = rng.integers(0, ns, nm)
    mp = ((sp[idx].astype(np.float64) + rng.normal(scale=0.05, size=(nm, dim))) @ Ti[:, :dim].T + Ti[:, dim]).astype(f32)
    mn = rng.normal(size=(nm, dim)).astype(f32)
    mp[5] = np.nan  # invalid measurement point (m = 5 has a correspondence)
    corr = [(int(idx[m]), m, float(rng.uniform(0, 80))) for m in range(nm) if m % 3 != 0]
    corr[0] = (corr[0][0], corr[0][1], 1.0)
    sp[corr[0][0]] = np.nan  # a NaN scene point hit by a correspondence that passes the response test
    if not normals:
        sn = mn = None
    return sp, sn, mp, mn, T, corr


def _corr_array(corr):
    arr = np.zeros(len(corr), dtype=[("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
    for k, c in enumerate(corr):
        arr[k] = c
    return arr


def _run_oracle(oracle, sp, sn, mp, mn, T, corr, params):
    """sn / mn None: a scene / measurement set without normals; corr None: no correspondences set (ncorr < 0)"""
    b = oracle.scene_binding()
    dim = _dim_of(T)
    scene, meas = mapping.Scene(b, dim), mapping.Scene(b, dim)
    scene.set(sp, sn)
    meas.set(mp, mn)
    mg = mapping.MergerCorrespondenceHomo(b, params)
    mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(T)
    if corr is not None:
        mg.set_correspondences(_corr_array(corr))
    res = mg.compute()
    p, n = scene.get()
    return p, n, res, mg.status()


@pytest.mark.parametrize("target", [200, 20, 0])
def test_merge_matches_reference_walk(oracle, target):
    sp, sn, mp, mn, T, corr = _clouds(7)
    assert len({c[0] for c in corr}) < len(corr)  # the case has scene points hit more than once
    params = mapping.MergerParams(50.0, 0.25, target)
    p, n, res, status = _run_oracle(oracle, sp, sn, mp, mn, T, corr, params)
    rp, rn, merged_n, added = merge_reference(sp, sn, mp, mn, T, corr, params)
    assert status == mapping.MERGER_SUCCESS
    assert (res["num_merged"], res["num_added"], res["scene_size"]) == (merged_n, added, len(rp))
    assert p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes()
    assert merged_n > 20
    if target == 200:
        assert added > 0  # target not reached: unmerged valid points appended (:92-115)
    if target <= 20:
        assert added == 0


def test_merge_without_correspondences_appends_valid_points(oracle):
    sp, sn, mp, mn, T, _ = _clouds(8)
    p, n, res, status = _run_oracle(oracle, sp, sn, mp, mn, T, None, mapping.default_merger_params())
    rp, rn, _, added = merge_reference(sp, sn, mp, mn, T, None, mapping.default_merger_params())
    assert added == len(mp) - 1 and res["num_added"] == added
    assert p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes()


def test_merge_rejects_out_of_range_indices(oracle):
    sp, sn, mp, mn, T, corr = _clouds(9)
    with pytest.raises(RuntimeError):
        _run_oracle(oracle, sp, sn, mp, mn, T, [(len(sp), 0, 1.0)], mapping.default_merger_params())


def test_clip_ball(oracle):
    rng = np.random.default_rng(3)
    sp = rng.uniform(-10, 10, (2000, 3)).astype(f32)
    sn = rng.normal(size=(2000, 3)).astype(f32)
    sp[17] = np.inf
    pose = syn.se3(np.array([1.0, -2.0, 0.5]), np.deg2rad(np.array([10.0, 5.0, -20.0]))).astype(f32)
    b = oracle.scene_binding()
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    full.set(sp, sn)
    cl = mapping.SceneClipperBall(b, range_max=6.0)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    cl.compute()
    assert cl.status() == mapping.CLIPPER_SUCCESSFUL
    L = oracle.se3_inverse(pose)
    keep, pts, nrm = [], [], []
    for i in range(len(sp)):
        if not np.all(np.isfinite(sp[i])):
            continue
        q = _xform(L, sp[i])
        if f32(f32(f32(q[0] * q[0]) + f32(q[1] * q[1])) + f32(q[2] * q[2])) <= f32(f32(6.0) * f32(6.0)):
            keep.append(i); pts.append(q); nrm.append(_rot(L, sn[i]))
    p, n = clipped.get()
    assert np.array_equal(cl.global_indices(), np.array(keep, np.int32))
    assert p.tobytes() == np.array(pts, f32).tobytes() and n.tobytes() == np.array(nrm, f32).tobytes()
    assert 100 < len(keep) < 1500
    # empty scene -> Ready (scene_clipper.h:27)
    full.set(np.zeros((0, 3), f32))
    cl.compute()
    assert cl.status() == mapping.CLIPPER_READY and clipped.size() == 0


@pytest.mark.parametrize("normals", [True, False])
def test_clip_ball_2d(oracle, normals):
    rng = np.random.default_rng(4)
    sp = rng.uniform(-10, 10, (2000, 2)).astype(f32)
    sn = rng.normal(size=(2000, 2)).astype(f32) if normals else None
    sp[17] = np.inf
    sp[18, 1] = np.nan
    pose = syn.se2(1.0, -2.0, np.deg2rad(-20.0)).astype(f32)
    b = oracle.scene_binding()
    full, clipped = mapping.Scene(b, 2), mapping.Scene(b, 2)
    full.set(sp, sn)
    cl = mapping.SceneClipperBall(b, range_max=6.0)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    cl.compute()
    assert cl.status() == mapping.CLIPPER_SUCCESSFUL
    keep, pts, nrm = clip_reference(sp, sn, pose, 6.0)
    p, n = clipped.get()
    assert np.array_equal(cl.global_indices(), keep)
    assert p.tobytes() == pts.tobytes() and n.tobytes() == nrm.tobytes()
    assert 100 < len(keep) < 1500 and n.any() == normals


# ---- 2-D (SE(2), MergerCorrespondencePointNormal2f) and clouds without normals ---------------------------------------------
# (merger_correspondence_homo.h:36-39: the reference's two concrete mergers are the 2-D point+normal one and a 3-D one whose
# points carry no normals)
_CASES = {"2d": (2, True), "2d_no_normals": (2, False), "3d_no_normals": (3, False)}


def _expect(res, status, rp, merged_n, added, ncorr):
    assert status == mapping.MERGER_SUCCESS
    assert res == {"status": mapping.MERGER_SUCCESS, "num_correspondences": ncorr, "num_merged": merged_n,
                   "num_added": added, "scene_size": len(rp)}, res


@pytest.mark.parametrize("target", [200, 20, 0])
@pytest.mark.parametrize("case", sorted(_CASES))
def test_merge_2d_and_normal_free_match_reference_walk(oracle, case, target):
    dim, normals = _CASES[case]
    sp, sn, mp, mn, T, corr = _clouds_nd(17, dim, normals=normals)
    assert len({c[0] for c in corr}) < len(corr)  # scene points hit more than once
    params = mapping.MergerParams(50.0, 0.25, target)
    p, n, res, status = _run_oracle(oracle, sp, sn, mp, mn, T, corr, params)
    rp, rn, merged_n, added = merge_reference(sp, sn, mp, mn, T, corr, params)
    _expect(res, status, rp, merged_n, added, len(corr))
    assert p.shape == rp.shape and p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes()
    assert merged_n > 20
    assert (added > 0) == (target == 200)
    assert np.isnan(p[corr[0][0]]).all()  # the NaN scene point stays NaN: its d2 is NaN, never < the gate
    if not normals:
        assert not n.any()


@pytest.mark.parametrize("case", sorted(_CASES))
@pytest.mark.parametrize("ncorr", [-1, 0])
def test_merge_2d_and_normal_free_without_correspondences(oracle, case, ncorr):
    """ncorr < 0: no correspondences set, every Valid point is appended (:30-41); ncorr = 0: an empty set, merged 0 < target"""
    dim, normals = _CASES[case]
    sp, sn, mp, mn, T, _ = _clouds_nd(18, dim, normals=normals)
    corr = None if ncorr < 0 else []
    params = mapping.default_merger_params()
    p, n, res, status = _run_oracle(oracle, sp, sn, mp, mn, T, corr, params)
    rp, rn, merged_n, added = merge_reference(sp, sn, mp, mn, T, corr, params)
    _expect(res, status, rp, 0, added, max(ncorr, 0))
    assert added == len(mp) - 1
    assert p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes()


def test_merge_2d_merged_normal_is_not_rotated(oracle):
    """:71 copies the measurement point whole, so a merged 2-D normal stays in the measurement frame; an appended one is rotated
    into the scene (transformInPlace, :110)"""
    T = syn.se2(0.5, -0.25, np.deg2rad(30.0)).astype(f32)
    sp, sn = np.array([[0.5, -0.25]], f32), np.array([[0.0, 1.0]], f32)
    mp, mn = np.array([[0.01, 0.02], [3.0, 1.0]], f32), np.array([[1.0, 0.0], [0.0, 1.0]], f32)
    params = mapping.MergerParams(50.0, 0.25, 10)
    p, n, res, _ = _run_oracle(oracle, sp, sn, mp, mn, T, [(0, 0, 1.0)], params)
    assert (res["num_merged"], res["num_added"]) == (1, 1)
    assert n[0].tolist() == [1.0, 0.0]
    assert n[1].tobytes() == _rot(T, mn[1]).tobytes() and abs(float(n[1][0]) + 0.5) < 1e-6
    rp, rn, _, _ = merge_reference(sp, sn, mp, mn, T, [(0, 0, 1.0)], params)
    assert p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes()


@pytest.mark.parametrize("dim", [2, 3])
def test_merge_normals_flag_follows_the_reference(oracle, dim):
    """A fresh scene takes has_normals from the measurement; a scene set without normals keeps none, so a clip of it carries
    zero normals even where the merge wrote some into its arrays.  Checked through a clip after the merge."""
    sp, sn, mp, mn, T, corr = _clouds_nd(20, dim)
    pose = (syn.se3(np.array([0.2, 0.1, -0.1]), np.deg2rad(np.array([3.0, -2.0, 10.0]))) if dim == 3
            else syn.se2(0.2, 0.1, np.deg2rad(10.0))).astype(f32)
    params = mapping.MergerParams(50.0, 0.25, 10 ** 6)
    b = oracle.scene_binding()
    for scene_p, scene_n, c, has in ((np.zeros((0, dim), f32), None, None, True),  # fresh scene, measurement with normals
                                     (sp, None, corr, False)):                     # scene without normals, measurement with
        scene, meas, clipped = mapping.Scene(b, dim), mapping.Scene(b, dim), mapping.Scene(b, dim)
        scene.set(scene_p, scene_n)
        meas.set(mp, mn)
        mg = mapping.MergerCorrespondenceHomo(b, params)
        mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(T)
        if c is not None:
            mg.set_correspondences(_corr_array(c))
        mg.compute()
        p, n = scene.get()
        rp, rn, _, _ = merge_reference(scene_p, scene_n, mp, mn, T, c, params)
        assert p.tobytes() == rp.tobytes() and n.tobytes() == rn.tobytes() and n.any()
        cl = mapping.SceneClipperBall(b, range_max=1.5)
        cl.set_full_scene(scene); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
        cl.compute()
        keep, kp, kn = clip_reference(rp, rn if has else None, pose, 1.5)
        cp, cn = clipped.get()
        assert np.array_equal(cl.global_indices(), keep) and 20 < len(keep) < len(rp)
        assert cp.tobytes() == kp.tobytes() and cn.tobytes() == kn.tobytes()
        assert cn.any() == has
