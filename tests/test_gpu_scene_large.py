"""GPU: the scene kernels past their launch cap and the exclusive scan past its first level (tests/scene_large_cases.py says where
the two thresholds come from), BIT FOR BIT against the oracle, the restatements and plain numpy on the inputs -- never against a
second device run.

  A  scan, second level   ball clip of T^2, T^2 + 1 and 2 T^2 + T + 1 points whose keep flags are set by geometry: the global
                          indices are np.flatnonzero(mask), the clipped scene is the oracle's; fresh, repeated, and empty
  B  clippers past CAP    ball (oracle), projective and scan (restatements) on CAP + 2 T + 1 points with normals, descriptors
                          and intensities; two or three clips into one clipped scene
  C  voxelize past CAP    more than CAP occupied cells (C1 centroid / normals / dim 3, C2 first / dim 2 / min_points 2), and
                          T^2 + T + 1 lattice points that each own a cell (C3: both scans of the call take the second level)
  D  normals past CAP     a 2-D curve of CAP + 2 T + 1 points (D1), and 40 000 surface points behind CAP dead ones (D2)

Seconds of the CPU reference per case (one core of the development machine; the device's share is small beside it):
  A  building the cloud 0.3 (T^2, dim 2) to 0.8 (2 T^2 + T + 1, dim 3); the oracle's three clips 0.15 to 0.35
  B  ball (oracle) under 0.1 per clip; clip_projective 0.08 per clip; clip_scan 0.16 per clip
  C  voxelize_vectorised: C1 0.5, C2 0.25, C3 2.9
  D  normals_restatement.estimate_normals: D1 7.6, D2 1.5 per run
"""
import time

import numpy as np
import pytest

import clip_projective_restatement as cr
import clip_scan_restatement as cs
import normals_restatement as nr
import scene_large_cases as lc
import voxel_restatement as vr
from srrg2_slam_interfaces_amd import mapping

pytestmark = pytest.mark.gpu
F = np.float32
T, CAP = lc.T, lc.CAP
MODES = {vr.CENTROID: "centroid", vr.FIRST: "first"}


class _Clock:
    """seconds spent on the reference and on everything else, printed (pytest -s); nothing is asserted about time"""

    def __init__(self, what):
        self.what, self.t0, self.ref = what, time.perf_counter(), 0.0

    def reference(self, fn, *a, **kw):
        t = time.perf_counter()
        out = fn(*a, **kw)
        self.ref += time.perf_counter() - t
        return out

    def done(self):
        total = time.perf_counter() - self.t0
        print("%s: %.2f s, of which the reference %.2f s" % (self.what, total, self.ref))


def _same_scene(a, b):
    pa, na = a.get()
    pb, nb = b.get()
    assert pa.shape == pb.shape
    assert pa.tobytes() == pb.tobytes()
    assert na.tobytes() == nb.tobytes()


def _ball(b, full, clipped, pose, range_max):
    cl = mapping.SceneClipperBall(b, range_max=range_max)
    cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
    cl.compute()
    return cl


def _close(*scenes):
    for s in scenes:
        s.close()


# ---- A ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.SCAN_SIZES)
@pytest.mark.parametrize("dim", [3, 2])
def test_scan_second_level_through_the_ball_clip(oracle, product, dim, n):
    """k_scan_sums' carry: a wrong one shifts every offset behind tile 2048.  One clipped handle takes the clip three times:
    fresh (the scatter waits for the total), again (launched behind the scan, the total unseen), and from a pose that keeps
    nothing"""
    clock = _Clock("A dim %d n %d" % (dim, n))
    c = clock.reference(lc.scan_case, n, dim)
    want = np.flatnonzero(c["mask"])
    pairs = []
    for b in (oracle.scene_binding(), product.scene_binding(0)):
        full, clipped = mapping.Scene(b, dim), mapping.Scene(b, dim)
        full.set(c["points"], c["normals"])
        pairs.append((b, full, clipped))
    (bo, full_o, clip_o), (bg, full_g, clip_g) = pairs
    for step, (pose, expect) in enumerate(((c["pose"], want), (c["pose"], want), (c["pose_far"], want[:0]))):
        ref = clock.reference(_ball, bo, full_o, clip_o, pose, c["range_max"])
        gpu = _ball(bg, full_g, clip_g, pose, c["range_max"])
        assert ref.status() == gpu.status() == mapping.CLIPPER_SUCCESSFUL
        g = gpu.global_indices()
        bad = np.flatnonzero(g[:min(len(g), len(expect))] != expect[:min(len(g), len(expect))])
        assert np.array_equal(g, expect), (step, len(g), len(expect), "first difference at kept point %s" % bad[:1])
        assert clip_g.size() == clip_o.size() == len(expect)
        _same_scene(clip_o, clip_g)
    _close(full_o, clip_o, full_g, clip_g)
    clock.done()


# ---- B ----------------------------------------------------------------------------------------------------------------------
def _full_scene(product, c, dim):
    """the case's cloud with every field on the device; the features' way in (k_ingest_*) and out checked on the spot"""
    b = product.scene_binding(0)
    full, clipped = mapping.Scene(b, dim), mapping.Scene(b, dim)
    full.set(c["points"], c["normals"])
    full.set_features(c["descriptors"], c["intensity"])
    d, i = full.features()
    assert full.has_features() == (True, True)
    assert np.array_equal(d, c["descriptors"]) and i.tobytes() == c["intensity"].tobytes()
    return b, full, clipped


def _crosses_the_cap(g):
    return len(g) > T and g[-1] >= CAP and (g < CAP).any()


def _features_follow(clipped, c, what):
    g = clipped.global_indices()
    d, i = clipped.features()
    assert clipped.has_features() == (True, True), what
    assert np.array_equal(d, c["descriptors"][g]) and i.tobytes() == c["intensity"][g].tobytes(), what
    assert _crosses_the_cap(g), what


@pytest.mark.parametrize("dim", [3, 2])
def test_ball_clip_past_the_cap_with_features(oracle, product, dim):
    clock = _Clock("B ball dim %d" % dim)
    c = lc.clip_case(dim)
    b, full, clipped = _full_scene(product, c, dim)
    bo = oracle.scene_binding()
    full_o, clip_o = mapping.Scene(bo, dim), mapping.Scene(bo, dim)
    full_o.set(c["points"], c["normals"])
    for k, pose in enumerate(lc.ball_poses(dim)):
        ref = clock.reference(_ball, bo, full_o, clip_o, pose, lc.BALL_RANGE[dim])
        gpu = _ball(b, full, clipped, pose, lc.BALL_RANGE[dim])
        assert ref.status() == gpu.status() == mapping.CLIPPER_SUCCESSFUL
        assert np.array_equal(ref.global_indices(), gpu.global_indices()), k
        _same_scene(clip_o, clipped)
        _features_follow(clipped, c, ("ball", dim, k))
    _close(full, clipped, full_o, clip_o)
    clock.done()


def _check_clip(clipped, r, res, c, same_bits, what):
    assert res == {k: r[k] for k in ("status", "num_valid", "num_in_view", "num_kept")}, (what, res)
    assert clipped.size() == r["num_kept"], what
    assert np.array_equal(clipped.global_indices(), r["global_indices"]), what
    pts, nrm = clipped.get()
    assert same_bits(pts, r["points"]) and same_bits(nrm, r["normals"]), what
    d, i = clipped.features()
    assert np.array_equal(d, r["descriptors"]) and same_bits(i, r["intensity"]), what
    _features_follow(clipped, c, what)


def test_projective_clip_past_the_cap_with_features(product):
    """occlusion on (k_view_min, k_view_flag<PinholeView, true>), then off, into one clipped scene"""
    clock = _Clock("B projective")
    c = lc.clip_case(3)
    b, full, clipped = _full_scene(product, c, 3)
    for pose, sensor, margin in lc.PROJECTIVE_RUNS:
        cl = mapping.SceneClipperProjective(b)
        cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
        cl.set_camera_matrix(lc.CAMERA_K)
        if sensor is not None:
            cl.set_sensor_in_robot(sensor)
        cl.params.image_rows, cl.params.image_cols = lc.CAMERA_ROWS, lc.CAMERA_COLS
        cl.params.depth_min, cl.params.depth_max = 0.4, 8.0
        cl.params.occlusion_margin = margin
        res = cl.compute()
        r = clock.reference(cr.clip_projective, c["points"], pose, lc.CAMERA_K, lc.CAMERA_ROWS, lc.CAMERA_COLS, 0.4, 8.0,
                            sensor_in_robot=sensor, occlusion_margin=margin, normals=c["normals"], descriptors=c["descriptors"],
                            intensity=c["intensity"])
        _check_clip(clipped, r, res, c, cr.same_bits, ("projective", margin))
        assert margin < 0 or r["num_kept"] < r["num_in_view"]  # occlusion removed points
    _close(full, clipped)
    clock.done()


def test_scan_clip_past_the_cap_with_features(product):
    """occlusion with the per-beam minimum in LDS tables (k_view_min_lds), in global memory (k_view_min: 100 000 beams), and
    off, into one clipped scene"""
    clock = _Clock("B scan")
    c = lc.clip_case(2)
    b, full, clipped = _full_scene(product, c, 2)
    paths = []
    for beams, a0, inc, pose, sensor, margin in lc.SCAN_RUNS:
        cl = mapping.SceneClipperScan(b)
        cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(pose)
        if sensor is not None:
            cl.set_sensor_in_robot(sensor)
        cl.params.angle_min, cl.params.angle_increment, cl.params.num_beams = a0, inc, beams
        cl.params.range_min, cl.params.range_max = lc.SCAN_CLIP_RANGES
        cl.params.occlusion_margin = margin
        res = cl.compute()
        r = clock.reference(cs.clip_scan, c["points"], pose, a0, inc, beams, *lc.SCAN_CLIP_RANGES, sensor_in_robot=sensor,
                            occlusion_margin=margin, normals=c["normals"], descriptors=c["descriptors"], intensity=c["intensity"])
        _check_clip(clipped, r, res, c, cs.same_bits, ("scan", beams, margin))
        if margin >= 0:
            assert r["num_kept"] < r["num_in_view"]
            paths.append(lc.scan_minimum_in_lds(lc.N_CAP, beams))
    assert sorted(paths) == [False, True]
    _close(full, clipped)
    clock.done()


# ---- C ----------------------------------------------------------------------------------------------------------------------
def _check_voxels(product, clock, pts, leaf, dim, mode, normals=None, features=False, min_points=1, tag=""):
    b = product.scene_binding(0)
    src, dst = mapping.Scene(b, dim), mapping.Scene(b, dim)
    src.set(pts, normals)
    desc = inten = None
    if features:
        desc, inten = lc.features(len(pts), 3)
        src.set_features(desc, inten)
    res, counts = src.voxelize(dst, leaf, mode=MODES[mode], min_points=min_points, return_counts=True)
    r = clock.reference(lc.voxelize_vectorised, pts, leaf, dim=dim, mode=mode, min_points=min_points, normals=normals,
                        descriptors=desc, intensity=inten)
    assert res == r["result"], (tag, res, r["result"])
    assert dst.size() == r["result"]["num_voxels"], tag
    assert np.array_equal(dst.global_indices(), r["global_indices"]), tag
    assert np.array_equal(counts, r["counts"]), tag
    c, nrm = dst.get()
    assert vr.same_bits(c, r["points"]), (tag, np.flatnonzero((c.view(np.uint32) != r["points"].view(np.uint32)).any(1))[:10])
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
    assert vr.same_bits(src.get()[0], pts), tag  # the source is left alone
    _close(src, dst)
    return r


def test_voxelize_more_cells_than_the_cap_centroid_3d(product):
    """C1: k_vox_finish strides over the occupied cells -- more than CAP of them, holding one, two or three points"""
    clock = _Clock("C1")
    c = lc.voxel_many_cells(3)
    r = _check_voxels(product, clock, c["points"], c["leaf"], 3, vr.CENTROID, c["normals"], features=True, tag="C1")
    res = r["result"]
    assert res["num_voxels"] == res["num_occupied"] == c["num_cells"] > CAP and res["max_points_per_voxel"] == 3
    assert 0 < res["num_with_normal"] < res["num_voxels"] and (r["global_indices"] >= CAP).sum() > T
    clock.done()


def test_voxelize_more_cells_than_the_cap_first_2d_min_points(product):
    """C2: min_points = 2 flags most of the cells 0"""
    clock = _Clock("C2")
    c = lc.voxel_many_cells(2)
    r = _check_voxels(product, clock, c["points"], c["leaf"], 2, vr.FIRST, None, features=True, min_points=2, tag="C2")
    res = r["result"]
    assert res["num_occupied"] == c["num_cells"] > CAP and T < res["num_voxels"] == c["num_twos"] + c["num_threes"]
    clock.done()


def test_voxelize_both_scans_take_the_second_level(product):
    """C3: T^2 + T + 1 points, each in a cell of its own: the scan of the cell heads and the scan of the keep flags both run past
    T tiles"""
    clock = _Clock("C3")
    pts, _ = lc.voxel_lattice()
    n = T * T + T + 1
    r = _check_voxels(product, clock, pts, 1.0, 3, vr.FIRST, tag="C3")
    assert r["result"]["num_voxels"] == r["result"]["num_occupied"] == n == len(pts)
    clock.done()


# ---- D ----------------------------------------------------------------------------------------------------------------------
def _check_normals(product, clock, pts, radius, dim, drop, viewpoint, features, tag):
    b = product.scene_binding(0)
    s = mapping.Scene(b, dim)
    s.set(pts)
    desc = inten = None
    if features:
        desc, inten = lc.features(len(pts), 3)
        s.set_features(desc, inten)
    res, curv = s.estimate_normals(radius, viewpoint=viewpoint, drop=drop, return_curvature=True, max_curvature=lc.NORMALS_MAX_CURVATURE)
    r = clock.reference(nr.estimate_normals, pts, radius, dim=dim, viewpoint=viewpoint, drop=drop, max_curvature=lc.NORMALS_MAX_CURVATURE)
    assert res == r["result"], (tag, res, r["result"])
    assert nr.same_bits(curv, r["curvature"]), tag
    c, m = s.get()
    assert s.size() == len(r["kept"]), tag
    assert nr.same_bits(c, r["points_out"]), tag
    assert nr.same_bits(m, r["normals_out"]), (tag, np.flatnonzero((m.view(np.uint32) != r["normals_out"].view(np.uint32)).any(1))[:10])
    if drop:
        assert np.array_equal(s.global_indices(), r["kept"]), tag
    if features:
        d, i = s.features()
        assert nr.same_bits(d, desc[r["kept"]]) and nr.same_bits(i, inten[r["kept"]]), tag
    _close(s)
    res = r["result"]
    assert res["num_with_normal"] > 0.5 * res["num_finite"] and res["num_too_few"] > 0, (tag, res)
    assert res["num_degenerate"] + res["num_too_curved"] > 0, (tag, res)
    return r


def test_normals_of_a_curve_past_the_cap(product):
    """D1: more than CAP finite points: k_grid_keys, k_nrm_gather, k_nrm_flag, k_nrm_scatter and the feature moves on their
    second trip"""
    clock = _Clock("D1")
    c = lc.normals_curve()
    r = _check_normals(product, clock, c["points"], c["radius"], 2, True, None, True, "D1")
    assert r["result"]["num_finite"] > CAP and r["result"]["scene_size"] > CAP and r["kept"][-1] >= CAP
    clock.done()


@pytest.mark.parametrize("drop", [True, False])
def test_normals_of_a_surface_behind_a_dead_head(product, drop):
    """D2: every point that takes part has a scene index of CAP or more: the 3-D keys / flag / scatter kernels do all their work
    on the second trip"""
    clock = _Clock("D2 drop %s" % drop)
    c = lc.normals_behind_a_dead_head()
    r = _check_normals(product, clock, c["points"], c["radius"], 3, drop, None if drop else lc.NORMALS_VIEW, True, ("D2", drop))
    assert r["result"]["num_finite"] == 40_000 and (not drop or r["kept"][0] >= CAP)
    clock.done()
