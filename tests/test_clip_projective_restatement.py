"""CPU: the numpy restatement of the projective clipper (tests/clip_projective_restatement.py) on hand-made scenes with known
answers, and its consistency with the oracle's projective finder: an aligner fed the clipped cloud (margin 0) finds, mapped
through the global indices, exactly the correspondences it finds on the whole robot-frame cloud."""
import numpy as np
import pytest

import clip_projective_cases as cases
import clip_projective_restatement as cr

F = np.float32
I34 = np.eye(3, 4, dtype=F)
# 6 x 8 image; fx = fy = 8 keeps the edge cases exact in float32
K = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1.0]], F)
ROWS, COLS = 6, 8


def _clip(points, **kw):
    kw.setdefault("robot_in_local_map", I34)
    return cr.clip_projective(np.asarray(points, F), K=K, rows=ROWS, cols=COLS, **kw)


def test_depth_range_and_points_behind_the_camera():
    pts = [[0, 0, -1.0], [0, 0, 0.4], [0, 0, 8.0], [0, 0, 0.39999], [0, 0, 8.001], [0, 0, 0.0]]
    r = _clip(pts)
    assert list(r["global_indices"]) == [1, 2]  # exactly on depth_min and on depth_max: both kept
    assert (r["num_valid"], r["num_in_view"], r["num_kept"], r["status"]) == (6, 2, 2, cr.CLIPPER_SUCCESSFUL)
    assert list(r["pix"][[1, 2]]) == [3 * COLS + 4] * 2  # u = 3.5, v = 2.5 -> column 4, row 3
    assert cr.same_bits(r["points"], np.asarray(pts, F)[[1, 2]])


def test_image_edges():
    # u + 0.5 == cols: out; u + 0.5 == 0: column 0; the same for rows
    pts = [[0.5, 0, 1.0], [-0.5, 0, 1.0], [0, 0.375, 1.0], [0, -0.375, 1.0], [0.49, 0, 1.0]]
    r = _clip(pts)
    assert list(r["global_indices"]) == [1, 3, 4]
    assert list(r["pix"]) == [-1, 3 * COLS + 0, -1, 0 * COLS + 4, 3 * COLS + 7]


def test_invalid_points_keep_their_index_out_of_the_result():
    pts = [[np.nan, 0, 1], [0, 0, 1.0], [0, np.inf, 1], [0, 0, -np.inf], [0.1, 0.1, 2.0]]
    inten = np.arange(5, dtype=F)
    desc = np.arange(5 * 32, dtype=np.uint8).reshape(5, 32)
    r = _clip(pts, intensity=inten, descriptors=desc)
    assert list(r["global_indices"]) == [1, 4] and r["num_valid"] == 2 and r["num_in_view"] == 2
    assert list(r["intensity"]) == [1.0, 4.0] and np.array_equal(r["descriptors"], desc[[1, 4]])
    assert _clip(np.zeros((0, 3), F))["status"] == cr.CLIPPER_READY


def test_ties_at_margin_zero_are_all_kept():
    pts = [[0.01, 0, 1.0], [0.02, 0, 1.0], [0.015, 0, 1.0000001], [0.0, 0, 1.5]]
    r = _clip(pts, occlusion_margin=0.0)
    assert len(set(r["pix"])) == 1  # one pixel
    assert list(r["global_indices"]) == [0, 1]
    assert list(_clip(pts, occlusion_margin=0.5)["global_indices"]) == [0, 1, 2, 3]
    assert list(_clip(pts, occlusion_margin=0.4)["global_indices"]) == [0, 1, 2]


def _two_walls():
    rr, cc = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    ray = np.stack([(cc - 3.5) / 8.0, (rr - 2.5) / 8.0, np.ones(cc.shape)], -1).reshape(-1, 3)
    near, far = ray * 1.0, ray * 2.0
    extra = np.array([[0, 0, -2.0], [50.0, 0, 1.0], [np.nan, 0, 1.0]])
    pts = np.concatenate([far[::2], near, extra, far[1::2]])
    is_near = np.zeros(len(pts), bool)
    is_near[len(far[::2]):len(far[::2]) + len(near)] = True
    return pts.astype(F), is_near


def test_near_wall_hides_far_wall():
    pts, is_near = _two_walls()
    r0 = _clip(pts, occlusion_margin=0.0)
    assert np.array_equal(r0["global_indices"], np.flatnonzero(is_near))
    assert 0 < r0["num_kept"] < r0["num_in_view"] < r0["num_valid"] < len(pts)
    r2 = _clip(pts, occlusion_margin=1.5)  # larger than the gap between the walls
    assert r2["num_kept"] == r2["num_in_view"] == 2 * ROWS * COLS
    for frustum in (_clip(pts), _clip(pts, occlusion_margin=np.inf)):
        assert np.array_equal(frustum["global_indices"], r2["global_indices"])
    assert _clip(pts, occlusion_margin=0.9)["num_kept"] == r0["num_kept"]


def test_sensor_in_robot_and_robot_in_local_map():
    S = cases.SENSOR_IN_ROBOT
    L = np.array([[1, 0, 0, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]], F)  # the robot stands at x = 1 in the local map
    pts = np.array([[3.5, 0, 0.25],     # robot (2.5, 0, 0.25) = camera (0, 0, 2): the image centre
                    [3.5, -0.25, 0.25],  # camera (0.25, 0, 2): u = 4.5
                    [0.0, 0, 0.25],     # behind the camera
                    [1.0, 0, 3.0]], F)  # above the robot: camera z = -0.5
    nrm = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, 1.0]], F)
    r = cr.clip_projective(pts, L, K, ROWS, COLS, sensor_in_robot=S, normals=nrm)
    assert list(r["global_indices"]) == [0, 1]
    assert list(r["pix"][:2]) == [3 * COLS + 4, 3 * COLS + 5] and list(r["depth"][:2]) == [2.0, 2.0]
    # output in the ROBOT frame, normals rotated by the (pure translation) local map transform
    assert cr.same_bits(r["points"], [[2.5, 0, 0.25], [2.5, -0.25, 0.25]]) and cr.same_bits(r["normals"], nrm[:2])
    # a rotated robot: normals turn with the points
    Lr = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0]], F)  # robot yawed by +90 degrees
    q = cr.clip_projective(np.array([[0, 2.5, 0.25]], F), Lr, K, ROWS, COLS, sensor_in_robot=S, normals=np.array([[0, 1.0, 0]], F))
    assert q["num_kept"] == 1 and cr.same_bits(q["points"], [[2.5, 0, 0.25]]) and cr.same_bits(q["normals"], [[1.0, 0, 0]])


@pytest.mark.parametrize("sensor", [None, cases.SENSOR_IN_ROBOT], ids=["identity", "sensor_in_robot"])
def test_clipped_cloud_gives_the_oracle_the_same_correspondences(oracle, sensor):
    d = cases.c3_layers(sensor_in_robot=sensor)
    r = cr.clip_projective(d["map"], I34, d["K"], d["rows"], d["cols"], d["depth_min"], d["depth_max"], sensor_in_robot=sensor,
                           occlusion_margin=0.0, normals=d["map_normals"])
    assert 0 < r["num_kept"] < r["num_in_view"] < r["num_valid"] == len(d["map"])
    assert r["num_kept"] < 0.4 * len(d["map"])  # the hidden layer and the one behind the camera are gone
    c_full = cases.first_association(oracle.OracleAligner, d, d["map"], d["map_normals"], sensor)
    c_clip = cases.first_association(oracle.OracleAligner, d, r["points"], r["normals"], sensor)
    assert len(c_full) > 5000
    cases.assert_same_association(c_clip, r["global_indices"], c_full)
