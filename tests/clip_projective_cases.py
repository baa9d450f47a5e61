"""Shared builders of the projective clipper's tests (CPU: restatement against the oracle; GPU: library against both)."""
import numpy as np

from helpers import projective_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

F = np.float32
KIND = abi.SE3_QUAT_RIGHT

# the camera looks along the robot's x axis: camera z = robot x, camera x = robot -y, camera y = robot -z
SENSOR_IN_ROBOT = np.array([[0, 0, 1, 0.5], [-1, 0, 0, 0.0], [0, -1, 0, 0.25]], F)


def c3_layers(rows=120, cols=160, sensor_in_robot=None, seed=5):
    """A C3-style pair at reduced resolution whose moving cloud is a local map in the ROBOT frame: the camera-2 render, a copy
    0.3 m behind it (hidden from the camera) and a copy behind the camera, shuffled so that scene order mixes the three."""
    d = syn.rgbd_pair(rows=rows, cols=cols)
    cam, nrm = d["moving"].astype(np.float64), d["moving_normals"].astype(np.float64)
    pts = np.concatenate([cam, cam + [0.0, 0.0, 0.3], cam * [1.0, 1.0, -1.0]])
    nrm = np.concatenate([nrm, nrm, nrm])
    order = np.random.default_rng(seed).permutation(len(pts))
    pts, nrm = pts[order], nrm[order]
    if sensor_in_robot is not None:
        S = np.asarray(sensor_in_robot, np.float64)
        pts, nrm = pts @ S[:, :3].T + S[:, 3], nrm @ S[:, :3].T
    d["map"], d["map_normals"] = np.ascontiguousarray(pts, F), np.ascontiguousarray(nrm, F)
    return d


def first_association(make_aligner, d, moving, normals, sensor_in_robot=None, gate=0.05):
    """correspondences of ONE iteration of the projective point-to-plane slice, guess at identity"""
    al = make_aligner()
    si = al.add_slice(projective_config(KIND, abi.SLICE_P2PLANE, d, gate=gate))
    if sensor_in_robot is not None:
        al.set_sensor_in_robot(si, sensor_in_robot)
    al.set_params(max_iterations=1)
    al.set_fixed(si, d["fixed"], d["fixed_normals"])
    al.set_moving(si, moving, normals)
    al.set_moving_in_fixed(syn.identity(3))
    al.compute()
    return al.correspondences(si)


def assert_same_association(c_clip, global_indices, c_full):
    """the clipped cloud's correspondences, mapped through the clip's global indices, are the whole cloud's"""
    assert len(c_full) > 0 and len(c_clip) == len(c_full), (len(c_clip), len(c_full))
    assert np.array_equal(global_indices[c_clip["moving_idx"]], c_full["moving_idx"])
    assert np.array_equal(c_clip["fixed_idx"], c_full["fixed_idx"])
    assert c_clip["response"].tobytes() == c_full["response"].tobytes()
