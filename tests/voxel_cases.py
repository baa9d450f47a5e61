"""The "through the stack" case of the voxel-grid decimation, shared by its Python and its C++ GPU test: two clouds without
normals -> voxelize -> estimate_normals -> point-to-plane alignment.  The expected side is made by the restatements
(tests/voxel_restatement.py, tests/normals_restatement.py) and aligned by the oracle."""
import numpy as np

import normals_restatement as nr
import voxel_restatement as vr
from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

F = np.float32
LEAF, RADIUS, GATE, VIEW = 0.05, 0.16, 0.3, (0.0, 0.0, 3.0)


def clouds(dim=3, n=6000):
    """(map points, measurement points): the measurement is the map moved a little, with noise"""
    rng = np.random.default_rng(21)
    if dim == 3:
        P = np.concatenate([nr.surface("plane", n // 2, 1, 0.1), nr.surface("crossing", n - n // 2, 2, 0.1)])
        X = np.eye(4)
        X[:3, :] = np.asarray(syn.se3((0.02, -0.015, 0.01), np.deg2rad([0.5, -0.4, 0.8])), np.float64)[:3, :]
    else:
        P = np.concatenate([nr.surface("crossing", n // 2, 1, 0.1, 2), nr.surface("circle", n - n // 2, 2, 0.1, 2)])
        X = np.asarray(syn.se2(0.004, -0.003, np.deg2rad(0.4)), np.float64)
    M = ((P.astype(np.float64) @ X[:dim, :dim].T + X[:dim, dim]) + rng.normal(scale=2e-4, size=P.shape)).astype(F)
    return P, M


def leaf_and_radius(dim):
    return (LEAF, RADIUS) if dim == 3 else (0.004, 0.02)


def restated(points, dim, mode=vr.CENTROID):
    """voxelize -> estimate_normals(drop) by the restatements: (voxel dict, normals dict)"""
    leaf, radius = leaf_and_radius(dim)
    v = vr.voxelize(points, leaf, dim=dim, mode=mode)
    return v, nr.estimate_normals(v["points"], radius, dim=dim, viewpoint=VIEW, drop=True)


def oracle_run(oracle, dim, fixed, moving):
    """the oracle's point-to-plane alignment of two restatement-made clouds (normals dicts)"""
    kind = abi.SE3_QUAT_RIGHT if dim == 3 else abi.SE2_RIGHT
    al = oracle.OracleAligner(kind)
    si = al.add_slice(config(dim))
    al.set_fixed(si, fixed["points_out"], fixed["normals_out"])
    al.set_moving(si, moving["points_out"], moving["normals_out"])
    al.set_moving_in_fixed(syn.identity(dim))
    al.compute()
    return al


def config(dim):
    kind = abi.SE3_QUAT_RIGHT if dim == 3 else abi.SE2_RIGHT
    return cue_config(kind, abi.SLICE_P2PLANE, GATE if dim == 3 else 0.05, robust=abi.ROBUST_CAUCHY)
