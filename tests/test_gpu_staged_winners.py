"""Winners of the staged neighbours of the converged passes ("The converged pass", item 12; csrc/kernels.hip,
icp_step_fast_body).  A point whose ball holds a few candidates is decided by the lane that owns it, among the candidates the team
kept apart during the wait; a wave with more than four thin lanes stages its near-ties alone; a winner that is not the neighbour the
point had is fetched.  None of this is a condition of correctness: twins, triplets, a pass that still moves and degenerate points
must give the oracle's bits, with fused control steps and with control launches.  Which way the points went is proven on the
-DSRRG2_FUSED_STALL build, whose counters the last test reads."""
import os
import subprocess
import sys

import pytest

import staged_neighbour_scenarios as sc
import staged_winner_scenarios as sw
from srrg2_slam_interfaces_amd import _abi as abi

pytestmark = pytest.mark.gpu

BOTH = [sc.FUSED, sc.UNFUSED]
K3, K2 = abi.SE3_QUAT_RIGHT, abi.SE2_RIGHT


@pytest.mark.parametrize("kind,slice_kind", [(K3, abi.SLICE_P2PLANE), (K3, abi.SLICE_P2P), (K2, abi.SLICE_P2PLANE)])
def test_twins(oracle, product, kind, slice_kind):
    """(the point-to-point slice carries no normal; the runner-up becomes the neighbour between passes)"""
    d, near_ties = sc.with_twins(sc.pair(2 if kind == K2 else 3))
    assert near_ties >= 32, near_ties
    sc.run_all(oracle, product, kind, slice_kind, d, BOTH)


def test_triplets(oracle, product):
    """three candidates inside the certificate's safety factors: the third one can win"""
    d, near_ties = sw.with_triplets(sc.pair(3))
    assert near_ties >= 32, near_ties  # (moving points with (d3 - d1) / d1 < 3e-5 at the ground truth)
    sc.run_all(oracle, product, K3, abi.SLICE_P2PLANE, d, BOTH)


def test_twins_in_passes_that_still_move(oracle, product):
    """the converged-pass kernel from iteration 1 on: waves with more than four thin lanes stage their near-ties alone"""
    d, _ = sc.with_twins(sc.pair(3))
    sc.run_all(oracle, product, K3, abi.SLICE_P2PLANE, d, [dict(sc.FUSED, fast_from_iteration=1), sc.UNFUSED])


def test_twins_and_edges(oracle, product):
    """NaN coordinates, nothing inside the gate, points outside the grid; an inlier-only run and a termination criterion that stops
    in the middle of the converged passes"""
    d, _ = sc.with_twins(sc.pair(3))
    d = sc.with_edges(d)
    runs = sc.run_all(oracle, product, K3, abi.SLICE_P2PLANE, d, BOTH, max_iterations=14, criterion=True, inlier_only=True)
    assert 3 < len(runs[0].iteration_stats()) < 28  # (the criterion fired, after the passes had converged)


def test_counters_of_the_stall_build():
    """the same scenarios on the library whose designated wave is delayed, bit for bit, and its counters: decisions by the owner alone,
    a changed neighbour that is fetched, lanes staged under the near-tie-only rule"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stall = os.path.join(root, "srrg2_slam_interfaces_amd", "lib", "libsrrg2_slam_amd_stall.so")
    assert os.path.exists(stall), "build it with `make -C srrg2_slam_interfaces_amd/csrc stall` (__graft_entry__.build() does)"
    env = dict(os.environ, SRRG2_AMD_LIB=stall)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers_scripts", "staged_winners_check.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "WINNERS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
