"""srrg2_align_batch_slices without a GPU: the declaration, the ctypes mirror of its struct, and the defining loop the oracle
backend runs for MultiAligner.compute_batch_slices."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import cue_config, prior_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import loop_detector as ld
from srrg2_slam_interfaces_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srrg2_slam_amd.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_struct_and_the_call():
    h = _header()
    m = re.search(r"typedef struct srrg2_batch_slice_clouds \{(.*?)\} srrg2_batch_slice_clouds;", h, re.S)
    assert m, "srrg2_batch_slice_clouds is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body.replace(",", ";"))
    assert fields == [f for f, _ in abi.BatchSliceClouds._fields_]
    decl = re.search(r"int srrg2_align_batch_slices\(([^;]*)\);", h, re.S)
    assert decl, "srrg2_align_batch_slices is not declared"
    params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
    assert [p.split()[-1].lstrip("*") for p in params.split(",")] == ["h", "K", "nslices", "clouds", "mem", "guesses", "results"]
    assert "#define SRRG2_AMD_ABI_VERSION 4" in h


LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "srrg2_slam_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(srrg2_batch_slice_clouds), offsetof(srrg2_batch_slice_clouds, coords),
         offsetof(srrg2_batch_slice_clouds, coord_stride_bytes), offsetof(srrg2_batch_slice_clouds, normals),
         offsetof(srrg2_batch_slice_clouds, normal_stride_bytes), offsetof(srrg2_batch_slice_clouds, offsets));
  return 0;
}
"""


def test_ctypes_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.BatchSliceClouds
    want = [C_sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert got == want


def C_sizeof(t):
    import ctypes

    return ctypes.sizeof(t)


def _two_slice_case(kind, K, seed):
    if kind == abi.SE2_RIGHT:
        s0 = syn.scan_pair_2d(beams=400, t=(0.05, -0.02), theta_deg=2.0, seed=seed)
        s1 = syn.scan_pair_2d(beams=300, t=(0.05, -0.02), theta_deg=2.0, seed=seed + 1)
        cfgs = [cue_config(kind, abi.SLICE_P2P, 0.3), cue_config(kind, abi.SLICE_P2P, 0.25, abi.ROBUST_CAUCHY, 0.02)]
        fixed = [(s0["fixed"], None), (s1["fixed"], None)]
        movs = [s0["moving"], s1["moving"]]
        nrms = [None, None]
        S = syn.se2(0.1, 0.0, 0.05)
    else:
        d0 = syn.cloud_pair_3d(n=1500, seed=seed)
        d1 = syn.cloud_pair_3d(n=1000, seed=seed + 1)
        cfgs = [cue_config(kind, abi.SLICE_P2PLANE, 0.25), cue_config(kind, abi.SLICE_P2P, 0.3)]
        fixed = [(d0["fixed"], d0["fixed_normals"]), (d1["fixed"], None)]
        movs = [d0["moving"], d1["moving"]]
        nrms = [d0["moving_normals"], None]
        S = syn.se3((0.02, 0.0, -0.01), (0.0, 0.5, 0.0))
    rng = np.random.default_rng(seed)
    moving, normals = {}, {}
    for si in (0, 1):
        cs, ns = [], []
        for k in range(K):
            n = movs[si].shape[0]
            sel = np.arange(0) if (si == 1 and k == 1) else np.sort(rng.choice(n, int(rng.integers(n // 2, n + 1)), replace=False))
            cs.append(movs[si][sel])
            ns.append(None if nrms[si] is None else nrms[si][sel])
        moving[si] = cs
        normals[si] = None if nrms[si] is None else ns
    guesses = [syn.identity(2 if kind == abi.SE2_RIGHT else 3)] * K
    return cfgs, fixed, S, moving, normals, guesses


def _oracle_handle(oracle, kind, cfgs, fixed, S, prior=False):
    al = oracle.OracleAligner(kind)
    al.set_params(max_iterations=6, min_num_inliers=10)
    for si, c in enumerate(cfgs):
        al.add_slice(c)
        al.set_fixed(si, *fixed[si])
    al.set_sensor_in_robot(1, S)
    if prior:
        p = al.add_slice(prior_config(kind))
        al.set_prior_measurement(p, syn.identity(al.dim))
    return al


@pytest.mark.parametrize("kind", [abi.SE3_QUAT_RIGHT, abi.SE2_RIGHT])
def test_oracle_loop_equals_fresh_single_computes(oracle, kind):
    K = 4
    cfgs, fixed, S, moving, normals, guesses = _two_slice_case(kind, K, 321)
    al = _oracle_handle(oracle, kind, cfgs, fixed, S, prior=True)
    assert al._batch_slices_fn() is None  # (the oracle backend runs the defining loop)
    res = al.compute_batch_slices(moving, guesses, normals)
    assert len(res) == K
    for k in range(K):
        one = _oracle_handle(oracle, kind, cfgs, fixed, S, prior=True)
        for si in (0, 1):
            one.set_moving(si, moving[si][k], None if normals[si] is None else normals[si][k])
        one.set_moving_in_fixed(guesses[k])
        st = one.compute()
        r = res[k]
        assert r["status"] == st
        assert r["moving_in_fixed"].tobytes() == one.moving_in_fixed().tobytes()
        n, last = one.last_iteration_stats()
        assert r["num_iterations"] == n and r["last"] == last
        assert r["num_correspondences"] == one.num_correspondences()
        assert r["information"].tobytes() == one.information().tobytes()
    assert res[0]["status"] == abi.SUCCESS


def test_callers_refuse_mixed_candidates(oracle):
    kind = abi.SE3_QUAT_RIGHT
    cfgs, fixed, S, moving, normals, guesses = _two_slice_case(kind, 2, 400)
    al = _oracle_handle(oracle, kind, cfgs, fixed, S)
    det = ld.MultiLoopDetectorBruteForce(al, relocalize_min_inliers=10)
    hints = [ld.ClosureHint(1, {0: moving[0][0], 1: moving[1][0]}), ld.ClosureHint(2, moving[0][1])]
    with pytest.raises(ValueError):
        det.compute(0, {0: fixed[0][0], 1: fixed[1][0]}, {0: fixed[0][1]}, hints)
    hints = [ld.ClosureHint(1, {0: moving[0][0], 1: moving[1][0]}), ld.ClosureHint(2, {0: moving[0][1]})]
    with pytest.raises(ValueError):
        det.compute(0, {0: fixed[0][0], 1: fixed[1][0]}, {0: fixed[0][1]}, hints)


def test_detector_with_per_slice_dicts_is_the_loop(oracle):
    """the detector's per-slice path on the oracle: the closures of its own per-hint loop"""
    kind = abi.SE3_QUAT_RIGHT
    K = 3
    cfgs, fixed, S, moving, normals, guesses = _two_slice_case(kind, K, 500)
    al = _oracle_handle(oracle, kind, cfgs, fixed, S)
    det = ld.MultiLoopDetectorBruteForce(al, relocalize_min_inliers=50, relocalize_max_chi_inliers=1.0,
                                         relocalize_min_inliers_ratio=0.1)
    hints = [ld.ClosureHint(10 + k, {0: moving[0][k], 1: moving[1][k]}, {0: normals[0][k]}) for k in range(K)]
    closures = det.compute(0, {0: fixed[0][0], 1: fixed[1][0]}, {0: fixed[0][1]}, hints)
    ref = _oracle_handle(oracle, kind, cfgs, fixed, S)
    res = ref.compute_batch_slices(moving, [syn.identity(3)] * K, {0: normals[0], 1: None})
    got = {c["target"]: c["measurement"].tobytes() for c in closures}
    assert got and all(got[10 + k] == res[k]["moving_in_fixed"].tobytes() for k in range(K) if 10 + k in got)
