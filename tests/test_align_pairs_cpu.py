"""Pair batches without a GPU: the Python mirror's defining loop on the oracle backend, and the C declaration."""
import os
import re
import subprocess

import numpy as np

from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srrg2_slam_amd.h")


def test_oracle_pairs_loop_equals_single_computes(oracle):
    """MultiAligner.compute_batch_pairs on a backend without srrg2_align_pairs runs set_fixed / set_moving /
    set_moving_in_fixed / compute() per pair: its records equal per-pair oracle compute() calls on fresh handles"""
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05)
    pairs = syn.batch_3d(K=3, n=1_500, seed=6100, shared_fixed_group=1)
    guesses = [syn.identity(3)] * 3
    al = oracle.OracleAligner(kind)
    al.add_slice(cfg)
    res = al.compute_batch_pairs([p["fixed"] for p in pairs], [p["moving"] for p in pairs], guesses,
                                 [p["fixed_normals"] for p in pairs], [p["moving_normals"] for p in pairs])
    assert len(res) == 3
    for k, p in enumerate(pairs):
        one = oracle.OracleAligner(kind)
        one.add_slice(cfg)
        one.set_fixed(0, p["fixed"], p["fixed_normals"])
        one.set_moving(0, p["moving"], p["moving_normals"])
        one.set_moving_in_fixed(guesses[k])
        st = one.compute()
        stats = one.iteration_stats()
        r = res[k]
        assert r["status"] == st
        assert r["moving_in_fixed"].tobytes() == one.moving_in_fixed().tobytes()
        assert r["num_iterations"] == len(stats) and r["last"] == stats[-1]
        assert r["num_correspondences"] == one.num_correspondences()
        assert r["information"].tobytes() == one.information().tobytes()
    # an SE(2) pair without normals goes through the same loop
    d = syn.scan_pair_2d(beams=360, seed=6200)
    al2 = oracle.OracleAligner(abi.SE2_RIGHT)
    al2.add_slice(cue_config(abi.SE2_RIGHT, abi.SLICE_P2P, 0.3))
    r2 = al2.compute_batch_pairs([d["fixed"]], [d["moving"]], [syn.identity(2)])
    assert r2[0]["moving_in_fixed"].shape == (3, 3)
    assert r2[0]["moving_in_fixed"].tobytes() == al2.moving_in_fixed().tobytes()


def test_align_pairs_is_declared_and_the_header_compiles(tmp_path):
    text = open(HEADER).read()
    assert re.search(r"int srrg2_align_pairs\(srrg2_aligner_h h, int K,", text)
    assert re.search(r"#define SRRG2_AMD_ABI_VERSION 4\b", text)
    c_src = tmp_path / "pairs.c"
    c_src.write_text('#include "srrg2_slam_amd.h"\nint (*p)(srrg2_aligner_h, int, const float*, int, const float*, int, '
                     'const int32_t*, const float*, int, const float*, int, const int32_t*, int, const float*, '
                     'srrg2_batch_result*) = srrg2_align_pairs;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(c_src)])
    cpp_src = tmp_path / "pairs.cpp"
    cpp_src.write_text('#include "srrg2_slam_amd.hpp"\n'
                       'using P = decltype(&srrg2_slam_amd::MultiAligner_<SRRG2_SE3_QUAT_RIGHT>::computeBatchPairs);\n'
                       'int main() { P p = &srrg2_slam_amd::MultiAligner_<SRRG2_SE3_QUAT_RIGHT>::computeBatchPairs; '
                       'return p ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(cpp_src)])


def test_the_library_exports_align_pairs():
    """the built library exports the entry point (a symbol check: no device needed)"""
    lib = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib", "libsrrg2_slam_amd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT srrg2_align_pairs$", out, re.M)
    assert np.dtype(abi.BatchResult).itemsize > 0
