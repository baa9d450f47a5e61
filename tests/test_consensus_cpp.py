"""The C++ side of the consensus pose on the CPU: the mirror (ConsensusVerifier in include/srrg2_slam_amd_loop_closure.hpp)
compiles as plain C++17 with every warning an error and the structs keep their sizes; and csrc/consensus_math.h -- the sampler and
the two minimal solvers the kernels run -- built with g++ into a small stand-alone program gives, hypothesis by hypothesis, the bit
patterns of tests/consensus_restatement.py.  Needs no GPU and no library."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIRROR = r"""
#include <cstdint>
#include <vector>
#include "srrg2_slam_amd_loop_closure.hpp"
using namespace srrg2_slam_amd;

static_assert(sizeof(srrg2_consensus_params) == 32 && sizeof(srrg2_consensus_result) == 96 && sizeof(srrg2_correspondence) == 12,
              "struct sizes");
static_assert(SRRG2_AMD_ABI_VERSION == 4, "adding a function does not bump the ABI");

template <int DIM>
long use(const float* fixed, int nf, const float* moving, const std::vector<int32_t>& offsets,
         const std::vector<CorrespondenceVector>& corr) {
  ConsensusVerifier<DIM> cv(0);
  cv.setNumHypotheses(512);
  cv.setInlierDistance(0.04f);
  cv.setMinSampleDistance(0.2f);
  cv.setMinInliers(20);
  cv.setSeed(7u);
  cv.setLengthCheck(true);
  cv.setFixed(fixed, nf, 16, SRRG2_MEM_HOST);
  cv.setMoving(moving, offsets, 16);
  cv.setCorrespondences(corr);
  cv.compute();
  long sum = cv.param.reserved[0];
  for (size_t k = 0; k < cv.results().size(); ++k) {
    const srrg2_consensus_result& r = cv.results()[k];
    const Isometry<DIM> X = cv.movingInFixed((int) k);
    const CorrespondenceVector in = cv.inliers((int) k);
    sum += r.status == SRRG2_CONSENSUS_FOUND ? (long) in.size() + (long) X.data()[0] : 0;
    sum += r.best_hypothesis + r.num_inliers + r.num_pairs + r.num_valid_pairs + r.num_degenerate + r.num_rejected + r.num_scored +
           r.cost_exponent + (long) r.cost + SRRG2_CONSENSUS_NO_HYPOTHESIS + SRRG2_CONSENSUS_TOO_FEW_INLIERS;
  }
  return sum;
}
template long use<2>(const float*, int, const float*, const std::vector<int32_t>&, const std::vector<CorrespondenceVector>&);
template long use<3>(const float*, int, const float*, const std::vector<int32_t>&, const std::vector<CorrespondenceVector>&);
"""

# reads: dim H seed N msd tau length_check, then N lines "valid fx fy fz mx my mz" (float32 bit patterns, hex);
# prints per hypothesis: status, the indices, the float64 pose as hex bit patterns
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "consensus_math.h"

static float f32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint64_t bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }

template <int S>
static void run(int H, uint32_t seed, int N, double msd, double tau, int lc, const std::vector<int>& valid,
                const std::vector<float>& f, const std::vector<float>& m) {
  for (int h = 0; h < H; ++h) {
    int idx[S] = {};
    double X[12] = {};
    int status = cm::HYP_DEGENERATE;
    const bool sampled = cm::sample<S>(seed, (uint32_t) h, N, idx);
    bool ok = sampled;
    for (int j = 0; j < S && ok; ++j) ok = valid[idx[j]] != 0;
    if (ok) {
      if (S == 3) status = cm::solve3(&m[3 * idx[0]], &m[3 * idx[1]], &m[3 * idx[S - 1]], &f[3 * idx[0]], &f[3 * idx[1]], &f[3 * idx[S - 1]],
                                      msd * msd, tau, lc, X);
      else status = cm::solve2(&m[3 * idx[0]], &m[3 * idx[1]], &f[3 * idx[0]], &f[3 * idx[1]], msd * msd, tau, lc, X);
    }
    std::printf("%d %d", status, sampled ? 1 : 0);
    for (int j = 0; j < S; ++j) std::printf(" %d", sampled ? idx[j] : -1);
    for (int i = 0; i < (S == 3 ? 12 : 9); ++i) std::printf(" %016" PRIx64, status == cm::HYP_SCORED ? bits(X[i]) : (uint64_t) 0);
    std::printf("\n");
  }
}

int main() {
  int dim, H, N, lc;
  uint32_t seed, msd_bits, tau_bits;
  if (std::scanf("%d %d %" SCNu32 " %d %" SCNx32 " %" SCNx32 " %d", &dim, &H, &seed, &N, &msd_bits, &tau_bits, &lc) != 7) return 2;
  std::vector<int> valid((size_t) N + 1);
  std::vector<float> f(3 * (size_t) N + 3), m(3 * (size_t) N + 3);
  for (int i = 0; i < N; ++i) {
    uint32_t u[6];
    if (std::scanf("%d %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &valid[i], &u[0], &u[1], &u[2], &u[3], &u[4],
                   &u[5]) != 7)
      return 3;
    for (int c = 0; c < 3; ++c) f[3 * i + c] = f32(u[c]), m[3 * i + c] = f32(u[3 + c]);
  }
  const double msd = (double) f32(msd_bits), tau = (double) f32(tau_bits);
  if (dim == 3) run<3>(H, seed, N, msd, tau, lc, valid, f, m);
  else run<2>(H, seed, N, msd, tau, lc, valid, f, m);
  return 0;
}
"""


def test_cpp_consensus_mirror_compiles(tmp_path):
    src = tmp_path / "consensus.cpp"
    src.write_text(MIRROR)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr


def test_ctypes_mirrors_keep_the_sizes():
    from srrg2_slam_interfaces_amd import _abi as abi

    assert C.sizeof(abi.ConsensusParams) == 32 and C.sizeof(abi.ConsensusResult) == 96
    assert (abi.CONSENSUS_FOUND, abi.CONSENSUS_NO_HYPOTHESIS, abi.CONSENSUS_TOO_FEW_INLIERS) == (0, 1, 2)
    assert abi.ABI_VERSION == 4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("consensus_math")
    src, exe = d / "main.cpp", d / "main"
    src.write_text(PROGRAM)
    out = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                          os.path.join(ROOT, "srrg2_slam_interfaces_amd", "csrc"), str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout + out.stderr
    return str(exe)


def _hex32(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


@pytest.mark.parametrize("name", sorted(cc.cpp_cases()))
def test_consensus_math_gives_the_restatements_bits(name, program):
    c = cc.cpp_cases()[name]
    dim, p = c["dim"], dict(cr.DEFAULTS, **c["params"])
    pf, pm, valid = cr.gather_pairs(dim, c["fixed"], c["movings"][0], c["corrs"][0])
    N = len(valid)
    lines = ["%d %d %d %d %s %s %d" % (dim, p["num_hypotheses"], p["seed"], N, _hex32(p["min_sample_distance"]),
                                       _hex32(p["inlier_distance"]), p["length_check"])]
    for i in range(N):
        f = list(pf[i]) + [0.0] * (3 - dim)
        m = list(pm[i]) + [0.0] * (3 - dim)
        lines.append(" ".join(["%d" % valid[i]] + [_hex32(v) for v in f + m]))
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    r = cr.consensus_one(dim, c["fixed"], c["movings"][0], c["corrs"][0], **c["params"])
    rows = out.stdout.strip().split("\n")
    assert len(rows) == p["num_hypotheses"]
    s, tsize = (3 if dim == 3 else 2), (12 if dim == 3 else 9)
    idx, ok = cr.sample(p["seed"], p["num_hypotheses"], N, s)
    seen = set()
    for h, row in enumerate(rows):
        w = row.split()
        status, sampled = int(w[0]), int(w[1])
        assert status == r["hyp_status"][h], (h, row)
        assert sampled == int(ok[h])
        if sampled:
            assert [int(v) for v in w[2:2 + s]] == list(idx[h])
        if status == cr.HYP_SCORED:
            got = np.array([int(v, 16) for v in w[2 + s:2 + s + tsize]], np.uint64)
            assert np.array_equal(got, r["hyp_pose64"][h].view(np.uint64)), (h, row)
        seen.add(status)
    assert cr.HYP_SCORED in seen and (name != "degenerate" or seen == {cr.HYP_SCORED, cr.HYP_DEGENERATE, cr.HYP_REJECTED})
