"""The C++ mirror of the measurement adaptors (DepthImageAdaptor / LaserScanAdaptor in include/srrg2_slam_amd.hpp): one small
translation unit compiled with plain g++ against include/ and linked with the built library.  Compiling and linking need no
GPU; the GPU leg runs the mirror classes on a small image and a small scan and prints the bit patterns, which must be the
numpy restatement's (tests/adaptor_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

ROWS, COLS, BEAMS = 6, 8, 9

SOURCE = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static void dump(const char* tag, const std::vector<float>& v) {
  std::printf("%s", tag);
  for (float f : v) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    std::printf(" %08x", u);
  }
  std::printf("\n");
}

int main(int argc, char**) {
  if (argc > 1) return 0;  // (link check only)
  const int rows = 6, cols = 8, beams = 9;
  std::vector<uint16_t> depth(rows * cols);
  std::vector<uint8_t> inten(rows * cols);
  for (int i = 0; i < rows * cols; ++i) {
    depth[i] = (uint16_t) (1000 + 37 * (i % cols) + 11 * (i / cols));
    inten[i] = (uint8_t) (3 * i);
  }
  depth[2 * cols + 3] = 0;  // no reading
  Scene<3> meas;
  DepthImageAdaptor ad;
  REQUIRE(ad.status() == DepthImageAdaptor::Initializing);
  const float K[9] = {10.f, 0.f, 3.5f, 0.f, 10.f, 2.5f, 0.f, 0.f, 1.f};
  std::memcpy(ad.param.camera_matrix, K, sizeof(K));
  ad.param.rows = rows, ad.param.cols = cols;
  ad.param.drop_points_without_normal = 0;
  ad.setMeas(&meas);
  ad.setRawData(depth.data(), SRRG2_IMAGE_U16, cols * 2, inten.data(), SRRG2_IMAGE_U8, cols);
  REQUIRE(ad.status() == DepthImageAdaptor::Error);
  ad.compute();
  REQUIRE(ad.status() == DepthImageAdaptor::Ready && ad.last().num_raw == rows * cols && ad.last().scene_size == rows * cols);
  REQUIRE(ad.last().num_in_range == rows * cols - 1 && meas.hasIntensity() && !meas.hasDescriptors());
  std::vector<float> c, n, it;
  std::vector<uint8_t> d;
  meas.get(c, n);
  meas.getFeatures(d, it);
  dump("depth_points", c);
  dump("depth_normals", n);
  dump("depth_intensity", it);
  ad.param.compact = 1;
  ad.compute(false);  // no counts asked for
  REQUIRE(ad.status() == DepthImageAdaptor::Ready && meas.size() == rows * cols - 1);
  bool thrown = false;
  ad.param.normal_row_gap = 0;  // exactly one gap 0: refused, the scene stays
  try { ad.compute(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && ad.status() == DepthImageAdaptor::Error && meas.size() == rows * cols - 1);
  ad.reset();
  REQUIRE(ad.status() == DepthImageAdaptor::Initializing);

  std::vector<float> ranges(beams);
  for (int k = 0; k < beams; ++k) ranges[k] = 2.f + 0.01f * (float) k;
  ranges[6] = 0.f;  // below range_min
  Scene<2> scan;
  LaserScanAdaptor sa;
  sa.param.angle_min = -0.2, sa.param.angle_increment = 0.05;
  sa.param.normal_max_distance_squared = 1.f;
  sa.setMeas(&scan);
  sa.setRawData(ranges.data(), beams);
  sa.compute();
  REQUIRE(sa.status() == LaserScanAdaptor::Ready && sa.last().num_in_range == beams - 1);
  scan.get(c, n);
  dump("scan_points", c);
  dump("scan_normals", n);
  std::printf("scan_valid %d\n", sa.last().num_valid);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "adaptors.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "adaptors"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_adaptors_compile_and_link(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def _bits(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


@pytest.mark.gpu
def test_cpp_adaptors_match_the_restatement(product, tmp_path):
    import adaptor_restatement as ar

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    i = np.arange(ROWS * COLS)
    depth = (1000 + 37 * (i % COLS) + 11 * (i // COLS)).astype(np.uint16).reshape(ROWS, COLS)
    depth[2, 3] = 0
    K = np.array([[10.0, 0, 3.5], [0, 10.0, 2.5], [0, 0, 1.0]], np.float32)
    r = ar.adapt_depth_image(depth, K, drop_points_without_normal=False, intensity=(3 * i).astype(np.uint8).reshape(ROWS, COLS))
    assert ar.same_bits(_bits(lines["depth_points"]).reshape(-1, 3), r["points"])
    assert ar.same_bits(_bits(lines["depth_normals"]).reshape(-1, 3), r["normals"])
    assert ar.same_bits(_bits(lines["depth_intensity"]), r["intensity"])
    assert r["has_normal"].sum() >= 5  # (not a vacuous case)
    ranges = (np.float32(2.0) + np.float32(0.01) * np.arange(BEAMS, dtype=np.float32)).astype(np.float32)
    ranges[6] = 0.0
    s = ar.adapt_laser_scan(ranges, -0.2, 0.05, max_distance_squared=1.0)
    assert ar.same_bits(_bits(lines["scan_points"]).reshape(-1, 2), s["points"])
    assert ar.same_bits(_bits(lines["scan_normals"]).reshape(-1, 2), s["normals"])
    assert int(lines["scan_valid"].split()[1]) == s["num_valid"] and s["num_valid"] >= 3
