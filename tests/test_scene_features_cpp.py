"""The C++ mirror of the scene features (Scene<DIM>::setFeatures / getFeatures, DescriptorDatabase::add / match on a scene):
one small translation unit compiled with plain g++ against include/ and linked with the built library.  Compiling and
linking need no GPU; running it does (-m gpu)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

SOURCE = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char**) {
  if (argc > 1) return 0;  // (link check only)
  const int n = 3000;
  std::vector<float> pts(3 * n), inten(n);
  std::vector<uint8_t> desc(32 * n);
  unsigned x = 12345u;
  auto rnd = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
  for (int i = 0; i < n; ++i) {
    for (int d = 0; d < 3; ++d) pts[3 * i + d] = (float) (rnd() % 2000) / 1000.f - 1.f;
    for (int k = 0; k < 32; ++k) desc[32 * i + k] = (uint8_t) rnd();
    inten[i] = (float) i;
  }
  pts[3 * 7] = NAN;  // an invalid point: keeps its index, is no matchable
  Scene<3> meas, scene, clipped;
  meas.set(pts.data(), 12, nullptr, 0, n);
  REQUIRE(!meas.hasDescriptors() && !meas.hasIntensity());
  meas.setFeatures(desc.data(), 32, inten.data(), 4, n);
  REQUIRE(meas.hasDescriptors() && meas.hasIntensity());
  // an empty scene adopts the measurement's fields; every Valid point is appended with its features
  MergerCorrespondenceHomo<3> merger;
  merger.setScene(&scene);
  merger.setMeasurement(&meas);
  merger.compute();
  REQUIRE(merger.last().num_added == n - 1 && scene.size() == n - 1);
  std::vector<uint8_t> d;
  std::vector<float> it;
  scene.getFeatures(d, it);
  REQUIRE((int) it.size() == n - 1 && d.size() == 32u * (n - 1));
  for (int k = 0; k < n - 1; ++k) {
    const int i = k < 7 ? k : k + 1;
    REQUIRE(it[k] == inten[i] && !std::memcmp(&d[32 * k], &desc[32 * i], 32));
  }
  SceneClipperBall<3> clipper;
  clipper.param_range = 0.8f;
  clipper.setFullScene(&scene);
  clipper.setClippedSceneInRobot(&clipped);
  clipper.compute();
  const std::vector<int> g = clipper.globalIndices();
  std::vector<uint8_t> cd;
  std::vector<float> ci;
  clipped.getFeatures(cd, ci);
  REQUIRE(g.size() > 100 && g.size() < (size_t) n - 1 && ci.size() == g.size());
  for (size_t k = 0; k < g.size(); ++k) REQUIRE(ci[k] == it[g[k]] && !std::memcmp(&cd[32 * k], &d[32 * g[k]], 32));
  // the database fed from the scene = fed from the host arrays with the finite-coordinate mask
  std::vector<uint8_t> valid(n, 1);
  valid[7] = 0;
  DescriptorDatabase dev, host;
  REQUIRE(dev.add(meas) == 0 && host.add(desc.data(), valid.data(), n) == 0);
  REQUIRE(dev.numDescriptors() == n - 1 && host.numDescriptors() == n - 1);
  auto a = dev.match(meas, 1, 25.f, 0, 10);
  auto b = host.match(desc.data(), valid.data(), n, 1, 25.f, 0, 10);
  REQUIRE(a.size() == 1 && b.size() == 1 && a[0].num_matches == b[0].num_matches);
  REQUIRE(a[0].correspondences.size() == (size_t) n - 1 && a[0].correspondences.size() == b[0].correspondences.size());
  REQUIRE(!std::memcmp(a[0].correspondences.data(), b[0].correspondences.data(), sizeof(srrg2_correspondence) * (n - 1)));
  // a scene without descriptors is refused
  Scene<3> bare;
  bare.set(pts.data(), 12, nullptr, 0, n);
  bool thrown = false;
  try { dev.add(bare); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && dev.size() == 1);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "scene_features.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "scene_features"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_mirror_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


@pytest.mark.gpu
def test_cpp_mirror_moves_features(product, tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
