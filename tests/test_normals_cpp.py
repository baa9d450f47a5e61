"""The C++ mirror of srrg2_scene_estimate_normals (Scene::estimateNormals in include/srrg2_slam_amd.hpp): one small translation
unit compiled with plain g++ against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg
estimates the normals of a lattice plane through the mirror and prints bit patterns and counts, which must be the numpy
restatement's (tests/normals_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")
M, SPACING, RADIUS = 9, 0.125, 0.26

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
  const int m = 9;
  std::vector<float> pts;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      pts.push_back(0.125f * (float) i);
      pts.push_back(0.125f * (float) j);
      pts.push_back(0.f);
    }
  pts.push_back(40.f), pts.push_back(0.f), pts.push_back(0.f);  // a lonely point: too few neighbours
  const int n = m * m + 1;
  Scene<3> scene;
  scene.set(pts.data(), 12, nullptr, 0, n);
  srrg2_normals_params p;
  srrg2_normals_default_params(&p, 3);
  REQUIRE(p.min_neighbours == 5 && p.drop_points_without_normal == 1);
  p.radius = 0.26f;
  p.viewpoint[0] = 0.5f, p.viewpoint[1] = 0.5f, p.viewpoint[2] = -2.f;
  std::vector<float> curv, c, nrm;
  const srrg2_normals_result r = scene.estimateNormals(p, &curv);
  REQUIRE(r.num_points == n && r.scene_size == scene.size() && (int) curv.size() == n);
  scene.get(c, nrm);
  dump("points", c);
  dump("normals", nrm);
  dump("curvature", curv);
  std::printf("counts %d %d %d %d %d %d %d\n", r.num_points, r.num_finite, r.num_with_normal, r.num_too_few, r.num_degenerate,
              r.num_too_curved, r.scene_size);
  bool thrown = false;
  p.radius = 0.f;  // refused: the scene stays
  try { scene.estimateNormals(p); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && scene.size() == r.scene_size);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "normals.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "normals"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_normals_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def _bits(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _restated():
    import normals_restatement as nr

    g = np.arange(M, dtype=np.float32) * np.float32(SPACING)
    x, y = np.meshgrid(g, g, indexing="ij")
    pts = np.concatenate([np.stack([x.ravel(), y.ravel(), np.zeros(M * M, np.float32)], 1), [[40.0, 0, 0]]]).astype(np.float32)
    return nr.estimate_normals(pts, RADIUS, viewpoint=(0.5, 0.5, -2.0), drop=True)


def test_the_case_is_not_vacuous():
    r = _restated()
    assert r["result"]["num_with_normal"] == M * M and r["result"]["num_too_few"] == 1
    assert np.array_equal(r["normals_out"], np.tile(np.array([0, 0, -1], np.float32), (M * M, 1)))


@pytest.mark.gpu
def test_cpp_normals_match_the_restatement(product, tmp_path):
    import normals_restatement as nr

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    r = _restated()
    assert nr.same_bits(_bits(lines["points"]).reshape(-1, 3), r["points_out"])
    assert nr.same_bits(_bits(lines["normals"]).reshape(-1, 3), r["normals_out"])
    assert nr.same_bits(_bits(lines["curvature"]), r["curvature"])
    res = r["result"]
    assert [int(w) for w in lines["counts"].split()[1:]] == [res[k] for k in (
        "num_points", "num_finite", "num_with_normal", "num_too_few", "num_degenerate", "num_too_curved", "scene_size")]
