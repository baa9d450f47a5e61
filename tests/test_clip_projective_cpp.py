"""The C++ mirror of the projective clipper (SceneClipperProjective in include/srrg2_slam_amd.hpp): one small translation unit
compiled with plain g++ against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg
runs a small clip through the mirror class and prints the bit patterns, which must be the numpy restatement's
(tests/clip_projective_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

N, ROWS, COLS = 40, 6, 8

SOURCE = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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
  const int n = 40;
  std::vector<float> pts(3 * n), nrm(3 * n), inten(n);
  for (int i = 0; i < n; ++i) {
    // robot frame: x forward (the camera's z), y left, z up; pairs of points share a ray at two depths
    pts[3 * i + 0] = 1.0f + 0.5f * (float) (i % 2) + 0.125f * (float) (i / 10);
    pts[3 * i + 1] = 0.0625f * (float) ((i / 2) % 5 - 2) * pts[3 * i + 0];
    pts[3 * i + 2] = 0.25f + 0.03125f * (float) (i / 10) * pts[3 * i + 0];
    nrm[3 * i + 0] = -1.f, nrm[3 * i + 1] = 0.f, nrm[3 * i + 2] = 0.f;
    inten[i] = (float) i;
  }
  pts[3 * 7 + 1] = std::numeric_limits<float>::quiet_NaN();
  pts[3 * 12 + 0] = -2.f;  // behind the camera
  Scene<3> full, clipped;
  full.set(pts.data(), 12, nrm.data(), 12, n);
  full.setFeatures(nullptr, 0, inten.data(), 4, n);
  SceneClipperProjective cl;
  REQUIRE(cl.status() == SceneClipperProjective::Error && cl.param.occlusion_margin < 0.f);
  const float K[9] = {8.f, 0.f, 3.5f, 0.f, 8.f, 2.5f, 0.f, 0.f, 1.f};
  cl.setCameraMatrix(K);
  cl.param.image_rows = 6, cl.param.image_cols = 8;
  Isometry<3> S = Isometry<3>::Identity(), L = Isometry<3>::Identity();
  const float s[12] = {0, 0, 1, 0.5f, -1, 0, 0, 0, 0, -1, 0, 0.25f};
  std::memcpy(S.data(), s, sizeof(s));
  L.data()[3] = 0.25f, L.data()[7] = -0.125f;
  cl.setSensorInRobot(S);
  cl.setRobotInLocalMap(L);
  cl.setFullScene(&full);
  cl.setClippedSceneInRobot(&clipped);
  std::vector<float> c, m, it;
  std::vector<uint8_t> d;
  const char* tags[2][4] = {{"frustum_points", "frustum_normals", "frustum_intensity", "frustum_indices"},
                            {"occlusion_points", "occlusion_normals", "occlusion_intensity", "occlusion_indices"}};
  for (int mode = 0; mode < 2; ++mode) {
    cl.param.occlusion_margin = mode ? 0.f : -1.f;
    cl.compute();
    REQUIRE(cl.status() == SceneClipperProjective::Successful && cl.last().num_valid == n - 1);
    REQUIRE(cl.last().num_kept == clipped.size() && cl.last().num_kept <= cl.last().num_in_view);
    REQUIRE(clipped.hasIntensity() && !clipped.hasDescriptors());
    clipped.get(c, m);
    clipped.getFeatures(d, it);
    dump(tags[mode][0], c);
    dump(tags[mode][1], m);
    dump(tags[mode][2], it);
    std::printf("%s", tags[mode][3]);
    for (int g : cl.globalIndices()) std::printf(" %d", g);
    std::printf("\n%s %d %d %d\n", mode ? "occlusion_counts" : "frustum_counts", cl.last().num_valid, cl.last().num_in_view,
                cl.last().num_kept);
  }
  const int kept = clipped.size();
  bool thrown = false;
  cl.param.depth_min = 0.f;  // refused: the clipped scene stays
  try { cl.compute(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && cl.status() == SceneClipperProjective::Error && clipped.size() == kept);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "clip_projective.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "clip_projective"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_clip_projective_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def _bits(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _scene():
    F = np.float32
    i = np.arange(N)
    x = (F(1.0) + F(0.5) * (i % 2).astype(F) + F(0.125) * (i // 10).astype(F)).astype(F)
    y = (F(0.0625) * ((i // 2) % 5 - 2).astype(F) * x).astype(F)
    z = (F(0.25) + F(0.03125) * (i // 10).astype(F) * x).astype(F)
    pts = np.stack([x, y, z], 1).astype(F)
    pts[7, 1] = np.nan
    pts[12, 0] = -2.0
    nrm = np.tile(np.array([-1.0, 0, 0], F), (N, 1))
    return pts, nrm, i.astype(F)


@pytest.mark.gpu
def test_cpp_clip_projective_matches_the_restatement(product, tmp_path):
    import clip_projective_restatement as cr

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    pts, nrm, inten = _scene()
    K = np.array([[8.0, 0, 3.5], [0, 8.0, 2.5], [0, 0, 1.0]], np.float32)
    S = np.array([[0, 0, 1, 0.5], [-1, 0, 0, 0], [0, -1, 0, 0.25]], np.float32)
    L = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.125], [0, 0, 1, 0]], np.float32)
    kept = []
    for tag, margin in (("frustum", -1.0), ("occlusion", 0.0)):
        r = cr.clip_projective(pts, L, K, ROWS, COLS, sensor_in_robot=S, occlusion_margin=margin, normals=nrm, intensity=inten)
        assert cr.same_bits(_bits(lines[tag + "_points"]).reshape(-1, 3), r["points"])
        assert cr.same_bits(_bits(lines[tag + "_normals"]).reshape(-1, 3), r["normals"])
        assert cr.same_bits(_bits(lines[tag + "_intensity"]), r["intensity"])
        assert [int(w) for w in lines[tag + "_indices"].split()[1:]] == list(r["global_indices"])
        assert [int(w) for w in lines[tag + "_counts"].split()[1:]] == [r["num_valid"], r["num_in_view"], r["num_kept"]]
        kept.append(r["num_kept"])
    assert 0 < kept[1] < kept[0] < N  # (not a vacuous case: the camera sees part of the scene, and occlusion removes some of that)
