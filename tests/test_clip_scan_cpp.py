"""The C++ mirror of the scan clipper (SceneClipperScan in include/srrg2_slam_amd.hpp): one small translation unit compiled with
plain g++ against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg runs a small clip
through the mirror class and prints the bit patterns, which must be the numpy restatement's (tests/clip_scan_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

N, BEAMS = 40, 91

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
  std::vector<float> pts(2 * n), nrm(2 * n), inten(n);
  for (int i = 0; i < n; ++i) {
    // the sensor stands at (0.75, -0.125) in the map and looks along +y: pairs of points share a ray at two ranges
    const float rho = 1.0f + 0.5f * (float) (i % 2) + 0.125f * (float) (i / 10);
    pts[2 * i + 0] = 0.75f + 0.125f * (float) ((i / 2) % 5 - 2) * rho;
    pts[2 * i + 1] = -0.125f + rho;
    nrm[2 * i + 0] = 0.f, nrm[2 * i + 1] = -1.f;
    inten[i] = (float) i;
  }
  pts[2 * 7 + 1] = std::numeric_limits<float>::quiet_NaN();
  pts[2 * 12 + 1] = -2.f;  // behind the sensor
  Scene<2> full, clipped;
  full.set(pts.data(), 8, nrm.data(), 8, n);
  full.setFeatures(nullptr, 0, inten.data(), 4, n);
  SceneClipperScan cl;
  REQUIRE(cl.status() == SceneClipperScan::Error && cl.param.occlusion_margin < 0.f && cl.param.num_beams == 0);
  cl.param.angle_min = -0.25, cl.param.angle_increment = 0.5 / 90.0, cl.param.num_beams = 91;
  Isometry<2> S = Isometry<2>::Identity(), L = Isometry<2>::Identity();
  const float s[9] = {0, -1, 0.5f, 1, 0, 0, 0, 0, 1};
  std::memcpy(S.data(), s, sizeof(s));
  L.data()[2] = 0.25f, L.data()[5] = -0.125f;
  cl.setSensorInRobot(S);
  cl.setRobotInLocalMap(L);
  cl.setFullScene(&full);
  cl.setClippedSceneInRobot(&clipped);
  std::vector<float> c, m, it;
  std::vector<uint8_t> d;
  const char* tags[2][4] = {{"sector_points", "sector_normals", "sector_intensity", "sector_indices"},
                            {"occlusion_points", "occlusion_normals", "occlusion_intensity", "occlusion_indices"}};
  for (int mode = 0; mode < 2; ++mode) {
    cl.param.occlusion_margin = mode ? 0.f : -1.f;
    cl.compute();
    REQUIRE(cl.status() == SceneClipperScan::Successful && cl.last().num_valid == n - 1);
    REQUIRE(cl.last().num_kept == clipped.size() && cl.last().num_kept <= cl.last().num_in_view);
    REQUIRE(clipped.hasIntensity() && !clipped.hasDescriptors());
    clipped.get(c, m);
    clipped.getFeatures(d, it);
    dump(tags[mode][0], c);
    dump(tags[mode][1], m);
    dump(tags[mode][2], it);
    std::printf("%s", tags[mode][3]);
    for (int g : cl.globalIndices()) std::printf(" %d", g);
    std::printf("\n%s %d %d %d\n", mode ? "occlusion_counts" : "sector_counts", cl.last().num_valid, cl.last().num_in_view,
                cl.last().num_kept);
  }
  const int kept = clipped.size();
  bool thrown = false;
  cl.param.range_min = 0.f;  // refused: the clipped scene stays
  try { cl.compute(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && cl.status() == SceneClipperScan::Error && clipped.size() == kept);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "clip_scan.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "clip_scan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_clip_scan_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def _bits(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _scene():
    F = np.float32
    i = np.arange(N)
    rho = (F(1.0) + F(0.5) * (i % 2).astype(F) + F(0.125) * (i // 10).astype(F)).astype(F)
    x = (F(0.75) + F(0.125) * ((i // 2) % 5 - 2).astype(F) * rho).astype(F)
    pts = np.stack([x, (F(-0.125) + rho).astype(F)], 1).astype(F)
    pts[7, 1] = np.nan
    pts[12, 1] = -2.0
    nrm = np.tile(np.array([0, -1.0], F), (N, 1))
    return pts, nrm, i.astype(F)


def _restated():
    import clip_scan_restatement as cs

    pts, nrm, inten = _scene()
    S = np.array([[0, -1, 0.5], [1, 0, 0], [0, 0, 1]], np.float32)
    L = np.array([[1, 0, 0.25], [0, 1, -0.125], [0, 0, 1]], np.float32)
    return [cs.clip_scan(pts, L, -0.25, 0.5 / 90.0, BEAMS, sensor_in_robot=S, occlusion_margin=margin, normals=nrm, intensity=inten)
            for margin in (-1.0, 0.0)]


def test_the_case_is_not_vacuous():
    sector, occlusion = _restated()
    # the scanner sees part of the scene, and occlusion removes some of that
    assert 0 < occlusion["num_kept"] < sector["num_kept"] < N


@pytest.mark.gpu
def test_cpp_clip_scan_matches_the_restatement(product, tmp_path):
    import clip_scan_restatement as cs

    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    for tag, r in zip(("sector", "occlusion"), _restated()):
        assert cs.same_bits(_bits(lines[tag + "_points"]).reshape(-1, 2), r["points"])
        assert cs.same_bits(_bits(lines[tag + "_normals"]).reshape(-1, 2), r["normals"])
        assert cs.same_bits(_bits(lines[tag + "_intensity"]), r["intensity"])
        assert [int(w) for w in lines[tag + "_indices"].split()[1:]] == list(r["global_indices"])
        assert [int(w) for w in lines[tag + "_counts"].split()[1:]] == [r["num_valid"], r["num_in_view"], r["num_kept"]]
