"""The C++ mirror of correlative scan matching (GridMap::buildLikelihood, likelihood, matchScans in include/srrg2_slam_amd.hpp): one
small translation unit compiled with plain g++ against include/ and linked with the built library.  Compiling, linking, the struct
sizes, the default table and the refusals that need no device run without a GPU; the GPU leg draws a map, builds the field, matches
a batch of scans and prints field, results and volume, which must be those of the restatement (tests/scan_match_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

SOURCE = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_gridmap_match_params) == 24 && sizeof(srrg2_gridmap_match_result) == 60, "struct sizes");
  const std::vector<uint8_t> lut = GridMap::defaultLikelihoodLut(4);
  REQUIRE(lut.size() == 17 && lut[0] == 255 && lut[1] == 240 && lut[16] == 15);
  bool thrown = false;
  try { GridMap::defaultLikelihoodLut(17); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  // refused without a handle: the parameters are checked first
  REQUIRE(srrg2_gridmap_build_likelihood(nullptr, 1, 50, 17, lut.data()) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "radius") != nullptr);
  REQUIRE(srrg2_gridmap_build_likelihood(nullptr, 1, 50, 4, lut.data()) == SRRG2_E_INVALID);  // only the handle is missing now
  REQUIRE(std::strstr(srrg2_amd_last_error(), "null handle") != nullptr);
  srrg2_gridmap_scan_params s;
  srrg2_gridmap_default_scan_params(&s);
  s.angle_increment = 0.01, s.num_beams = 4;
  srrg2_gridmap_match_params w;
  std::memset(&w, 0, sizeof(w));
  w.half_window_x = -1;
  float r4[4] = {1, 1, 1, 1}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  srrg2_gridmap_match_result res;
  std::memset(&res, 0x5a, sizeof(res));
  REQUIRE(srrg2_gridmap_match_scans(nullptr, r4, 1, eye, SRRG2_MEM_HOST, &s, &w, &res, nullptr, SRRG2_MEM_HOST) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "half window") != nullptr && res.dx == 0x5a5a5a5a);
  w.half_window_x = 40000, w.half_window_y = 40000;
  REQUIRE(srrg2_gridmap_match_scans(nullptr, r4, 1, eye, SRRG2_MEM_HOST, &s, &w, &res, nullptr, SRRG2_MEM_HOST) == SRRG2_E_UNSUPPORTED);
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  // the case file: rows, cols, K, num_beams, M, wx, wy, ht; resolution, origin, range_min, range_max; bearings, theta_step;
  // poses; ranges; then the M scans to match: guesses; ranges
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[8];
  float fl[5];
  double dbl[3];
  REQUIRE(std::fread(shape, 4, 8, f) == 8 && std::fread(fl, 4, 5, f) == 5 && std::fread(dbl, 8, 3, f) == 3);
  const int K = shape[2], nb = shape[3], M = shape[4];
  std::vector<float> poses((size_t) K * 9), ranges((size_t) K * nb), guesses((size_t) M * 9), scans((size_t) M * nb);
  REQUIRE(std::fread(poses.data(), 4, poses.size(), f) == poses.size() && std::fread(ranges.data(), 4, ranges.size(), f) == ranges.size());
  REQUIRE(std::fread(guesses.data(), 4, guesses.size(), f) == guesses.size() && std::fread(scans.data(), 4, scans.size(), f) == scans.size());
  std::fclose(f);
  GridMap map;
  map.params.rows = shape[0], map.params.cols = shape[1], map.params.resolution = fl[0];
  map.params.origin[0] = fl[1], map.params.origin[1] = fl[2];
  map.scan.angle_min = dbl[0], map.scan.angle_increment = dbl[1], map.scan.num_beams = nb;
  map.scan.range_min = fl[3], map.scan.range_max = fl[4];
  map.reset();
  map.integrate(ranges.data(), K, poses.data());
  w.half_window_x = shape[5], w.half_window_y = shape[6], w.half_steps_theta = shape[7], w.theta_step = dbl[2];
  thrown = false;  // no field yet
  try { map.matchScans(scans.data(), M, guesses.data(), w); } catch (const std::exception& e) { thrown = std::strstr(e.what(), "stale") != nullptr; }
  REQUIRE(thrown);
  map.buildLikelihood(1, 50, 3);
  std::printf("field");
  for (uint8_t v : map.likelihood()) std::printf(" %d", (int) v);
  std::printf("\n");
  std::vector<int32_t> volume;
  const std::vector<srrg2_gridmap_match_result> out = map.matchScans(scans.data(), M, guesses.data(), w, SRRG2_MEM_HOST, &volume);
  REQUIRE((int) out.size() == M);
  for (const srrg2_gridmap_match_result& r : out) {
    std::printf("result %d %d %d %d %d %d", r.dx, r.dy, r.jtheta, r.score, r.score_at_guess, r.num_scored_beams);
    for (float v : r.robot_in_world) {
      uint32_t u;
      std::memcpy(&u, &v, 4);
      std::printf(" %08x", u);
    }
    std::printf("\n");
  }
  std::printf("volume");
  for (int32_t v : volume) std::printf(" %d", v);
  std::printf("\n");
  REQUIRE(map.matchScans(scans.data(), M, guesses.data(), w).size() == out.size());  // (without the volume)
  map.remove(ranges.data(), 1, poses.data());
  thrown = false;  // the planes changed: stale again
  try { map.likelihood(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "scan_match.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "scan_match"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_scan_match_compile_and_link(tmp_path):
    """... and the struct sizes, the default table and the refusals without a handle hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_scan_match_bit_for_bit(product, tmp_path):
    import gridmap_cases as gc
    import gridmap_restatement as gr
    import scan_match_restatement as sm

    g, sc, poses, ranges = gc.shape_case(((64, 64), 6, 361), seed=31)
    ranges = gc.mixed(ranges, seed=32)
    room = gc.room_of(g)
    truth = gc.trajectory(room, 3, 33)
    scans = gc.mixed(gc.room_scans(room, truth, sc, sigma=0.004, seed=34), 35)
    guesses = np.stack([p @ gc.pose(0.11, -0.07, 0.06) for p in truth]).astype(np.float32)
    wx, wy, ht, step = 4, 3, 2, 0.03
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([g["rows"], g["cols"], 6, 361, 3, wx, wy, ht], np.int32).tobytes())
        f.write(np.array([g["res"], g["ox"], g["oy"], sc["range_min"], sc["range_max"]], np.float32).tobytes())
        f.write(np.array([sc["angle_min"], sc["angle_increment"], step], np.float64).tobytes())
        f.write(poses.astype(np.float32).tobytes() + ranges.astype(np.float32).tobytes())
        f.write(guesses.tobytes() + scans.astype(np.float32).tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.strip()]
    h, m = gr.new_planes(g)
    gr.integrate(h, m, ranges, poses, sc, g)
    field = sm.likelihood(h, m, 1, 50, 3, sm.default_lut(3))
    want = sm.match(field, scans, guesses, sc, g, wx, wy, ht, step)
    assert want["score"].min() > 0 and field.any()
    got_field = [l for l in lines if l[0] == "field"][0][1:]
    assert np.array_equal(np.array(got_field, np.int64).reshape(field.shape), field)
    results = [l[1:] for l in lines if l[0] == "result"]
    assert len(results) == 3
    for k, r in enumerate(results):
        assert [int(v) for v in r[:6]] == [int(want[n][k]) for n in ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")]
        pose = np.array([int(v, 16) for v in r[6:]], np.uint32).view(np.float32)
        assert pose.tobytes() == want["robot_in_world"][k].tobytes()
    got_volume = [l for l in lines if l[0] == "volume"][0][1:]
    assert np.array_equal(np.array(got_volume, np.int64).reshape(want["scores"].shape), want["scores"])
