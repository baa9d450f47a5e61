"""The C++ mirror of pruned scan matching (GridMap::buildBounds, bounds, matchScansPruned, localize in include/srrg2_slam_amd.hpp):
one small translation unit compiled with plain g++ against include/ and linked with the built library.  Compiling, linking, the
struct sizes, the default parameters and the refusals that need no device run without a GPU; the GPU leg draws the recovery map,
builds field and planes, matches and localises, and prints planes, results and statistics, which must be those of the restatement
(tests/scan_match_pruned_restatement.py)."""
import math
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

static void print(const char* tag, const std::vector<srrg2_gridmap_match_result>& out, const std::vector<srrg2_gridmap_prune_stats>& stats) {
  for (size_t k = 0; k < out.size(); ++k) {
    const srrg2_gridmap_match_result& r = out[k];
    std::printf("%s %d %d %d %d %d %d", tag, r.dx, r.dy, r.jtheta, r.score, r.score_at_guess, r.num_scored_beams);
    for (float v : r.robot_in_world) {
      uint32_t u;
      std::memcpy(&u, &v, 4);
      std::printf(" %08x", u);
    }
    const srrg2_gridmap_prune_stats& s = stats[k];
    std::printf(" %d %d %d %d", s.num_candidates, s.floor_score, s.seed_block, s.fell_back);
    for (int l = 0; l < 7; ++l) std::printf(" %d %d", s.num_evaluated[l], s.num_survivors[l]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_gridmap_prune_params) == 8 && sizeof(srrg2_gridmap_prune_stats) == 72, "struct sizes");
  srrg2_gridmap_prune_params pp;
  std::memset(&pp, 0x5a, sizeof(pp));
  srrg2_gridmap_default_prune_params(&pp);
  REQUIRE(pp.num_levels == 4 && pp.max_list_entries == 0);
  // refused without a handle: the parameters are checked first
  REQUIRE(srrg2_gridmap_build_bounds(nullptr, 7) == SRRG2_E_INVALID && std::strstr(srrg2_amd_last_error(), "num_levels") != nullptr);
  REQUIRE(srrg2_gridmap_build_bounds(nullptr, 6) == SRRG2_E_INVALID && std::strstr(srrg2_amd_last_error(), "null handle") != nullptr);
  srrg2_gridmap_scan_params s;
  srrg2_gridmap_default_scan_params(&s);
  s.angle_increment = 0.01, s.num_beams = 4;
  srrg2_gridmap_match_params w;
  std::memset(&w, 0, sizeof(w));
  float r4[4] = {1, 1, 1, 1}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  srrg2_gridmap_match_result res;
  srrg2_gridmap_prune_stats st;
  std::memset(&res, 0x5a, sizeof(res));
  std::memset(&st, 0x5a, sizeof(st));
  pp.num_levels = 0;
  REQUIRE(srrg2_gridmap_match_scans_pruned(nullptr, r4, 1, eye, SRRG2_MEM_HOST, &s, &w, &pp, &res, &st) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "num_levels") != nullptr && res.dx == 0x5a5a5a5a && st.fell_back == 0x5a5a5a5a);
  pp.num_levels = 2, pp.max_list_entries = -1;
  REQUIRE(srrg2_gridmap_match_scans_pruned(nullptr, r4, 1, eye, SRRG2_MEM_HOST, &s, &w, &pp, &res, &st) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "max_list_entries") != nullptr);
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  // the case file: rows, cols, K, num_beams, M, wx, wy, ht; resolution, origin, range_min, range_max; bearings, theta_step, the
  // step of localize; poses; ranges; then the M scans to match: guesses; ranges
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[8];
  float fl[5];
  double dbl[4];
  REQUIRE(std::fread(shape, 4, 8, f) == 8 && std::fread(fl, 4, 5, f) == 5 && std::fread(dbl, 8, 4, f) == 4);
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
  map.buildLikelihood(1, 50, 4);
  bool thrown = false;  // a field, no planes yet
  try { map.matchScansPruned(scans.data(), M, guesses.data(), w, 2); } catch (const std::exception& e) { thrown = std::strstr(e.what(), "stale") != nullptr; }
  REQUIRE(thrown);
  map.buildBounds(3);
  std::printf("plane");
  for (uint8_t v : map.bounds(3)) std::printf(" %d", (int) v);
  std::printf("\n");
  std::vector<srrg2_gridmap_prune_stats> stats;
  const std::vector<srrg2_gridmap_match_result> out = map.matchScansPruned(scans.data(), M, guesses.data(), w, 0, 0, SRRG2_MEM_HOST, &stats);
  REQUIRE((int) out.size() == M && (int) stats.size() == M);
  print("pruned", out, stats);
  const std::vector<srrg2_gridmap_match_result> full = map.matchScans(scans.data(), M, guesses.data(), w);
  for (int k = 0; k < M; ++k) REQUIRE(std::memcmp(&full[k], &out[k], sizeof(full[k])) == 0);
  print("fallback", map.matchScansPruned(scans.data(), M, guesses.data(), w, 2, 4, SRRG2_MEM_HOST, &stats), stats);
  print("localize", map.localize(scans.data(), M, dbl[3], 3, &stats), stats);
  map.buildLikelihood(1, 50, 4);
  print("rebuilt", map.localize(scans.data(), M, dbl[3], 0, &stats), stats);  // (localize builds four levels itself)
  REQUIRE(map.bounds(4).size() == (size_t) (shape[0] + 15) * (size_t) (shape[1] + 15));
  map.remove(ranges.data(), 1, poses.data());
  thrown = false;  // the planes changed: stale again
  try { map.bounds(1); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "scan_match_pruned.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "scan_match_pruned"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_scan_match_pruned_compile_and_link(tmp_path):
    """... and the struct sizes, the default parameters and the refusals without a handle hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_scan_match_pruned_bit_for_bit(product, tmp_path):
    import scan_match_cases as smc
    import scan_match_pruned_cases as pc
    import scan_match_pruned_restatement as sp

    rm = smc.recovery_map()
    g, sc, field = rm["g"], rm["sc"], rm["field"]
    truth, scans, guesses = pc.recovery_batch()
    scans, guesses = scans[:3], guesses[:3]
    wx, wy, ht, step, lstep = 9, 7, 4, math.radians(1.0), math.radians(6.0)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([g["rows"], g["cols"], len(rm["poses"]), 361, 3, wx, wy, ht], np.int32).tobytes())
        f.write(np.array([g["res"], g["ox"], g["oy"], sc["range_min"], sc["range_max"]], np.float32).tobytes())
        f.write(np.array([sc["angle_min"], sc["angle_increment"], step, lstep], np.float64).tobytes())
        f.write(rm["poses"].astype(np.float32).tobytes() + rm["ranges"].astype(np.float32).tobytes())
        f.write(guesses.tobytes() + scans.astype(np.float32).tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.strip()]
    planes = pc.recovery_planes()
    got_plane = [l for l in lines if l[0] == "plane"][0][1:]
    assert np.array_equal(np.array(got_plane, np.int64).reshape(planes[3].shape), planes[3])
    centre = np.tile(pc.centre_pose(g), (3, 1, 1))
    lw = pc.localize_window(g, lstep)
    wants = {"pruned": sp.match(field, scans, guesses, sc, g, wx, wy, ht, step, 3, planes=planes),
             "fallback": sp.match(field, scans, guesses, sc, g, wx, wy, ht, step, 2, 4, planes=planes),
             "localize": sp.match(field, scans, centre, sc, g, *lw, lstep, 3, planes=planes),
             "rebuilt": sp.match(field, scans, centre, sc, g, *lw, lstep, 4, planes=planes)}
    assert any(s["fell_back"] for s in wants["fallback"]["stats"]) and wants["localize"]["score"].min() > 0
    for tag, want in wants.items():
        rows = [l[1:] for l in lines if l[0] == tag]
        assert len(rows) == 3, tag
        for k, r in enumerate(rows):
            assert [int(v) for v in r[:6]] == [int(want[n][k]) for n in pc.MEMBERS], (tag, k)
            pose = np.array([int(v, 16) for v in r[6:15]], np.uint32).view(np.float32)
            assert pose.tobytes() == want["robot_in_world"][k].tobytes(), (tag, k)
            st = want["stats"][k]
            flat = [st["num_candidates"], st["floor_score"], st["seed_block"], st["fell_back"]]
            for l in range(7):
                flat += [st["num_evaluated"][l], st["num_survivors"][l]]
            assert [int(v) for v in r[15:]] == flat, (tag, k)
