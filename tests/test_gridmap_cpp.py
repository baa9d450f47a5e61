"""The C++ mirror of the occupancy grid (GridMap in include/srrg2_slam_amd.hpp): one small translation unit compiled with plain g++
against include/ and linked with the built library.  Compiling, linking, the defaults, the struct sizes and the refusals that need
no device run without a GPU; the GPU leg integrates a batch of scans, takes half of it out again and prints the planes, the
counters, the image and the exported scene, which must be those of the restatement (tests/gridmap_restatement.py)."""
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

static void dump_result(const char* tag, const srrg2_gridmap_result& r) {
  std::printf("%s %lld %lld %lld %lld %lld %lld\n", tag, (long long) r.num_beams_total, (long long) r.num_returns,
              (long long) r.num_cleared_only, (long long) r.num_skipped, (long long) r.num_hits_in_grid, (long long) r.num_miss_updates);
}

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_gridmap_params) == 20 && sizeof(srrg2_gridmap_scan_params) == 72 && sizeof(srrg2_gridmap_result) == 48,
                "struct sizes");
  srrg2_gridmap_params p;
  std::memset(&p, 0xff, sizeof(p));
  srrg2_gridmap_default_params(&p);
  REQUIRE(p.rows == 0 && p.cols == 0 && p.resolution == 0.05f && p.origin[0] == 0.f && p.origin[1] == 0.f);
  srrg2_gridmap_scan_params s;
  std::memset(&s, 0xff, sizeof(s));
  srrg2_gridmap_default_scan_params(&s);
  REQUIRE(s.num_beams == 0 && s.range_min == 0.05f && s.range_max == 30.f && s.clear_beyond_max == 1);
  for (int i = 0; i < 9; ++i) REQUIRE(s.sensor_in_robot[i] == (i % 4 == 0 ? 1.f : 0.f));
  // refused without a handle: the parameters are checked first
  p.resolution = 0.f;
  REQUIRE(srrg2_gridmap_reset(nullptr, &p) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "resolution") != nullptr);
  p.resolution = 0.05f;
  REQUIRE(srrg2_gridmap_reset(nullptr, &p) == SRRG2_E_INVALID);  // only the handle is missing now
  REQUIRE(std::strstr(srrg2_amd_last_error(), "null handle") != nullptr);
  s.angle_increment = 0.01, s.num_beams = 4;
  float r4[4] = {1, 1, 1, 1}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  REQUIRE(srrg2_gridmap_integrate_scans(nullptr, r4, 1, eye, SRRG2_MEM_HOST, &s, 3, nullptr) == SRRG2_E_INVALID);
  REQUIRE(std::strstr(srrg2_amd_last_error(), "weight") != nullptr);
  REQUIRE(srrg2_gridmap_destroy(nullptr) == 0);
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  // the case file: rows, cols, K, num_beams, clear; resolution, origin, range_min, range_max; bearings; mount; poses; ranges
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[5];
  float fl[5], mount[9];
  double bearing[2];
  REQUIRE(std::fread(shape, 4, 5, f) == 5 && std::fread(fl, 4, 5, f) == 5 && std::fread(bearing, 8, 2, f) == 2 &&
          std::fread(mount, 4, 9, f) == 9);
  const int K = shape[2], nb = shape[3];
  std::vector<float> poses((size_t) K * 9), ranges((size_t) K * nb);
  REQUIRE(std::fread(poses.data(), 4, poses.size(), f) == poses.size() && std::fread(ranges.data(), 4, ranges.size(), f) == ranges.size());
  std::fclose(f);
  GridMap map;
  map.params.rows = shape[0], map.params.cols = shape[1], map.params.resolution = fl[0];
  map.params.origin[0] = fl[1], map.params.origin[1] = fl[2];
  map.scan.angle_min = bearing[0], map.scan.angle_increment = bearing[1], map.scan.num_beams = nb;
  map.scan.range_min = fl[3], map.scan.range_max = fl[4], map.scan.clear_beyond_max = shape[4];
  std::memcpy(map.scan.sensor_in_robot, mount, sizeof(mount));
  bool thrown = false;  // no grid yet
  try { map.integrate(ranges.data(), K, poses.data()); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  map.reset();
  dump_result("all", map.integrate(ranges.data(), K, poses.data()));
  const int half = K / 2;
  dump_result("out", map.remove(ranges.data(), half, poses.data()));
  map.integrateQueued(ranges.data(), 1, poses.data());  // (the first scan back in, without waiting)
  std::vector<int32_t> hits, misses;
  map.counts(hits, misses);
  std::printf("hits");
  for (int32_t v : hits) std::printf(" %d", v);
  std::printf("\nmisses");
  for (int32_t v : misses) std::printf(" %d", v);
  std::printf("\nimage");
  for (uint8_t v : map.render(2)) std::printf(" %d", (int) v);
  std::printf("\n");
  Scene<2> scene;
  map.toScene(scene, 2, 60);
  std::vector<float> pts, nrm;
  scene.get(pts, nrm);
  std::printf("points");
  for (float v : pts) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    std::printf(" %08x", u);
  }
  std::printf("\nindices");
  for (int v : scene.globalIndices()) std::printf(" %d", v);
  std::printf("\n");
  thrown = false;  // a 3-D scene is refused and stays as it was
  Scene<3> wrong;
  try { srrg2_slam_amd::check(srrg2_gridmap_to_scene(map.handle(), 1, 50, wrong.handle())); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && wrong.size() == 0);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "gridmap.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "gridmap"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_gridmap_compile_and_link(tmp_path):
    """... and the defaults, the struct sizes and the refusals without a handle hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


@pytest.mark.gpu
def test_cpp_gridmap_bit_for_bit(product, tmp_path):
    import gridmap_cases as gc
    import gridmap_restatement as gr

    mount = gc.pose(0.1, -0.05, 0.3)
    g, sc, poses, ranges = gc.shape_case(((64, 64), 6, 361), seed=31, sensor_in_robot=mount, range_max=1.2)
    ranges = gc.mixed(ranges, seed=32)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([g["rows"], g["cols"], 6, 361, 1], np.int32).tobytes())
        f.write(np.array([g["res"], g["ox"], g["oy"], sc["range_min"], sc["range_max"]], np.float32).tobytes())
        f.write(np.array([sc["angle_min"], sc["angle_increment"]], np.float64).tobytes())
        f.write(mount.astype(np.float32).tobytes() + poses.astype(np.float32).tobytes() + ranges.astype(np.float32).tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    h, m = gr.new_planes(g)
    keys = ("num_beams_total", "num_returns", "num_cleared_only", "num_skipped", "num_hits_in_grid", "num_miss_updates")
    r_all = gr.integrate(h, m, ranges, poses, sc, g)
    r_out = gr.integrate(h, m, ranges[:3], poses[:3], sc, g, -1)
    gr.integrate(h, m, ranges[:1], poses[:1], sc, g)
    assert r_all["num_cleared_only"] > 0 and r_all["num_skipped"] > 0 and h.any()
    assert list(_ints(lines["all"])) == [r_all[k] for k in keys] and list(_ints(lines["out"])) == [r_out[k] for k in keys]
    assert np.array_equal(_ints(lines["hits"]).reshape(h.shape), h) and np.array_equal(_ints(lines["misses"]).reshape(m.shape), m)
    assert np.array_equal(_ints(lines["image"]).reshape(h.shape), gr.render(h, m, 2))
    pts, idx = gr.to_scene(h, m, g, 2, 60)
    assert len(idx) > 10 and np.array_equal(_ints(lines["indices"]), idx)
    got = np.array([int(w, 16) for w in lines["points"].split()[1:]], np.uint32).view(np.float32).reshape(-1, 2)
    assert got.tobytes() == pts.tobytes()
