"""The C++ mirror of the lidar frame (LidarSweepAdaptor and SceneClipperSpherical in include/srrg2_slam_amd.hpp): one small
translation unit compiled with plain g++ against include/ and linked with the built library.  Compiling and linking need no GPU;
the GPU leg runs adapt (two sweeps, compact) -> set (a map from the first) -> clip -> setFixed / setMoving -> compute() through
the mirror and prints bit patterns, which must be those of the restatement (tests/lidar_restatement.py) and of the oracle's
alignment of the restatement-made clouds."""
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

static void dump(const char* tag, const float* v, size_t n) {
  std::printf("%s", tag);
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &v[i], 4);
    std::printf(" %08x", u);
  }
  std::printf("\n");
}

static void dump_ints(const char* tag, const std::vector<int>& v) {
  std::printf("%s", tag);
  for (int i : v) std::printf(" %d", i);
  std::printf("\n");
}

static bool read_floats(std::FILE* f, std::vector<float>& v, int width) {
  int32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n <= 0) return false;
  v.resize((size_t) n * width);
  return std::fread(v.data(), 4, v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_spherical_model) == 48 && sizeof(srrg2_lidar_adaptor_params) == 72 &&
                sizeof(srrg2_spherical_clip_params) == 104, "struct sizes");
  LidarSweepAdaptor probe;
  REQUIRE(probe.param.normal_col_gap == 1 && probe.param.normal_row_gap == 1 && probe.param.normal_max_distance_squared == 1.f);
  REQUIRE(probe.param.drop_points_without_normal == 1 && probe.param.compact == 0 && probe.param.reserved == 0);
  REQUIRE(probe.param.model.range_min == 0.5f && probe.param.model.range_max == 120.f && probe.param.model.rows == 0);
  REQUIRE(probe.status() == AdaptorBase_::Initializing);
  SceneClipperSpherical idle;
  REQUIRE(idle.param.occlusion_margin == -1.f && idle.param.reserved == 0 && idle.param.sensor_in_robot[5] == 1.f);
  bool thrown = false;
  try { probe.setFullTurnModel(1, 8, -0.1, 0.1); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[2];
  double elevation[2];
  float margin = 0.f, gate = 0.f;
  REQUIRE(std::fread(shape, 4, 2, f) == 2 && std::fread(elevation, 8, 2, f) == 2);
  REQUIRE(std::fread(&margin, 4, 1, f) == 1 && std::fread(&gate, 4, 1, f) == 1);
  std::vector<float> sweep[2], hidden, hidden_normals;
  REQUIRE(read_floats(f, sweep[0], 4) && read_floats(f, sweep[1], 4) && read_floats(f, hidden, 3) && read_floats(f, hidden_normals, 3));
  std::fclose(f);

  // adapt: interleaved XYZI records from the host, compact
  Scene<3> meas[2], full, clipped;
  const char* names[2] = {"a", "b"};
  char tag[64];
  std::vector<float> pts[2], nrm[2];
  for (int k = 0; k < 2; ++k) {
    LidarSweepAdaptor ad;
    ad.setFullTurnModel(shape[0], shape[1], elevation[0], elevation[1]);
    ad.param.compact = 1;
    ad.setMeas(&meas[k]);
    ad.setRawData(sweep[k].data(), 16, (int) sweep[k].size() / 4, sweep[k].data() + 3, 16);
    REQUIRE(ad.status() == AdaptorBase_::Error);
    ad.compute();
    REQUIRE(ad.status() == AdaptorBase_::Ready && ad.last().num_raw == (int) sweep[k].size() / 4);
    REQUIRE(ad.last().scene_size == meas[k].size() && ad.last().num_valid == meas[k].size() && meas[k].hasIntensity());
    meas[k].get(pts[k], nrm[k]);
    std::snprintf(tag, sizeof(tag), "%s_points", names[k]);
    dump(tag, pts[k].data(), pts[k].size());
    std::snprintf(tag, sizeof(tag), "%s_normals", names[k]);
    dump(tag, nrm[k].data(), nrm[k].size());
    std::snprintf(tag, sizeof(tag), "%s_gidx", names[k]);
    dump_ints(tag, meas[k].globalIndices());
    std::printf("%s_result %d %d %d\n", names[k], ad.last().num_in_range, ad.last().num_valid, ad.last().scene_size);
  }
  // a refused adapt leaves the scene as it was
  {
    LidarSweepAdaptor bad;
    bad.setFullTurnModel(shape[0], shape[1], elevation[0], elevation[1]);
    bad.param.normal_row_gap = 0;
    bad.setMeas(&meas[0]);
    bad.setRawData(sweep[0].data(), 16, (int) sweep[0].size() / 4);
    thrown = false;
    try { bad.compute(); } catch (const std::exception&) { thrown = true; }
    REQUIRE(thrown && bad.status() == AdaptorBase_::Error && meas[0].size() == (int) pts[0].size() / 3);
  }

  // the map: the first measurement and what lies behind the wall, in the first sensor's frame
  std::vector<float> mp(pts[0]), mn(nrm[0]);
  mp.insert(mp.end(), hidden.begin(), hidden.end());
  mn.insert(mn.end(), hidden_normals.begin(), hidden_normals.end());
  full.set(mp.data(), 12, mn.data(), 12, (int) mp.size() / 3);
  SceneClipperSpherical clipper;
  clipper.setFullScene(&full);
  clipper.setClippedSceneInRobot(&clipped);
  clipper.setRobotInLocalMap(Isometry<3>::Identity());
  clipper.setModel(probe.param.model);  // (zeroed angles: refused)
  thrown = false;
  try { clipper.compute(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && clipper.status() == SceneClipperSpherical::Error);
  srrg2_spherical_model model;
  REQUIRE(srrg2_spherical_model_full_turn(&model, shape[0], shape[1], elevation[0], elevation[1]) == 0);
  clipper.setModel(model);
  clipper.param.occlusion_margin = margin;
  clipper.compute();
  REQUIRE(clipper.status() == SceneClipperSpherical::Successful && clipper.last().num_kept == clipped.size());
  std::vector<float> cp, cn;
  clipped.get(cp, cn);
  dump("clip_points", cp.data(), cp.size());
  dump("clip_normals", cn.data(), cn.size());
  dump_ints("clip_gidx", clipper.globalIndices());
  std::printf("clip_result %d %d %d\n", clipper.last().num_valid, clipper.last().num_in_view, clipper.last().num_kept);

  using Aligner = MultiAligner_<SRRG2_SE3_QUAT_RIGHT>;
  Aligner al(0);
  srrg2_slice_config cfg = Aligner::defaultSliceConfig();
  cfg.kind = SRRG2_SLICE_P2PLANE;
  cfg.finder = SRRG2_FINDER_NN_GATED;
  cfg.finder_max_distance = gate;
  cfg.robustifier = SRRG2_ROBUST_CAUCHY;
  cfg.robustifier_chi_threshold = 0.05f;
  cfg.finder_normal_cos = -2.f;
  cfg.min_num_correspondences = 0;
  const int si = al.addSlice(cfg);
  const float *movp, *movn, *fixp, *fixn;
  int nm = 0, nf = 0;
  clipped.deviceArrays(movp, movn, nm);
  meas[1].deviceArrays(fixp, fixn, nf);
  REQUIRE(movn && fixn);
  al.setFixed(si, fixp, 16, fixn, 16, nf, SRRG2_MEM_DEVICE);
  al.setMoving(si, movp, 16, movn, 16, nm, SRRG2_MEM_DEVICE);
  al.setMovingInFixed(Isometry<3>::Identity());
  al.compute();
  const Isometry<3>& X = al.movingInFixed();
  dump("estimate", X.data(), 12);
  std::printf("run %d %d %d\n", (int) al.status(), (int) al.iterationStats().size(),
              al.iterationStats().empty() ? -1 : al.iterationStats().back().num_correspondences);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "lidar.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "lidar"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_lidar_compiles_and_links(tmp_path):
    """... and the mirrors' defaults and the full-turn helper's refusal hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def _floats(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


@pytest.mark.gpu
def test_cpp_lidar_through_the_stack(product, oracle, tmp_path):
    import lidar_cases as lc
    import lidar_restatement as lr

    s = lc.stack_case()
    m = s["a"]["model"]
    hidden = len(s["map_points"]) - len(s["meas_a"]["points"])
    path = tmp_path / "sweeps.bin"
    with open(path, "wb") as f:
        f.write(np.array([m.rows, m.cols], np.int32).tobytes())
        f.write(np.array(s["a"]["elevation"], np.float64).tobytes())
        f.write(np.array([0.1, lc.GATE], np.float32).tobytes())
        for sweep in (s["a"], s["b"]):
            f.write(np.int32(len(sweep["points"])).tobytes())
            f.write(np.concatenate([sweep["points"], sweep["intensity"][:, None]], axis=1).astype(np.float32).tobytes())
        for arr in (s["map_points"][-hidden:], s["map_normals"][-hidden:]):
            f.write(np.int32(len(arr)).tobytes())
            f.write(np.ascontiguousarray(arr, np.float32).tobytes())
    # (the model the mirror builds from first / last elevation is the one the restatement used)
    again = lr.Model.full_turn(m.rows, m.cols, *s["a"]["elevation"])
    assert vars(again) == vars(m) and s["b"]["elevation"] == s["a"]["elevation"]
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    for name, want in (("a", s["meas_a"]), ("b", s["meas_b"])):
        assert lr.same_bits(_floats(lines[name + "_points"]).reshape(-1, 3), want["points"]), name
        assert lr.same_bits(_floats(lines[name + "_normals"]).reshape(-1, 3), want["normals"]), name
        assert np.array_equal(_ints(lines[name + "_gidx"]), want["global_indices"])
        assert list(_ints(lines[name + "_result"])) == [want["num_in_range"], want["num_valid"], want["scene_size"]]
    c = s["clipped"]
    assert lr.same_bits(_floats(lines["clip_points"]).reshape(-1, 3), c["points"])
    assert lr.same_bits(_floats(lines["clip_normals"]).reshape(-1, 3), c["normals"])
    assert np.array_equal(_ints(lines["clip_gidx"]), c["global_indices"])
    assert list(_ints(lines["clip_result"])) == [c["num_valid"], c["num_in_view"], c["num_kept"]]
    ref = lc.stack_oracle_run(oracle, s["meas_b"]["points"], s["meas_b"]["normals"], c["points"], c["normals"])
    status, iterations, ncorr = (int(w) for w in lines["run"].split()[1:])
    assert status == ref.status() and iterations == len(ref.iteration_stats())
    assert ncorr == ref.iteration_stats()[-1]["num_correspondences"] > c["num_kept"] // 2
    assert _floats(lines["estimate"]).tobytes() == np.ascontiguousarray(ref.moving_in_fixed(), np.float32).tobytes()
