"""The C++ mirror of the ring tables and the de-skew (LidarSweepAdaptor::setRingElevations / setTimes / setMotion and
SceneClipperSpherical::setRingElevations in include/srrg2_slam_amd.hpp): one small translation unit compiled with plain g++
against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg adapts a moving sweep with a
two-block ring table and its motion (XYZIT records from the host, compact), clips a map with the same table and prints bit
patterns, which must be those of the restatement (tests/lidar_motion_restatement.py)."""
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

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_spherical_model) == 48 && sizeof(srrg2_lidar_adaptor_params) == 72 &&
                sizeof(srrg2_spherical_clip_params) == 104 && sizeof(srrg2_lidar_sweep_extras) == 104, "struct sizes");
  LidarSweepAdaptor probe;
  const srrg2_lidar_sweep_extras& x = probe.extras();
  REQUIRE(!x.ring_elevations && !x.times && x.time_stride_bytes == 0 && x.deskew == 0 && x.reference == 1.0);
  REQUIRE(x.time_begin == 0.0 && x.time_end == 0.0 && x.reserved[0] == 0 && x.reserved[1] == 0);
  REQUIRE(x.motion[0] == 1.f && x.motion[5] == 1.f && x.motion[10] == 1.f && x.motion[3] == 0.f && x.motion[1] == 0.f);
  REQUIRE(probe.ringElevations().empty());
  double table[4] = {-0.3, -0.1, 0.1, 0.3};
  probe.setRingElevations(table, 4);
  table[0] = 9.0;  // (the mirror owns a copy)
  REQUIRE(probe.ringElevations().size() == 4 && probe.ringElevations()[0] == -0.3);
  probe.setRingElevations(nullptr, 0);
  REQUIRE(probe.ringElevations().empty());
  Isometry<3> M = Isometry<3>::Identity();
  M.data()[3] = 0.25f;
  probe.setMotion(M, 0.5);
  REQUIRE(probe.extras().deskew == 1 && probe.extras().reference == 0.5 && probe.extras().motion[3] == 0.25f);
  float tm[2] = {0.f, 1.f};
  probe.setTimes(tm, 4, 0.0, 1.0);
  REQUIRE(probe.extras().times == tm && probe.extras().time_stride_bytes == 4 && probe.extras().time_end == 1.0);
  SceneClipperSpherical idle;
  REQUIRE(idle.ringElevations().empty());
  table[0] = -0.3;
  idle.setRingElevations(table, 4);
  REQUIRE(idle.ringElevations().size() == 4 && idle.ringElevations()[3] == 0.3);
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[3];  // rows, cols, n
  float motion[12], margin = 0.f;
  double reference = 0.0;
  REQUIRE(std::fread(shape, 4, 3, f) == 3 && std::fread(motion, 4, 12, f) == 12 && std::fread(&margin, 4, 1, f) == 1);
  REQUIRE(std::fread(&reference, 8, 1, f) == 1);
  std::vector<double> rings((size_t) shape[0]);
  REQUIRE(std::fread(rings.data(), 8, rings.size(), f) == rings.size());
  std::vector<float> xyzit((size_t) shape[2] * 5);
  REQUIRE(std::fread(xyzit.data(), 4, xyzit.size(), f) == xyzit.size());
  std::fclose(f);

  Scene<3> meas, full, clipped;
  LidarSweepAdaptor ad;
  ad.setFullTurnModel(shape[0], shape[1], rings.front(), rings.back());
  ad.param.compact = 1;
  ad.setMeas(&meas);
  ad.setRawData(xyzit.data(), 20, shape[2], xyzit.data() + 3, 20);
  ad.setRingElevations(rings.data(), shape[0]);
  ad.setTimes(xyzit.data() + 4, 20, 0.0, 1.0);
  Isometry<3> motion_iso;
  std::memcpy(motion_iso.data(), motion, sizeof(motion));
  ad.setMotion(motion_iso, reference);
  ad.compute();
  REQUIRE(ad.status() == AdaptorBase_::Ready && ad.last().num_raw == shape[2] && ad.last().scene_size == meas.size());
  std::vector<float> pts, nrm;
  meas.get(pts, nrm);
  dump("points", pts.data(), pts.size());
  dump("normals", nrm.data(), nrm.size());
  dump_ints("gidx", meas.globalIndices());
  std::printf("result %d %d %d\n", ad.last().num_in_range, ad.last().num_valid, ad.last().scene_size);
  // a table of the wrong length is refused by the mirror, a non-monotonic one by the library; the scene stays
  {
    LidarSweepAdaptor bad;
    bad.setFullTurnModel(shape[0], shape[1], rings.front(), rings.back());
    bad.setMeas(&meas);
    bad.setRawData(xyzit.data(), 20, shape[2]);
    bad.setRingElevations(rings.data(), shape[0] - 1);
    bool thrown = false;
    try { bad.compute(); } catch (const std::exception&) { thrown = true; }
    REQUIRE(thrown && meas.size() == (int) pts.size() / 3);
    std::vector<double> twisted(rings);
    twisted[2] = twisted[1];
    bad.setRingElevations(twisted.data(), shape[0]);
    thrown = false;
    try { bad.compute(); } catch (const std::exception&) { thrown = true; }
    REQUIRE(thrown && bad.status() == AdaptorBase_::Error && meas.size() == (int) pts.size() / 3);
  }
  // the map: the measurement itself, seen again from its own frame through the same table
  full.set(pts.data(), 12, nrm.data(), 12, (int) pts.size() / 3);
  SceneClipperSpherical clipper;
  clipper.setFullScene(&full);
  clipper.setClippedSceneInRobot(&clipped);
  clipper.setRobotInLocalMap(Isometry<3>::Identity());
  clipper.setModel(ad.param.model);
  clipper.setRingElevations(rings.data(), shape[0]);
  clipper.param.occlusion_margin = margin;
  clipper.compute();
  REQUIRE(clipper.status() == SceneClipperSpherical::Successful && clipper.last().num_kept == clipped.size());
  std::vector<float> cp, cn;
  clipped.get(cp, cn);
  dump("clip_points", cp.data(), cp.size());
  dump("clip_normals", cn.data(), cn.size());
  dump_ints("clip_gidx", clipper.globalIndices());
  std::printf("clip_result %d %d %d\n", clipper.last().num_valid, clipper.last().num_in_view, clipper.last().num_kept);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "lidar_motion.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "lidar_motion"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_lidar_motion_compiles_and_links(tmp_path):
    """... and the new setters' defaults and copies hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def _floats(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


@pytest.mark.gpu
def test_cpp_lidar_motion_through_the_mirror(product, tmp_path):
    import lidar_motion_cases as mc
    import lidar_motion_restatement as mr

    c = mc.moving_case("two_block_desc")
    m, e, reference, margin = c["model"], c["ring_elevations"], 0.5, 0.1
    xyzit = np.concatenate([c["points"], c["intensity"][:, None], c["times"][:, None]], axis=1).astype(np.float32)
    path = tmp_path / "sweep.bin"
    with open(path, "wb") as f:
        f.write(np.array([m.rows, m.cols, len(xyzit)], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["motion"], np.float32).tobytes())
        f.write(np.float32(margin).tobytes())
        f.write(np.float64(reference).tobytes())
        f.write(np.ascontiguousarray(e, np.float64).tobytes())
        f.write(xyzit.tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    want = mr.adapt_lidar_sweep_ex(c["points"], m, ring_elevations=e, motion=c["motion"], reference=reference, times=c["times"],
                                   time_begin=0.0, time_end=1.0, compact=True, intensity=c["intensity"])
    assert mr.same_bits(_floats(lines["points"]).reshape(-1, 3), want["points"])
    assert mr.same_bits(_floats(lines["normals"]).reshape(-1, 3), want["normals"])
    assert np.array_equal(_ints(lines["gidx"]), want["global_indices"])
    assert list(_ints(lines["result"])) == [want["num_in_range"], want["num_valid"], want["scene_size"]]
    assert want["num_valid"] > 3000
    clip = mr.clip_spherical_rings(want["points"], np.eye(3, 4, dtype=np.float32), m, e, None, margin, normals=want["normals"])
    assert mr.same_bits(_floats(lines["clip_points"]).reshape(-1, 3), clip["points"])
    assert mr.same_bits(_floats(lines["clip_normals"]).reshape(-1, 3), clip["normals"])
    assert np.array_equal(_ints(lines["clip_gidx"]), clip["global_indices"])
    assert list(_ints(lines["clip_result"])) == [clip["num_valid"], clip["num_in_view"], clip["num_kept"]]
    assert 0 < clip["num_kept"] <= clip["num_in_view"]
