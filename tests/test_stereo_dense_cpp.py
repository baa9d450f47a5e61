"""The C++ mirror of the dense stereo adaptor (StereoDenseAdaptor in include/srrg2_slam_amd.hpp): one small translation unit
compiled with plain g++ against include/ and linked with the built library.  Compiling, linking, the defaults and the struct
sizes need no GPU; the GPU leg runs a pair through the mirror, organised and compact, and prints bit patterns, which must be
those of the restatement (tests/stereo_dense_restatement.py)."""
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

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_dense_stereo_params) == 44 && sizeof(srrg2_dense_stereo_result) == 32, "struct sizes");
  StereoDenseAdaptor probe;
  REQUIRE(probe.stereo.baseline == 0.f && probe.stereo.min_disparity == 1 && probe.stereo.max_disparity == 64);
  REQUIRE(probe.stereo.paths == 4 && probe.stereo.p1 == 8 && probe.stereo.p2 == 48 && probe.stereo.uniqueness_ratio == 10);
  REQUIRE(probe.stereo.lr_check == 1 && probe.stereo.lr_tolerance == 1 && probe.stereo.subpixel == 1 && probe.stereo.reserved == 0);
  REQUIRE(probe.camera.depth_scale == 0.001f && probe.camera.rows == 0);
  REQUIRE(probe.status() == AdaptorBase_::Initializing && probe.disparity().empty());
  bool thrown = false;
  try { probe.compute(); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  {  // refused before a device is touched: no baseline
    uint8_t px[7 * 16] = {0};
    probe.camera.rows = 7, probe.camera.cols = 16;
    probe.setRawData(px, 16, px, 16);
    thrown = false;
    try { probe.compute(true, true); } catch (const std::exception&) { thrown = true; }
    REQUIRE(thrown && probe.status() == AdaptorBase_::Error && probe.disparity().empty());
  }
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[2];
  float K[9], baseline;
  REQUIRE(std::fread(shape, 4, 2, f) == 2 && std::fread(K, 4, 9, f) == 9 && std::fread(&baseline, 4, 1, f) == 1);
  const size_t n = (size_t) shape[0] * shape[1];
  std::vector<uint8_t> left(n), right(n);
  REQUIRE(std::fread(left.data(), 1, n, f) == n && std::fread(right.data(), 1, n, f) == n);
  std::fclose(f);

  Scene<3> meas;
  const char* names[2] = {"organised", "compact"};
  char tag[64];
  for (int k = 0; k < 2; ++k) {
    StereoDenseAdaptor ad;
    std::memcpy(ad.camera.camera_matrix, K, sizeof(K));
    ad.camera.rows = shape[0], ad.camera.cols = shape[1];
    ad.camera.compact = k;
    ad.stereo.baseline = baseline;
    ad.stereo.max_disparity = 24;
    ad.setMeas(&meas);
    ad.setRawData(left.data(), shape[1], right.data(), shape[1]);
    REQUIRE(ad.status() == AdaptorBase_::Error);
    ad.compute(true, true);
    REQUIRE(ad.status() == AdaptorBase_::Ready && ad.last().scene_size == meas.size() && ad.disparity().size() == n);
    REQUIRE(meas.hasIntensity() && !meas.hasDescriptors());
    std::vector<float> pts, nrm, inten;
    std::vector<uint8_t> desc;
    meas.get(pts, nrm);
    meas.getFeatures(desc, inten);
    std::snprintf(tag, sizeof(tag), "%s_disparity", names[k]);
    dump(tag, ad.disparity().data(), n);
    std::snprintf(tag, sizeof(tag), "%s_points", names[k]);
    dump(tag, pts.data(), pts.size());
    std::snprintf(tag, sizeof(tag), "%s_normals", names[k]);
    dump(tag, nrm.data(), nrm.size());
    std::snprintf(tag, sizeof(tag), "%s_intensity", names[k]);
    dump(tag, inten.data(), inten.size());
    std::printf("%s_gidx", names[k]);
    for (int i : meas.globalIndices()) std::printf(" %d", i);
    const srrg2_dense_stereo_result& r = ad.result();
    std::printf("\n%s_result %d %d %d %d %d %d %d %d\n", names[k], r.status, r.num_pixels, r.num_evaluated, r.num_unique,
                r.num_consistent, r.num_in_range, r.num_valid, r.scene_size);
  }
  {  // the disparity alone, no scene
    StereoDenseAdaptor ad;
    std::memcpy(ad.camera.camera_matrix, K, sizeof(K));
    ad.camera.rows = shape[0], ad.camera.cols = shape[1];
    ad.stereo.baseline = baseline;
    ad.stereo.max_disparity = 24;
    ad.setRawData(left.data(), shape[1], right.data(), shape[1]);
    ad.compute(false, true);
    REQUIRE(ad.status() == AdaptorBase_::Ready);
    dump("alone_disparity", ad.disparity().data(), n);
  }
  {  // a refused call leaves the scene as it was
    const int before = meas.size();
    StereoDenseAdaptor bad;
    bad.camera.rows = shape[0], bad.camera.cols = shape[1];
    bad.stereo.baseline = baseline;
    bad.stereo.paths = 8;
    bad.setMeas(&meas);
    bad.setRawData(left.data(), shape[1], right.data(), shape[1]);
    bool refused = false;
    try { bad.compute(true, true); } catch (const std::exception&) { refused = true; }
    REQUIRE(refused && bad.status() == AdaptorBase_::Error && meas.size() == before && bad.disparity().empty());
  }
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "stereo_dense.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "stereo_dense"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_stereo_dense_compile_and_link(tmp_path):
    """... and the mirror's defaults, the struct sizes and a refusal hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def _floats(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


@pytest.mark.gpu
def test_cpp_stereo_dense_bit_for_bit(product, tmp_path):
    import adaptor_restatement as ar
    import stereo_dense_cases as dc
    import stereo_dense_restatement as sd

    name = "two_plane_67x101"
    left, right = dc.named(name)
    path = tmp_path / "pair.bin"
    with open(path, "wb") as f:
        f.write(np.array(left.shape, np.int32).tobytes())
        f.write(np.array(dc.CAMERA, np.float32).tobytes())
        f.write(np.array([dc.BASELINE], np.float32).tobytes())
        f.write(left.tobytes())
        f.write(right.tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    for mode, compact in (("organised", 0), ("compact", 1)):
        want = dc.want(name, compact=compact, **dc.TWO_PLANE_RANGE)
        assert want["scene_size"] > 1000
        assert _floats(lines[mode + "_disparity"]).tobytes() == want["disparity"].tobytes(), mode
        assert ar.same_bits(_floats(lines[mode + "_points"]).reshape(-1, 3), want["points"]), mode
        assert ar.same_bits(_floats(lines[mode + "_normals"]).reshape(-1, 3), want["normals"]), mode
        assert ar.same_bits(_floats(lines[mode + "_intensity"]), want["intensity"]), mode
        gidx = want["global_indices"] if compact else np.zeros(0, np.int64)
        assert np.array_equal(_ints(lines[mode + "_gidx"]), gidx), mode
        assert list(_ints(lines[mode + "_result"])) == [want[k] for k in sd.COUNTERS], mode
    assert _floats(lines["alone_disparity"]).tobytes() == dc.want(name, **dc.TWO_PLANE_RANGE)["disparity"].tobytes()
