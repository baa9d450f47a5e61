"""The C++ mirror of the rectification stage (ImageRectifier / StereoRectifier in include/srrg2_slam_amd.hpp): one small translation
unit compiled with plain g++ against include/ and linked with the built library.  Compiling, linking, the defaults, the struct
sizes, the host-only stereo calibration and the refusals that need no device run without a GPU; the GPU leg prints the bit
patterns of one map and one rectified image (and of a pair), which must be those of the restatement
(tests/rectify_restatement.py)."""
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

static void dump_doubles(const char* tag, const double* v, size_t n) {
  std::printf("%s", tag);
  for (size_t i = 0; i < n; ++i) {
    uint64_t u;
    std::memcpy(&u, &v[i], 8);
    std::printf(" %016llx", (unsigned long long) u);
  }
  std::printf("\n");
}

int main(int argc, char** argv) {
  static_assert(sizeof(srrg2_rectifier_params) == 35 * 8 + 16 && sizeof(srrg2_rectifier_info) == 24, "struct sizes");
  srrg2_rectifier_params p;
  std::memset(&p, 0xff, sizeof(p));
  srrg2_rectifier_default_params(&p);
  for (int i = 0; i < 9; ++i) REQUIRE(p.camera_matrix[i] == 0.0 && p.new_camera_matrix[i] == 0.0 && p.rotation[i] == (i % 4 == 0 ? 1.0 : 0.0));
  for (int i = 0; i < 8; ++i) REQUIRE(p.distortion[i] == 0.0);
  REQUIRE(p.src_rows == 0 && p.src_cols == 0 && p.dst_rows == 0 && p.dst_cols == 0);
  // refused without a handle: the parameters are checked first
  REQUIRE(srrg2_rectifier_set(nullptr, &p, nullptr) == SRRG2_E_INVALID);  // fx = 0
  p.camera_matrix[0] = p.camera_matrix[4] = p.new_camera_matrix[0] = p.new_camera_matrix[4] = 100.0;
  p.camera_matrix[1] = 0.5;
  REQUIRE(srrg2_rectifier_set(nullptr, &p, nullptr) == SRRG2_E_UNSUPPORTED);
  p.camera_matrix[1] = 0.0;
  REQUIRE(srrg2_rectifier_set(nullptr, &p, nullptr) == SRRG2_E_INVALID);  // only the handle is missing now
  {  // the calibration's rotations need no device
    const double K[9] = {80, 0, 50, 0, 80, 33, 0, 0, 1}, I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {-0.3, 0, 0}, zero[3] = {0, 0, 0};
    double R1[9], R2[9], Kn[9], b = 0;
    StereoRectifier::rotations(K, K, I, t, R1, R2, Kn, &b);
    REQUIRE(b == 0.3 && Kn[0] == 80 && Kn[4] == 80 && Kn[2] == 50 && Kn[5] == 33);
    for (int i = 0; i < 9; ++i) REQUIRE(R1[i] == I[i] && R2[i] == I[i]);
    bool thrown = false;
    try { StereoRectifier::rotations(K, K, I, zero, R1, R2, Kn, &b); } catch (const std::exception&) { thrown = true; }
    REQUIRE(thrown);
  }
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only: nothing above touches a device)

  // the case file: shapes, then the doubles of the single camera and of the rig, then the images
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  int32_t shape[4];
  double cam[9 + 8 + 9 + 9], rig[9 + 8 + 9 + 3];
  REQUIRE(std::fread(shape, 4, 4, f) == 4 && std::fread(cam, 8, 35, f) == 35 && std::fread(rig, 8, 29, f) == 29);
  const size_t ns = (size_t) shape[0] * shape[1], nd = (size_t) shape[2] * shape[3];
  std::vector<uint8_t> src(ns), left(nd), right(nd);
  REQUIRE(std::fread(src.data(), 1, ns, f) == ns && std::fread(left.data(), 1, nd, f) == nd && std::fread(right.data(), 1, nd, f) == nd);
  std::fclose(f);
  {
    ImageRectifier r;
    std::memcpy(r.params.camera_matrix, cam, 72);
    std::memcpy(r.params.distortion, cam + 9, 64);
    std::memcpy(r.params.rotation, cam + 17, 72);
    std::memcpy(r.params.new_camera_matrix, cam + 26, 72);
    r.params.src_rows = shape[0], r.params.src_cols = shape[1], r.params.dst_rows = shape[2], r.params.dst_cols = shape[3];
    const srrg2_rectifier_info& info = r.set();
    std::printf("info %d %d %d %d %d %d\n", info.num_pixels, info.num_valid, info.first_row, info.last_row, info.first_col, info.last_col);
    std::printf("map");
    for (int32_t v : r.map()) std::printf(" %d", v);
    std::printf("\n");
    std::vector<uint8_t> out(nd, 0xaa);
    r.rectify(src.data(), SRRG2_IMAGE_U8, shape[1], out.data(), shape[3], SRRG2_MEM_HOST, SRRG2_MEM_HOST, nullptr, 200);
    std::printf("image");
    for (uint8_t v : out) std::printf(" %d", (int) v);
    std::printf("\n");
    srrg2_depth_adaptor_params c;
    srrg2_adapt_default_depth_params(&c);
    r.camera(c);
    REQUIRE(c.rows == shape[2] && c.cols == shape[3] && c.camera_matrix[0] == (float) cam[26] && c.camera_matrix[5] == (float) cam[31]);
    REQUIRE(c.depth_scale == 0.001f);
    bool refused = false;  // a depth image under this camera's rotation
    std::vector<uint16_t> d16(ns), o16(nd, 7);
    try { r.rectify(d16.data(), SRRG2_IMAGE_U16, 2 * shape[1], o16.data(), 2 * shape[3]); } catch (const std::exception&) { refused = true; }
    REQUIRE(refused && o16[0] == 7 && o16[nd - 1] == 7);
  }
  {  // the rig: sources and targets of the target's shape
    StereoRectifier s;
    s.setCalibration(rig, rig + 9, rig, rig + 9, rig + 17, rig + 26, shape[2], shape[3], shape[2], shape[3]);
    dump_doubles("R1", s.R1, 9);
    dump_doubles("R2", s.R2, 9);
    dump_doubles("Knew", s.new_camera_matrix, 9);
    dump_doubles("baseline", &s.baseline, 1);
    std::vector<uint8_t> ol(nd), orr(nd);
    s.rectify(left.data(), shape[3], right.data(), shape[3], ol.data(), shape[3], orr.data(), shape[3]);
    std::printf("left");
    for (uint8_t v : ol) std::printf(" %d", (int) v);
    std::printf("\nright");
    for (uint8_t v : orr) std::printf(" %d", (int) v);
    std::printf("\n");
  }
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "rectify.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "rectify"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_rectify_compile_and_link(tmp_path):
    """... and the defaults, the struct sizes, the host-only calibration and the refusals without a handle hold without a device"""
    exe = _build(tmp_path)
    out = subprocess.run([exe, "link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


def _doubles(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint64).view(np.float64)


@pytest.mark.gpu
def test_cpp_rectify_bit_for_bit(product, tmp_path):
    import rectify_cases as rc
    import rectify_restatement as rr

    K, dist, R, shape = rc.model("small", "tilted")
    dst = (67, 101)
    new_K = rc.target_K("small", dst)
    new_K[0, 0] *= 0.8  # (a shorter focal length: the target sees past the source's edges, so some entries are invalid)
    new_K[1, 1] *= 0.8
    g = rc.rig()
    assert g["shape"] == dst
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array(shape + dst, np.int32).tobytes())
        for a in (K, dist, R, new_K, rc.RIG_K, rc.RIG_DISTORTION, rc.RIG_R, rc.RIG_T):
            f.write(np.asarray(a, np.float64).tobytes())
        f.write(rc.image(shape).tobytes())
        f.write(g["raw"][0].tobytes())
        f.write(g["raw"][1].tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    uv, info = rr.build_map(K, dist, R, new_K, shape, dst)
    assert 0 < info["num_valid"] < info["num_pixels"]
    assert list(_ints(lines["info"])) == [info[k] for k in ("num_pixels", "num_valid", "first_row", "last_row", "first_col", "last_col")]
    assert np.array_equal(_ints(lines["map"]).reshape(dst + (2,)), uv)
    assert np.array_equal(_ints(lines["image"]).reshape(dst), rr.remap(uv, rc.image(shape), 200))
    for tag, want in (("R1", g["R1"]), ("R2", g["R2"]), ("Knew", g["Knew"]), ("baseline", np.array([g["baseline"]]))):
        assert _doubles(lines[tag]).tobytes() == np.asarray(want, np.float64).tobytes(), tag
    wl, wr = rc.rig_rectified()
    assert np.array_equal(_ints(lines["left"]).reshape(dst), wl) and np.array_equal(_ints(lines["right"]).reshape(dst), wr)
