"""The C++ mirror of the TSDF volume (TsdfVolume in include/srrg2_slam_amd.hpp): one small translation unit compiled with plain
g++ against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg fuses the wall case of
tests/tsdf_cases.py through the mirror class and prints the planes' sums and the raycast's bit patterns, which must be the numpy
restatement's (tests/tsdf_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

import tsdf_cases as tc
import tsdf_restatement as tr

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

static_assert(sizeof(srrg2_tsdf_params) == 32 && sizeof(srrg2_tsdf_frame_params) == 8 && sizeof(srrg2_tsdf_raycast_params) == 16, "");
static_assert(sizeof(srrg2_tsdf_result) == 32 && sizeof(srrg2_tsdf_raycast_result) == 28 && sizeof(srrg2_tsdf_export_result) == 8, "");

int main(int argc, char**) {
  if (argc > 1) return 0;  // (link check only)
  // the wall case of tests/tsdf_cases.py
  const int rows = 24, cols = 32;
  const float poses[3][12] = {{1, 0, 0, 0.0f, 0, 1, 0, 0.0f, 0, 0, 1, 0.0f},
                              {1, 0, 0, 0.1f, 0, 1, 0, -0.05f, 0, 0, 1, 0.1f},
                              {1, 0, 0, -0.08f, 0, 1, 0, 0.04f, 0, 0, 1, -0.15f}};
  std::vector<float> depth((size_t) 3 * rows * cols);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < rows * cols; ++i) depth[(size_t) k * rows * cols + i] = (float) (1.4 - (double) poses[k][11]);
  TsdfVolume vol;
  REQUIRE(vol.params.nx == 0 && vol.params.voxel_size == 0.02f && vol.frame.mu == 0.06f && vol.ray.min_weight == 1 && vol.ray.skip_empty == 0);
  vol.params.nx = 24, vol.params.ny = 20, vol.params.nz = 16, vol.params.voxel_size = 0.05f;
  vol.params.origin[0] = -0.6f, vol.params.origin[1] = -0.5f, vol.params.origin[2] = 1.0f;
  vol.reset();
  const float K[9] = {30, 0, 15.5f, 0, 30, 11.5f, 0, 0, 1};
  std::memcpy(vol.camera.camera_matrix, K, sizeof(K));
  vol.camera.rows = rows, vol.camera.cols = cols, vol.camera.depth_min = 0.4f, vol.camera.depth_max = 3.0f;
  vol.frame.mu = 0.15f;
  const srrg2_tsdf_result& res = vol.integrate(depth.data(), SRRG2_IMAGE_F32, 4 * cols, 3, &poses[0][0]);
  std::vector<int32_t> sum, weight, isum;
  vol.planes(sum, weight, isum);
  REQUIRE(isum.empty() && sum.size() == vol.voxels());
  long long s = 0, w = 0;
  for (size_t i = 0; i < sum.size(); ++i) s += sum[i], w += weight[i];
  std::printf("counters %lld %lld %lld %lld\nplanes %lld %lld\n", (long long) res.num_frames, (long long) res.num_pixels,
              (long long) res.num_valid_depth, (long long) res.num_voxel_updates, s, w);
  vol.ray.step = 0.05f;
  Scene<3> scene, cloud;
  const std::vector<float> image = vol.raycast(&poses[0][0], &scene);
  REQUIRE(scene.size() == rows * cols && vol.lastRaycast().num_pixels == rows * cols);
  std::printf("image");
  for (float f : image) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    std::printf(" %08x", u);
  }
  std::printf("\nsurface %d\nexport %d\n", vol.lastRaycast().num_surface, vol.toScene(cloud, 3));
  REQUIRE(cloud.size() > 0);
  // taken out again: zeros
  vol.remove(depth.data(), SRRG2_IMAGE_F32, 4 * cols, 3, &poses[0][0]);
  vol.planes(sum, weight, isum);
  for (size_t i = 0; i < sum.size(); ++i) REQUIRE(sum[i] == 0 && weight[i] == 0);
  bool thrown = false;
  vol.frame.mu = 0.f;  // refused
  try { vol.integrate(depth.data(), SRRG2_IMAGE_F32, 4 * cols, 3, &poses[0][0]); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "tsdf.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "tsdf"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_tsdf_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def _restated():
    vol, K, rows, cols, poses, depth, wall, mu = tc.wall_case()
    v = tr.volume(**vol)
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 3.0)
    planes = tr.new_planes(v)
    out = tr.integrate(planes, v, cam, depth, poses, mu)
    image, _ = tr.raycast(planes, v, cam, poses[0], 0.05)
    return out, planes, image, tr.to_scene(planes, v, 3)[2].size


def test_the_cpp_case_is_the_wall_case():
    """the constants written into the C++ source are those of tests/tsdf_cases.py"""
    vol, K, rows, cols, poses, depth, wall, mu = tc.wall_case()
    assert (rows, cols, wall, mu) == (24, 32, 1.4, 0.15) and vol == dict(nx=24, ny=20, nz=16, voxel_size=0.05, origin=(-0.6, -0.5, 1.0))
    assert np.array_equal(poses[:, :, 3], np.array([[0, 0, 0], [0.1, -0.05, 0.1], [-0.08, 0.04, -0.15]], np.float32))
    assert np.array_equal(poses[:, :, :3], np.tile(np.eye(3, dtype=np.float32), (3, 1, 1)))
    assert np.array_equal(K, np.array([[30, 0, 15.5], [0, 30, 11.5], [0, 0, 1]], np.float32))
    assert np.array_equal(depth[:, 0, 0], (1.4 - poses[:, 2, 3].astype(np.float64)).astype(np.float32))


@pytest.mark.gpu
def test_cpp_tsdf_matches_the_restatement(product, tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.strip()}
    want, planes, image, exported = _restated()
    assert [int(x) for x in lines["counters"]] == [want["num_frames"], want["num_pixels"], want["num_valid_depth"], want["num_voxel_updates"]]
    assert [int(x) for x in lines["planes"]] == [int(planes[0].sum(dtype=np.int64)), int(planes[1].sum(dtype=np.int64))]
    got = np.array([int(x, 16) for x in lines["image"]], np.uint32).view(np.float32).reshape(image.shape)
    assert tr.same_bits(got, image)
    assert int(lines["surface"][0]) == int((image != 0).sum()) > 0 and int(lines["export"][0]) == exported
