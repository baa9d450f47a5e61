"""The C++ mirror of the feature tracker (FeatureTracker in include/srrg2_slam_amd.hpp) compiles as plain C++17 with every warning
an error: one small translation unit that names every member, syntax-checked with g++; the C structs keep their sizes.  Needs no
GPU and no library."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include <cstdint>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

static_assert(sizeof(srrg2_track_params) == 72 && sizeof(srrg2_track_result) == 32 && sizeof(srrg2_correspondence) == 12,
              "struct sizes");
static_assert(SRRG2_AMD_ABI_VERSION == 4, "adding a function does not bump the ABI");

int use(Scene<3>& clipped_map, const Scene<3>& meas, const float* K, int rows, int cols) {
  FeatureTracker ft;
  ft.setCameraMatrix(K);
  ft.param.image_rows = rows, ft.param.image_cols = cols;
  ft.param.depth_min = 0.5f, ft.param.depth_max = 6.f;
  ft.param.search_radius = 12, ft.param.max_distance = 40, ft.param.min_margin = 3, ft.param.cross_check = 1;
  ft.setFixed(&meas);
  ft.setMoving(&clipped_map);
  ft.setMovingInSensor(Isometry3f::Identity());
  ft.compute();
  const srrg2_track_result& r = ft.result();
  const CorrespondenceVector& c = ft.correspondences();
  const CorrespondenceVector m = FeatureTracker::toMerger(c, clipped_map.globalIndices());
  MergerCorrespondenceHomo<3> merger;
  merger.setCorrespondences(&m);
  int sum = r.num_moving + r.num_fixed + r.num_in_view + r.num_with_candidate + r.num_accepted + r.num_mutual + r.num_correspondences;
  for (size_t i = 0; i < c.size(); ++i) sum += c[i].fixed_idx + c[i].moving_idx + (int) c[i].response + m[i].fixed_idx;
  return sum;
}
"""


def test_cpp_tracking_mirror_compiles(tmp_path):
    src = tmp_path / "tracking.cpp"
    src.write_text(SOURCE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def test_ctypes_mirrors_keep_the_sizes():
    from srrg2_slam_interfaces_amd import _abi as abi

    assert C.sizeof(abi.TrackParams) == 72 and C.sizeof(abi.TrackResult) == 32
