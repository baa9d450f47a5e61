"""The C++ mirror of the stereo-feature adaptor (StereoFeatureAdaptor in include/srrg2_slam_amd.hpp) compiles as plain C++17 with
every warning an error: one small translation unit that names every member, syntax-checked with g++.  Needs no GPU and no
library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include <cstdint>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

static_assert(sizeof(srrg2_stereo_params) == 32 && sizeof(srrg2_stereo_match) == 16 && sizeof(srrg2_stereo_result) == 32,
              "struct sizes");

int use(Scene<3>& meas, const uint8_t* left, const uint8_t* right, int rows, int cols) {
  StereoFeatureAdaptor ad;
  ad.camera.rows = rows, ad.camera.cols = cols;
  ad.stereo.baseline = 0.1f;
  ad.stereo.row_tolerance = 2;
  ad.param.max_features = 500;
  ad.setMeas(&meas);
  ad.setRawData(left, cols, right, cols);
  if (ad.status() != AdaptorBase_::Error) return -1;
  ad.compute();
  const srrg2_stereo_result& r = ad.result();
  const std::vector<srrg2_keypoint>& kp = ad.keypoints();
  const std::vector<srrg2_stereo_match>& m = ad.matches();
  int sum = r.num_left + r.num_right + r.num_matched + r.num_mutual + r.num_in_range + ad.last().scene_size;
  for (size_t i = 0; i < m.size(); ++i) sum += m[i].left_pixel - kp[i].pixel + m[i].right_pixel + m[i].distance + (int) m[i].disparity;
  ad.reset();
  return sum;
}
"""


def test_cpp_stereo_mirror_compiles(tmp_path):
    src = tmp_path / "stereo.cpp"
    src.write_text(SOURCE)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
