// scene_device.h -- what the kernels that move scene points share: scene.hip (clip, merge) and normals.hip
// (drop_points_without_normal).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// what a feature-carrying kernel needs: source (measurement / full scene) and destination (scene / clipped scene) arrays; a
// null pair = that field is absent.  Descriptor halves move as 16-byte vectors.
struct Feat {
  const uint4* src_desc;
  const float* src_inten;
  uint4* dst_desc;
  float* dst_inten;
};

__device__ __forceinline__ void move_features(const Feat& f, int from, int to) {
  if (f.dst_desc) {
    const uint4 a = f.src_desc[2 * (size_t) from], b = f.src_desc[2 * (size_t) from + 1];
    f.dst_desc[2 * (size_t) to]     = a;
    f.dst_desc[2 * (size_t) to + 1] = b;
  }
  if (f.dst_inten) f.dst_inten[to] = f.src_inten[from];
}

// grid of the one-thread-per-point kernels (blockDim = 256, grid-stride loops)
int blocks_for(int n) {
  int b = (n + 255) / 256;
  return b < 1 ? 1 : (b > 2048 ? 2048 : b);
}

}  // namespace
