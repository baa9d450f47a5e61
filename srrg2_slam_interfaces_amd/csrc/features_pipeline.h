// features_pipeline.h -- the per-image keypoint pipeline of features.hip (score, maxima, cap, orientation, descriptor) as two
// queued halves with caller-owned buffers, so that one call can run it on more than one image: srrg2_adapt_image_features writes
// straight into its scene, srrg2_adapt_stereo_features (stereo.hip) into per-call buffers, twice.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "scene_state.h"

namespace srrg2amd {

enum { FEAT_MARGIN = 16 };
// counters block of one image (ints): [0] candidates, [1] maxima, [2] selected, [3] s*, [4] ties kept, [5] ties seen (the tie
// scan's total), [6] free for the caller (stereo.hip: the keep scan's total); the score histogram of the keypoints behind them
enum { FEAT_C_CANDIDATES = 0, FEAT_C_MAXIMA = 1, FEAT_C_SELECTED = 2, FEAT_C_CUT = 3, FEAT_C_QUOTA = 4, FEAT_C_TIES = 5,
       FEAT_C_KEPT = 6, FEAT_C_HIST = 16, FEAT_C_WORDS = FEAT_C_HIST + 256 };

struct FeatImage {
  const unsigned char* p;
  long long stride;  // bytes per row
  int rows, cols;
};

// the keypoint's own depth pixel and the pinhole model (the arithmetic of DepthSource in adaptor.hip, expression for expression)
struct FeatDepth {
  const unsigned char* p;  // null: no depth image, z = 1
  long long stride;
  int f32;  // F32 metres (else U16 counts)
  float ifx, ify, cx, cy, scale, zmin, zmax;

  __device__ __forceinline__ bool depth_at(int r, int c, float& z) const {
    if (!p) {
      z = 1.f;
      return true;
    }
    const unsigned char* at = p + (long long) r * stride;
    if (f32) {
      z = reinterpret_cast<const float*>(at)[c];
    } else {
      const uint16_t raw = reinterpret_cast<const uint16_t*>(at)[c];
      if (raw == (uint16_t) 0) return false;
      z = (float) raw * scale;
    }
    return isfinite(z) && zmin <= z && z <= zmax;
  }
  __device__ __forceinline__ float3 point_at(int r, int c, float z) const {
    return make_float3((((float) c - cx) * ifx) * z, (((float) r - cy) * ify) * z, z);
  }
};

// one image's scratch: score / box of feat_padded_pixels(rows, cols) elements, is_max of n = rows * cols, tie and flags of
// n + 1, ctr of FEAT_C_WORDS, scan_sums of scan_num_blocks(n) + 2
struct FeatWork {
  unsigned char* score;
  unsigned short* box;
  unsigned char* is_max;
  int* tie;
  int* ctr;
  int* flags;
  int* scan_sums;
};

// what the describe half writes per kept keypoint k: gidx (pixel), desc (4 words) and kps always; pts / nrm / inten when not null
struct FeatOut {
  int* gidx;
  unsigned long long* desc;
  srrg2_keypoint* kps;
  float4* pts;
  float4* nrm;
  float* inten;
};

// the refusals that depend on the camera, the feature parameters and the capacity alone (0, or the error code with the text set)
int feat_check_params(const std::string& who, const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* p,
                      int keypoint_capacity);
// dst becomes an empty feature scene (arrays for one point, as the adaptors leave them)
int feat_empty_scene(srrg2_scene* s);
size_t feat_padded_pixels(int rows, int cols);
// the 32 rotated patterns in s->feat_pattern, uploaded once per scene (waits for the upload the first time)
int feat_pattern_upload(srrg2_scene* s);
// queues counters reset, score + box, maxima, cut, ties and select: w.flags[0 .. n) = keep flag per pixel (cap, then D's gate)
int feat_queue_select(const FeatImage& I, const FeatDepth& D, int fast_threshold, int max_features, const FeatWork& w, hipStream_t st);
// w.flags holds the exclusive scan of the keep flags and `total` its sum (> 0): queues the scatter of the kept pixels and their
// description
int feat_queue_describe(const FeatImage& I, const FeatDepth& D, int oriented, const FeatWork& w, const unsigned* pattern, int total,
                        const FeatOut& o, hipStream_t st);

}  // namespace srrg2amd
