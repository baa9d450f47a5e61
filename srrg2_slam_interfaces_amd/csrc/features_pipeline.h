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

// Where level l of a scale pyramid (pyramid.hip) sits over level 0: a level pixel's centre lies at (2c+1) num / (2 den) - 1/2 level-0
// pixels, num = scale_num^l, den = scale_den^l.  The depth gate and the point are taken there; the identity map (level 0) gives
// 256 c, c and the arithmetic of the single-scale extractor, bit for bit.
struct FeatLevel {
  long long num, den;
  int rows0, cols0;  // level 0's size
  int level;
  int keep_none;  // the level's quota under the cap is 0: nothing is selected (inside the cap proper, 0 means "no cap")

  __device__ __forceinline__ int q8(int c) const { return (int) (((long long) (2 * c + 1) * num * 128) / den - 128); }
  __device__ __forceinline__ static int nearest(int q8, int size0) { return min((q8 + 128) >> 8, size0 - 1); }
  // FeatDepth::point_at with u = u_q8 / 256 in place of (float) c
  __device__ __forceinline__ static float3 point_at(const FeatDepth& D, int u_q8, int v_q8, float z) {
    const float u = (float) u_q8 * (1.0f / 256.0f), v = (float) v_q8 * (1.0f / 256.0f);
    return make_float3(((u - D.cx) * D.ifx) * z, ((v - D.cy) * D.ify) * z, z);
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
// every refusal of srrg2_adapt_image_features, in its order (0, or the error code with the text set)
int feat_check_images(const std::string& who, srrg2_scene* dst, const void* intensity, int intensity_type, int intensity_stride,
                      const void* depth, int depth_type, int depth_stride, int mem, const srrg2_depth_adaptor_params* cam,
                      const srrg2_feature_params* p, int keypoint_capacity);
// the views of the checked images and camera; SRRG2_MEM_HOST images are copied into s->staging, queued on s->stream
int feat_stage_images(srrg2_scene* s, const void* intensity, int intensity_stride, const void* depth, int depth_type, int depth_stride,
                      int mem, const srrg2_depth_adaptor_params* cam, FeatImage* image, FeatDepth* view);
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
// The same two halves on level L of a pyramid.  select: the depth gate reads D at the keypoint's nearest level-0 pixel.  describe:
// the kept LEVEL pixels go to lpix[0 .. total), o.gidx takes the nearest level-0 pixel, o.pts the point at the level-0 position,
// rec the pyramid records; o.kps is not written
int feat_queue_select_level(const FeatImage& I, const FeatDepth& D, const FeatLevel& L, int fast_threshold, int max_features,
                            const FeatWork& w, hipStream_t st);
int feat_queue_describe_level(const FeatImage& I, const FeatDepth& D, const FeatLevel& L, int oriented, const FeatWork& w,
                              const unsigned* pattern, int total, int* lpix, const FeatOut& o, srrg2_pyramid_keypoint* rec,
                              hipStream_t st);

}  // namespace srrg2amd
