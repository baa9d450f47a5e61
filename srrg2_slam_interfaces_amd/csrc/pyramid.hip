// pyramid.hip -- srrg2_adapt_image_features_pyramid: the keypoint pipeline of features.hip on every level of an integer-resampled
// scale pyramid of the image, into ONE feature scene (level-major).  No reference counterpart; DESIGN.md section 4 "Image
// features: scale pyramid" is the contract and tests/pyramid_restatement.py its executable form.  All image arithmetic is
// integer: the result is a function of the pixels and the parameters alone, bit for bit.
//   k_pyr_downscale   one 64 x 16 destination tile per workgroup; its source footprint (at most 129 x 33 pixels at a ratio <= 2,
//                      clamped at the borders) is read ONCE into LDS; a thread owns 4 adjacent destination pixels and writes them
//                      as one word.  Destination pitch: a multiple of 4, so the next level's k_feat_score_box reads words.
//   (per level: the pipeline of features.hip through features_pipeline.h with the level's map -- every level's select half and
//   keep-flag scan is queued before the call's ONE host wait; the kept counts place the levels in dst, then every level's describe
//   half writes its slice of the scene)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "features_pipeline.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_state.h"

using srrg2amd::fail;
using srrg2amd::FeatDepth;
using srrg2amd::FeatImage;
using srrg2amd::FeatLevel;

namespace {

enum { MAX_LEVELS = 8, TILE_W = 64, TILE_H = 16, SRC_W = 2 * TILE_W + 4, SRC_H = 2 * TILE_H + 4, MAX_SIDE = 1 << 22 };

// source coordinate of destination index i in 1/256 pixel: ((2i+1) num 256) / (2 den) - 128 >= 0 (num > den)
__device__ __forceinline__ int source_q8(int i, int num, int den) {
  return (int) (((long long) (2 * i + 1) * num * 256) / (2 * den)) - 128;
}

// dst: rows x cols at `pitch` (a multiple of 4; the pad columns of a row are written too, as 0)
__global__ __launch_bounds__(256) void k_pyr_downscale(FeatImage S, int num, int den, unsigned char* __restrict__ dst, int rows,
                                                       int cols, int pitch) {
  __shared__ unsigned char src[SRC_H * SRC_W];
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;
  // the tile's footprint: source columns x_lo .. x_lo + w - 1 and rows y_lo .. y_lo + h - 1, before the clamp
  const int c_last = min(c0 + TILE_W, cols) - 1, r_last = min(r0 + TILE_H, rows) - 1;
  const int x_lo = source_q8(c0, num, den) >> 8, y_lo = source_q8(r0, num, den) >> 8;
  const int w = min((source_q8(c_last, num, den) >> 8) + 2 - x_lo, (int) SRC_W);  // (<= 129 at num <= 2 den: the min never cuts)
  const int h = min((source_q8(r_last, num, den) >> 8) + 2 - y_lo, (int) SRC_H);  // (<= 33)
  for (int i = threadIdx.x; i < w * h; i += blockDim.x) {
    const int ly = i / w, lx = i - ly * w;
    const int y = min(y_lo + ly, S.rows - 1), x = min(x_lo + lx, S.cols - 1);
    src[ly * SRC_W + lx] = S.p[(long long) y * S.stride + x];
  }
  __syncthreads();
  const int r = r0 + (threadIdx.x >> 4), c = c0 + (threadIdx.x & 15) * 4;  // the thread's pixels: (r, c .. c + 3)
  if (r >= rows || c >= pitch) return;
  const int Y  = source_q8(r, num, den);
  const int ly = (Y >> 8) - y_lo, fy = Y & 255;
  unsigned word = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (c + q >= cols) break;
    const int X  = source_q8(c + q, num, den);
    const int lx = (X >> 8) - x_lo, fx = X & 255;
    const unsigned char* at = src + ly * SRC_W + lx;  // (lx + 1 < w, ly + 1 < h: the footprint holds x1 and y1 before their clamp)
    const unsigned v = ((unsigned) at[0] * (256 - fx) * (256 - fy) + (unsigned) at[1] * fx * (256 - fy) +
                        (unsigned) at[SRC_W] * (256 - fx) * fy + (unsigned) at[SRC_W + 1] * fx * fy + 32768u) >> 16;
    word |= v << (8 * q);
  }
  *reinterpret_cast<unsigned*>(dst + (size_t) r * pitch + c) = word;
}

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// one level: its image size, its slices of the scratch blocks (element offsets) and its quota
struct Level {
  int rows, cols, n, pitch;
  size_t img, padded, max, tie, sums;
  int quota;
};

}  // namespace

extern "C" void srrg2_adapt_default_pyramid_params(srrg2_pyramid_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->num_levels = 4;
  p->scale_num  = 6;
  p->scale_den  = 5;
}

extern "C" int srrg2_adapt_image_features_pyramid(srrg2_scene_h dst, const void* intensity, int intensity_type, int intensity_stride,
                                                  const void* depth, int depth_type, int depth_stride, int mem,
                                                  const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* p,
                                                  const srrg2_pyramid_params* pyr, srrg2_pyramid_keypoint* keypoints_out,
                                                  int keypoint_capacity, srrg2_pyramid_result* out) {
  const std::string who = "adapt_image_features_pyramid: ";
  int rc;
  if ((rc = srrg2amd::feat_check_images(who, dst, intensity, intensity_type, intensity_stride, depth, depth_type, depth_stride, mem,
                                        cam, p, keypoint_capacity)))
    return rc;
  if (!pyr) return fail(SRRG2_E_INVALID, who + "null pyramid params");
  if (pyr->num_levels < 1 || pyr->num_levels > MAX_LEVELS) return fail(SRRG2_E_INVALID, who + "num_levels 1 .. 8");
  const int num = pyr->scale_num, den = pyr->scale_den;
  if (den < 1 || den >= num || num > 2 * den || num > 8) return fail(SRRG2_E_INVALID, who + "1 <= scale_den < scale_num <= 2 scale_den, scale_num <= 8");
  if (pyr->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  if (cam->rows > MAX_SIDE || cam->cols > MAX_SIDE) return fail(SRRG2_E_UNSUPPORTED, who + "rows or cols above 4194304");
  srrg2_scene* const s = dst;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  if (s->pending) {  // an adaptor's queued write
    HIP_TRY(hipStreamSynchronize(st));
    s->pending = false;
  }
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status = cam->rows * cam->cols == 0 ? SRRG2_ADAPTOR_INITIALIZING : SRRG2_ADAPTOR_READY;
  }
  // the levels that are built, their slices and quotas
  Level lv[MAX_LEVELS];
  int nb = 0;
  size_t img_bytes = 0, padded = 0, maxes = 0, ties = 0, sums = 0;
  long long area = 0;
  for (int l = 0, rows = cam->rows, cols = cam->cols; l < pyr->num_levels; ++l, rows = rows * den / num, cols = cols * den / num) {
    if (rows <= 2 * srrg2amd::FEAT_MARGIN || cols <= 2 * srrg2amd::FEAT_MARGIN) break;  // no pixel 16 away from every border
    Level& L = lv[nb++];
    L.rows = rows, L.cols = cols, L.n = rows * cols, L.pitch = (cols + 3) / 4 * 4;
    L.img = img_bytes, L.padded = padded, L.max = maxes, L.tie = ties, L.sums = sums;
    if (l > 0) img_bytes += round_up((size_t) L.pitch * (size_t) rows, 64);
    padded += srrg2amd::feat_padded_pixels(rows, cols);
    maxes += round_up((size_t) L.n, 64);
    ties += round_up((size_t) L.n + 1, 64);
    sums += round_up((size_t) srrg2amd::scan_num_blocks(L.n) + 2, 16);
    area += L.n;
  }
  if (nb == 0) return srrg2amd::feat_empty_scene(s);
  long long handed = 0;
  for (int l = 0; l < nb; ++l) handed += lv[l].quota = (int) ((long long) p->max_features * lv[l].n / area);
  lv[0].quota += (int) (p->max_features - handed);

  FeatImage I[MAX_LEVELS];
  FeatDepth D;
  if ((rc = srrg2amd::feat_stage_images(s, intensity, intensity_stride, depth, depth_type, depth_stride, mem, cam, &I[0], &D))) return rc;
  if ((rc = s->pyr_img.reserve(img_bytes + 64)) || (rc = s->pyr_score.reserve(padded)) || (rc = s->pyr_box.reserve(padded)) ||
      (rc = s->pyr_max.reserve(maxes)) || (rc = s->pyr_tie.reserve(ties)) || (rc = s->pyr_flags.reserve(ties)) ||
      (rc = s->pyr_sums.reserve(sums)) || (rc = s->pyr_ctr.reserve((size_t) nb * srrg2amd::FEAT_C_WORDS)) ||
      (rc = s->pyr_host.reserve(8 * MAX_LEVELS)))
    return rc;
  if ((rc = srrg2amd::feat_pattern_upload(s))) return rc;  // the 32 rotated patterns, once per scene
  srrg2amd::FeatWork work[MAX_LEVELS];
  FeatLevel map[MAX_LEVELS];
  long long num_l = 1, den_l = 1;
  for (int l = 0; l < nb; ++l, num_l *= num, den_l *= den) {  // every level up to its kept count, behind one wait
    const Level& L = lv[l];
    if (l > 0) {
      I[l] = FeatImage{s->pyr_img.p + L.img, (long long) L.pitch, L.rows, L.cols};
      hipLaunchKernelGGL(k_pyr_downscale, dim3((L.pitch + TILE_W - 1) / TILE_W, (L.rows + TILE_H - 1) / TILE_H), dim3(256), 0, st, I[l - 1],
                         num, den, s->pyr_img.p + L.img, L.rows, L.cols, L.pitch);
    }
    work[l] = srrg2amd::FeatWork{s->pyr_score.p + L.padded, s->pyr_box.p + L.padded, s->pyr_max.p + L.max, s->pyr_tie.p + L.tie,
                                 s->pyr_ctr.p + (size_t) l * srrg2amd::FEAT_C_WORDS, s->pyr_flags.p + L.tie, s->pyr_sums.p + L.sums};
    map[l] = FeatLevel{num_l, den_l, cam->rows, cam->cols, l, p->max_features > 0 && L.quota == 0 ? 1 : 0};
    if ((rc = srrg2amd::feat_queue_select_level(I[l], D, map[l], p->fast_threshold, L.quota, work[l], st))) return rc;
    srrg2amd::launch_exclusive_scan(work[l].flags, L.n, work[l].scan_sums, work[l].ctr + srrg2amd::FEAT_C_KEPT, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->pyr_host.p + 8 * l, work[l].ctr, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  int offset[MAX_LEVELS + 1] = {0};
  for (int l = 0; l < nb; ++l) {
    const int kept = s->pyr_host.p[8 * l + srrg2amd::FEAT_C_KEPT];
    if (kept < 0 || kept > lv[l].n || (long long) offset[l] + kept > 0x7fffffffLL)
      return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
    offset[l + 1] = offset[l] + kept;
  }
  const int total = offset[nb];
  // the content is replaced from here on
  const size_t room = (size_t) (total > 0 ? total : 1);
  s->has_desc = s->has_inten = true;
  if ((rc = srrg2amd::scene_make_room(s, (int) room, 0))) return rc;
  if ((rc = s->gidx.reserve(room)) || (rc = s->pyr_lpix.reserve(room)) || (rc = s->pyr_kp.reserve(room))) return rc;
  s->n = s->ng = total;
  s->has_normals = false;
  s->pyr_levels  = nb;  // (for the tracker: where each level's keypoints lie)
  for (int l = 0; l <= MAX_LEVELS; ++l) s->pyr_offset[l] = offset[l < nb ? l : nb];
  if (total > 0) {
    for (int l = 0; l < nb; ++l) {
      const int kept = offset[l + 1] - offset[l], at = offset[l];
      if (kept == 0) continue;
      const srrg2amd::FeatOut o{s->gidx.p + at, reinterpret_cast<unsigned long long*>(s->desc.p) + (size_t) at * 4, nullptr, s->pts.p + at,
                                s->nrm.p + at, s->inten.p + at};
      if ((rc = srrg2amd::feat_queue_describe_level(I[l], D, map[l], p->oriented, work[l], s->feat_pattern.p, kept, s->pyr_lpix.p + at, o,
                                                    s->pyr_kp.p + at, st)))
        return rc;
    }
    const int copied = keypoints_out ? (total < keypoint_capacity ? total : keypoint_capacity) : 0;
    if (copied > 0)
      HIP_TRY(hipMemcpyAsync(keypoints_out, s->pyr_kp.p, sizeof(srrg2_pyramid_keypoint) * (size_t) copied, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // dst, and the caller's images, are done with
  }
  if (out) {
    out->num_levels_built = nb;
    out->scene_size       = total;
    for (int l = 0; l < nb; ++l) {
      const int* const c     = s->pyr_host.p + 8 * l;
      out->rows[l]           = lv[l].rows;
      out->cols[l]           = lv[l].cols;
      out->num_candidates[l] = c[srrg2amd::FEAT_C_CANDIDATES];
      out->num_maxima[l]     = c[srrg2amd::FEAT_C_MAXIMA];
      out->num_selected[l]   = c[srrg2amd::FEAT_C_SELECTED];
      out->num_with_depth[l] = offset[l + 1] - offset[l];
      out->quota[l]          = lv[l].quota;
    }
  }
  return 0;
}
