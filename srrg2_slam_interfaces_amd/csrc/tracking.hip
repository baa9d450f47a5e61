// tracking.hip -- srrg2_scene_track_features: which keypoint of the measurement is which landmark of the clipped local map, on
// the device.  The reference declares this slot and leaves it empty (CorrespondenceFinder_::compute() is pure virtual,
// S/registration/correspondence_finder.h:56); DESIGN.md section 4 "Feature tracking" is the contract and
// tests/tracking_restatement.py its executable form.  The projection is that of srrg2_scene_clip_projective, operation for
// operation, in float32; everything behind it is integer arithmetic: the result is a function of the two scenes, the pose and the
// parameters alone, bit for bit.
//   k_track_project   one thread per landmark: its pixel rv * cols + cu, or -1 when it is not in view
//   (the keypoints' row table, which checks that their pixels ascend strictly inside the image and raises the error word
//   otherwise, then the banded descriptor search of desc_band.hip with the runner-up's distance and, with the cross check, the
//   reverse atomicMin table: srrg2amd::launch_band_rows, launch_band_search -- the column gate is [-R, R])
//   (`fixed` a pyramid scene of several levels -- level-major, its pixels ascend inside a level only: row table and search once per
//   level on the level's slice of the keypoints, then)
//   k_track_merge    one thread per landmark: the levels' (best, runner-up) pairs -> those of all keypoints, the keypoint index
//                     made global; the same merge the search runs across its lanes, so the result is that of one search
//   k_track_resolve  one thread per landmark: the gates, the cross check, the record and the keep flag; the four counters are
//                     block sums with one atomic per block and counter
//   (exclusive scan of the keep flags: srrg2amd::launch_exclusive_scan, what srrg2amd::scene_scan_flags runs -- its total rides
//   on the call's one wait)
//   k_track_scatter   kept landmark -> its slot of the capacity-bounded output, behind the counters in one block
// No launch is capped: every kernel has one thread (or wave) per element and no loop behind a cap.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "device_util.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_state.h"

using srrg2amd::fail;

namespace {

// words of the output block (srrg2_scene::trk_out): the counters, the error word, the scan's total; the records from T_WORDS on
enum { T_IN_VIEW = 0, T_CANDIDATE = 1, T_ACCEPTED = 2, T_MUTUAL = 3, T_ERROR = 4, T_TOTAL = 5, T_WORDS = 8 };
using srrg2amd::NO_CANDIDATE;
using srrg2amd::NO_SECOND;

struct TrackCam {
  float m[12];  // rows of moving_in_sensor
  float K0, K2, K4, K5, depth_min, depth_max;
  int rows, cols;
};

// the non-empty levels of a pyramid scene as `fixed`: level s holds keypoints offset[s] .. offset[s + 1]
struct TrackLevels {
  int n;
  int offset[9];
};

// best_level / second_level: per level s and landmark q (at s * nm + q) what the banded search found among that level's keypoints,
// the index counted inside the level.  Disjoint candidate sets: the smaller key wins, the loser's distance is a distance of
// "another candidate" as both runner-ups are (merge_best of desc_band.hip).
__global__ __launch_bounds__(256) void k_track_merge(int nm, TrackLevels L, const unsigned long long* __restrict__ best_level,
                                                     const unsigned* __restrict__ second_level, unsigned long long* __restrict__ best,
                                                     unsigned* __restrict__ second) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nm) return;
  unsigned long long key = NO_CANDIDATE;
  unsigned sec           = NO_SECOND;
  for (int s = 0; s < L.n; ++s) {
    unsigned long long k = best_level[(size_t) s * nm + q];
    if (k != NO_CANDIDATE) k += (unsigned) L.offset[s];  // (index + offset < the scene's size: no carry into the distance)
    sec = min(min(sec, second_level[(size_t) s * nm + q]), (unsigned) ((k < key ? key : k) >> 32));
    key = k < key ? k : key;
  }
  best[q]   = key;
  second[q] = sec;
}

// srrg2_scene_clip_projective's steps behind its two transforms (scene.hip pclip_project): the same operations in the same order
__global__ __launch_bounds__(256) void k_track_project(TrackCam C, const float4* __restrict__ pts, int n, int* __restrict__ pix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int out = -1;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const float cx = ((C.m[0] * p.x + C.m[1] * p.y) + C.m[2] * p.z) + C.m[3];
    const float cy = ((C.m[4] * p.x + C.m[5] * p.y) + C.m[6] * p.z) + C.m[7];
    const float cz = ((C.m[8] * p.x + C.m[9] * p.y) + C.m[10] * p.z) + C.m[11];
    if (isfinite(cx) && isfinite(cy) && isfinite(cz) && cz >= C.depth_min && cz <= C.depth_max) {
      const float u  = (C.K0 * cx) / cz + C.K2;
      const float v  = (C.K4 * cy) / cz + C.K5;
      const float uf = u + 0.5f, vf = v + 0.5f;
      if (uf >= 0.f && uf < (float) C.cols && vf >= 0.f && vf < (float) C.rows) out = (int) floorf(vf) * C.cols + (int) floorf(uf);
    }
  }
  pix[i] = out;
}

// One thread per landmark; cross = 0: best_fixed is not read.  counters: the output block's first words.
__global__ __launch_bounds__(256) void k_track_resolve(int nm, const int* __restrict__ m_pix, const unsigned long long* __restrict__ best,
                                                       const unsigned* __restrict__ second,
                                                       const unsigned long long* __restrict__ best_fixed, int max_distance,
                                                       int min_margin, int cross, srrg2_correspondence* __restrict__ rec,
                                                       int* __restrict__ flags, int* __restrict__ counters) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int in_view = 0, candidate = 0, accepted = 0, mutual = 0;
  if (i < nm && counters[T_ERROR] == 0) {
    in_view                    = m_pix[i] >= 0 ? 1 : 0;
    const unsigned long long k = best[i];
    const unsigned h = (unsigned) (k >> 32), s = second[i];
    const int j = (int) (unsigned) (k & 0xffffffffull);
    candidate   = k != NO_CANDIDATE ? 1 : 0;
    accepted    = candidate && (int) h <= max_distance && (min_margin == 0 || s == NO_SECOND || (int) (s - h) >= min_margin) ? 1 : 0;
    mutual      = accepted && (!cross || (int) (unsigned) (best_fixed[j] & 0xffffffffull) == i) ? 1 : 0;
    srrg2_correspondence c;
    c.fixed_idx = mutual ? j : -1, c.moving_idx = i, c.response = mutual ? (float) h : 0.f;
    rec[i] = c;
  }
  if (i < nm) flags[i] = mutual;
  block_add(in_view, &counters[T_IN_VIEW]);
  block_add(candidate, &counters[T_CANDIDATE]);
  block_add(accepted, &counters[T_ACCEPTED]);
  block_add(mutual, &counters[T_MUTUAL]);
}

// offset: the exclusive scan of the keep flags (nm + 1 words); out holds cap records
__global__ __launch_bounds__(256) void k_track_scatter(int nm, const int* __restrict__ offset, const srrg2_correspondence* __restrict__ rec,
                                                       srrg2_correspondence* __restrict__ out, int cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nm) return;
  const int k = offset[i];
  if (offset[i + 1] == k || k < 0 || k >= cap) return;
  out[k] = rec[i];
}

unsigned blocks_of(long long threads) { return (unsigned) ((threads + 255) / 256); }

}  // namespace

extern "C" void srrg2_track_default_params(srrg2_track_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->depth_min     = 0.4f;  // (the projective clipper's interval)
  p->depth_max     = 8.f;
  p->search_radius = 16;  // untuned
  p->max_distance  = 48;  // untuned, as the stereo matcher's
  p->min_margin    = 0;
  p->cross_check   = 1;
}

extern "C" int srrg2_scene_track_features(srrg2_scene_h moving, srrg2_scene_h fixed, const float* moving_in_sensor,
                                          const srrg2_track_params* p, srrg2_correspondence* correspondences_out, int capacity,
                                          srrg2_track_result* out) {
  const std::string who = "scene_track_features: ";
  if (!moving || !fixed || !moving_in_sensor || !p) return fail(SRRG2_E_INVALID, who + "null scene, pose or params");
  if (moving == fixed || moving->device != fixed->device)
    return fail(SRRG2_E_INVALID, who + "moving and fixed must be two scenes on one device");
  if (moving->dim != 3 || fixed->dim != 3) return fail(SRRG2_E_INVALID, who + "both scenes must have dim 3");
  if (p->image_rows <= 0 || p->image_cols <= 0 || (long long) p->image_rows * (long long) p->image_cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, who + "image_rows, image_cols > 0 and rows*cols within int32");
  const float fx = p->camera_matrix[0], fy = p->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, who + "fx and fy must be finite and non-zero");
  if (!(p->depth_min > 0.f) || !(p->depth_max >= p->depth_min)) return fail(SRRG2_E_INVALID, who + "0 < depth_min <= depth_max");
  if (p->search_radius < 0 || p->search_radius > 255) return fail(SRRG2_E_INVALID, who + "search_radius 0 .. 255");
  if (p->max_distance < 0 || p->max_distance > 256) return fail(SRRG2_E_INVALID, who + "max_distance 0 .. 256");
  if (p->min_margin < 0 || p->min_margin > 256) return fail(SRRG2_E_INVALID, who + "min_margin 0 .. 256");
  if (p->cross_check != 0 && p->cross_check != 1) return fail(SRRG2_E_INVALID, who + "cross_check must be 0 or 1");
  if (p->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  if (capacity < 0) return fail(SRRG2_E_INVALID, who + "capacity >= 0");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(moving_in_sensor[k])) return fail(SRRG2_E_INVALID, who + "moving_in_sensor is not finite");
  if (p->camera_matrix[1] != 0.f) return fail(SRRG2_E_UNSUPPORTED, who + "a camera matrix with skew (K[0][1] != 0)");
  srrg2_scene* const s = moving;
  HIP_TRY(hipSetDevice(s->device));
  for (srrg2_scene* q : {moving, fixed})
    if (q->pending) {  // an adaptor's queued write
      HIP_TRY(hipStreamSynchronize(q->stream));
      q->pending = false;
    }
  const int nm = moving->n, nf = fixed->n;
  if ((nm > 0 && !moving->has_desc) || (nf > 0 && !fixed->has_desc)) return fail(SRRG2_E_STATE, who + "a scene without descriptors");
  if (nf > 0 && fixed->ng != nf)
    return fail(SRRG2_E_STATE, who + "the fixed scene has no global indices (an adaptor's or a clipper's output has)");
  srrg2_track_result res;
  std::memset(&res, 0, sizeof(res));
  res.num_moving = nm, res.num_fixed = nf;
  if (nm == 0) {  // nothing to project: the device is not asked (fixed's pixels stay unchecked)
    if (out) *out = res;
    return 0;
  }

  int rc;
  hipStream_t st = s->stream;
  const int rows = p->image_rows, cols = p->image_cols;
  const int cap       = capacity < nm ? capacity : nm;  // (records the output block has room for)
  const size_t words  = (size_t) T_WORDS + 3 * (size_t) cap;
  static_assert(sizeof(srrg2_correspondence) == 12, "three words per record");
  if ((rc = s->trk_pix.reserve((size_t) nm)) || (rc = s->trk_best.reserve((size_t) nm)) || (rc = s->trk_second.reserve((size_t) nm)) ||
      (rc = s->trk_rec.reserve((size_t) nm)) || (rc = s->trk_rows.reserve((size_t) rows + 1)) ||
      (rc = s->trk_best_fixed.reserve((size_t) nf + 1)) || (rc = s->trk_out.reserve(words)) ||
      (rc = s->flags.reserve((size_t) nm + 1)) || (rc = s->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(nm) + 2)))
    return rc;
  if ((rc = s->trk_host.reserve(words, words / 8 + 64))) return rc;
  // `fixed` written by srrg2_adapt_image_features_pyramid and untouched since: its non-empty levels
  TrackLevels levels;
  std::memset(&levels, 0, sizeof(levels));
  if (fixed->pyr_levels > 1 && fixed->pyr_offset[fixed->pyr_levels] == nf)
    for (int l = 0; l < fixed->pyr_levels; ++l)
      if (fixed->pyr_offset[l + 1] > fixed->pyr_offset[l]) {
        levels.offset[levels.n]     = fixed->pyr_offset[l];
        levels.offset[++levels.n]   = fixed->pyr_offset[l + 1];
      }
  if (levels.n > 1 && ((rc = s->trk_rows.reserve((size_t) levels.n * ((size_t) rows + 1))) ||
                       (rc = s->trk_best_level.reserve((size_t) levels.n * nm)) || (rc = s->trk_second_level.reserve((size_t) levels.n * nm))))
    return rc;
  TrackCam C;
  std::memcpy(C.m, moving_in_sensor, sizeof(C.m));
  C.K0 = fx, C.K2 = p->camera_matrix[2], C.K4 = fy, C.K5 = p->camera_matrix[5];
  C.depth_min = p->depth_min, C.depth_max = p->depth_max;
  C.rows = rows, C.cols = cols;
  int* const block                   = s->trk_out.p;
  srrg2_correspondence* const d_recs = reinterpret_cast<srrg2_correspondence*>(block + T_WORDS);
  unsigned long long* const reverse  = p->cross_check ? s->trk_best_fixed.p : nullptr;

  HIP_TRY(hipMemsetAsync(block, 0, T_WORDS * sizeof(int), st));
  if (reverse) HIP_TRY(hipMemsetAsync(reverse, 0xff, sizeof(unsigned long long) * (size_t) (nf + 1), st));
  hipLaunchKernelGGL(k_track_project, dim3(blocks_of(nm)), dim3(256), 0, st, C, moving->pts.p, nm, s->trk_pix.p);
  if (levels.n <= 1) {
    srrg2amd::launch_band_rows(fixed->gidx.p, nf, rows, cols, s->trk_rows.p, block + T_ERROR, st);
    srrg2amd::launch_band_search(nm, s->trk_pix.p, moving->desc.p, fixed->gidx.p, fixed->desc.p, s->trk_rows.p, rows, cols,
                                 p->search_radius, -p->search_radius, p->search_radius, block + T_ERROR, s->trk_best.p,
                                 s->trk_second.p, reverse, st);
  } else {  // a pyramid scene: level by level (the pixels must ascend strictly inside every level), then one merge
    for (int l = 0; l < levels.n; ++l) {
      const int at = levels.offset[l], count = levels.offset[l + 1] - at;
      int* const table = s->trk_rows.p + (size_t) l * ((size_t) rows + 1);
      srrg2amd::launch_band_rows(fixed->gidx.p + at, count, rows, cols, table, block + T_ERROR, st);
      srrg2amd::launch_band_search(nm, s->trk_pix.p, moving->desc.p, fixed->gidx.p + at, fixed->desc.p + 2 * (size_t) at, table, rows, cols,
                                   p->search_radius, -p->search_radius, p->search_radius, block + T_ERROR,
                                   s->trk_best_level.p + (size_t) l * nm, s->trk_second_level.p + (size_t) l * nm,
                                   reverse ? reverse + at : nullptr, st);
    }
    hipLaunchKernelGGL(k_track_merge, dim3(blocks_of(nm)), dim3(256), 0, st, nm, levels, s->trk_best_level.p, s->trk_second_level.p,
                       s->trk_best.p, s->trk_second.p);
  }
  hipLaunchKernelGGL(k_track_resolve, dim3(blocks_of(nm)), dim3(256), 0, st, nm, s->trk_pix.p, s->trk_best.p, s->trk_second.p, reverse,
                     p->max_distance, p->min_margin, p->cross_check, s->trk_rec.p, s->flags.p, block);
  srrg2amd::launch_exclusive_scan(s->flags.p, nm, s->scan_sums.p, block + T_TOTAL, st);
  if (cap > 0) hipLaunchKernelGGL(k_track_scatter, dim3(blocks_of(nm)), dim3(256), 0, st, nm, s->flags.p, s->trk_rec.p, d_recs, cap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->trk_host.p, block, words * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the call's one host wait: counters, error word, total and records together

  const int* const h = s->trk_host.p;
  if (h[T_ERROR])
    return fail(SRRG2_E_INVALID, who + "the fixed scene's global indices must ascend strictly inside [0, rows*cols)");
  const int total = h[T_TOTAL];
  if (total < 0 || total > nm || total != h[T_MUTUAL]) return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
  const int give = correspondences_out ? (total < cap ? total : cap) : 0;
  if (give > 0) std::memcpy(correspondences_out, h + T_WORDS, sizeof(srrg2_correspondence) * (size_t) give);
  res.num_in_view         = h[T_IN_VIEW];
  res.num_with_candidate  = h[T_CANDIDATE];
  res.num_accepted        = h[T_ACCEPTED];
  res.num_mutual          = h[T_MUTUAL];
  res.num_correspondences = total;
  if (out) *out = res;
  return 0;
}
