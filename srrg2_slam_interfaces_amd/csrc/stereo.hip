// stereo.hip -- srrg2_adapt_stereo_features: a rectified pair of 8-bit images -> a compact scene of the left image's keypoints
// that found their partner in the right image, triangulated, with descriptor and intensity, on the device.  No reference
// counterpart (the reference's stereo pipeline, initializers/initializer_camera.h InitializerStereoCamera_, reads such clouds);
// DESIGN.md section 4 "Stereo features" is the contract and tests/stereo_restatement.py its executable form.  Matching and the
// sub-pixel costs are integer arithmetic, the depth is two float32 operations in a fixed order: the result is a function of the
// pixels and the parameters alone, bit for bit.
//   (per image: the pipeline of features.hip through features_pipeline.h -- both queued before the call's first host wait)
//   (per image the row table, then once per direction the banded descriptor search of desc_band.hip: srrg2amd::launch_band_rows,
//   launch_band_search -- the disparity gate is an interval on candidate column - query column)
//   k_stereo_resolve  one wave per left keypoint: distance gate, cross check, the three 7x7 costs (lane = window pixel, wave
//                      reduction); lane 0 computes the offset, the depth, its gate, the keep flag and the keypoint's record
//   k_stereo_count     num_matched and num_mutual from the records: grid-stride sums, two atomics per wave
//   (exclusive scan of the keep flags: srrg2amd::scene_scan_flags -- the second host wait)
//   k_stereo_scatter   kept left keypoint -> point, descriptor, intensity, global index and the two records of its slot
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "features_pipeline.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_device.h"
#include "scene_state.h"

using srrg2amd::fail;
using srrg2amd::FeatDepth;
using srrg2amd::FeatImage;

namespace {

enum { S_MATCHED = 0, S_MUTUAL = 1, S_WORDS = 2 };
using srrg2amd::NO_CANDIDATE;

// One wave per left keypoint (4 per workgroup).  best_r null: no cross check.  fb = fx * baseline.  Every read stays inside the
// images: a keypoint is >= 16 pixels from the borders, the window reaches 3 and the shifted one 4.
__global__ __launch_bounds__(256) void k_stereo_resolve(FeatImage L, FeatImage R, int nl, const int* __restrict__ l_pixel,
                                                        const int* __restrict__ r_pixel, const unsigned long long* __restrict__ best_l,
                                                        const unsigned long long* __restrict__ best_r, int max_distance, int subpixel,
                                                        float fb, float zmin, float zmax, srrg2_stereo_match* __restrict__ match,
                                                        float* __restrict__ depth, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int i    = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nl) return;  // (the whole wave)
  const unsigned long long k = best_l[i];
  const int h = (int) (k >> 32), j = (int) (unsigned) (k & 0xffffffffull);
  const bool matched = k != NO_CANDIDATE && h <= max_distance;  // (the same for every lane)
  const bool mutual  = matched && (!best_r || (int) (unsigned) (best_r[j] & 0xffffffffull) == i);
  const int pl = l_pixel[i];
  srrg2_stereo_match m;
  m.left_pixel = pl, m.right_pixel = -1, m.distance = matched ? h : -1, m.disparity = 0.f;  // (what k_stereo_count reads)
  float z  = 0.f;
  int keep = 0;
  if (mutual) {
    const int pr = r_pixel[j];
    const int r = pl / L.cols, cl = pl - r * L.cols, rr = pr / L.cols, cr = pr - rr * L.cols;
    int cm = 0, c0 = 0, cp = 0;  // cost(-1), cost(0), cost(1): <= 49 * 255
    if (subpixel) {
      if (lane < 49) {
        const int dy = lane / 7 - 3, dx = lane - (dy + 3) * 7 - 3;
        const int v = L.p[(long long) (r + dy) * L.stride + (cl + dx)];
        const unsigned char* row = R.p + (long long) (rr + dy) * R.stride + (cr + dx);
        cm = abs(v - (int) row[-1]), c0 = abs(v - (int) row[0]), cp = abs(v - (int) row[1]);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        cm += __shfl_xor(cm, off);
        c0 += __shfl_xor(c0, off);
        cp += __shfl_xor(cp, off);
      }
    }
    if (lane == 0) {
      float off   = 0.f;
      const int D = cm - 2 * c0 + cp;
      if (subpixel && c0 <= cm && c0 <= cp && D > 0) off = (float) (cm - cp) / (float) (2 * D);
      m.right_pixel = pr;
      m.disparity   = (float) (cl - cr) - off;
      z             = fb / m.disparity;
      keep          = isfinite(z) && zmin <= z && z <= zmax ? 1 : 0;
    }
  }
  if (lane == 0) {
    match[i] = m;
    depth[i] = z;
    flags[i] = keep;
  }
}

// the counters from the per-keypoint records (distance >= 0: matched, right_pixel >= 0: mutual): a grid-stride sum, reduced
// across the wave, two atomics per wave -- not three per keypoint on the same three words
__global__ __launch_bounds__(256) void k_stereo_count(const srrg2_stereo_match* __restrict__ match, int nl, int* __restrict__ counts) {
  int matched = 0, mutual = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x) {
    matched += match[i].distance >= 0 ? 1 : 0;
    mutual += match[i].right_pixel >= 0 ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    matched += __shfl_xor(matched, off);
    mutual += __shfl_xor(mutual, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (matched) atomicAdd(&counts[S_MATCHED], matched);
    if (mutual) atomicAdd(&counts[S_MUTUAL], mutual);
  }
}

// offset: the exclusive scan of the keep flags (nl + 1 words)
__global__ __launch_bounds__(256) void k_stereo_scatter(FeatImage L, FeatDepth D, int nl, const int* __restrict__ offset, int total,
                                                        const int* __restrict__ l_pixel, const srrg2_keypoint* __restrict__ l_kp,
                                                        const srrg2_stereo_match* __restrict__ match, const float* __restrict__ depth,
                                                        Feat f /* descriptors only */, float4* __restrict__ pts,
                                                        float4* __restrict__ nrm, float* __restrict__ inten, int* __restrict__ gidx, srrg2_keypoint* __restrict__ kps,
                                                        srrg2_stereo_match* __restrict__ matches) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x) {
    const int k = offset[i];
    if (offset[i + 1] == k || k < 0 || k >= total) continue;
    const int pixel = l_pixel[i];
    const int r = pixel / L.cols, c = pixel - r * L.cols;
    const float3 q = D.point_at(r, c, depth[i]);
    pts[k] = make_float4(q.x, q.y, q.z, 0.f);
    nrm[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    move_features(f, i, k);
    inten[k]   = (float) L.p[(long long) r * L.stride + c];
    gidx[k]    = pixel;
    kps[k]     = l_kp[i];
    matches[k] = match[i];
  }
}

}  // namespace

extern "C" void srrg2_adapt_default_stereo_params(srrg2_stereo_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_disparity = 1;
  p->max_disparity = 128;  // untuned
  p->row_tolerance = 1;
  p->max_distance  = 48;  // untuned
  p->cross_check   = 1;
  p->subpixel      = 1;
}

extern "C" int srrg2_adapt_stereo_features(srrg2_scene_h dst, const void* left, int left_stride, const void* right, int right_stride,
                                           int mem, const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* fp,
                                           const srrg2_stereo_params* sp, srrg2_keypoint* keypoints_out, int keypoint_capacity,
                                           srrg2_stereo_match* matches_out, int match_capacity, srrg2_stereo_result* out) {
  const std::string who = "adapt_stereo_features: ";
  int rc;
  if (!dst || !cam || !fp || !sp) return fail(SRRG2_E_INVALID, who + "null scene or params");
  if (dst->dim != 3) return fail(SRRG2_E_INVALID, who + "the scene must have dim 3");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if ((rc = srrg2amd::feat_check_params(who, cam, fp, keypoint_capacity))) return rc;
  if (match_capacity < 0) return fail(SRRG2_E_INVALID, who + "match_capacity >= 0");
  if (!std::isfinite(sp->baseline) || !(sp->baseline > 0.f)) return fail(SRRG2_E_INVALID, who + "baseline must be finite and > 0");
  if (sp->min_disparity < 1 || sp->max_disparity < sp->min_disparity)
    return fail(SRRG2_E_INVALID, who + "1 <= min_disparity <= max_disparity");
  if (sp->row_tolerance < 0 || sp->row_tolerance > 8) return fail(SRRG2_E_INVALID, who + "row_tolerance 0 .. 8");
  if (sp->max_distance < 0 || sp->max_distance > 256) return fail(SRRG2_E_INVALID, who + "max_distance 0 .. 256");
  if ((sp->cross_check != 0 && sp->cross_check != 1) || (sp->subpixel != 0 && sp->subpixel != 1))
    return fail(SRRG2_E_INVALID, who + "cross_check and subpixel must be 0 or 1");
  if (sp->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  const int rows = cam->rows, cols = cam->cols;
  const int n = rows * cols;
  if (n > 0) {
    if (!left || !right) return fail(SRRG2_E_INVALID, who + "null image");
    if ((long long) left_stride < (long long) cols || (long long) right_stride < (long long) cols)
      return fail(SRRG2_E_INVALID, who + "row stride smaller than a row");
  }
  srrg2_scene* const s = dst;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  if (s->pending) {  // an adaptor's queued write
    HIP_TRY(hipStreamSynchronize(st));
    s->pending = false;
  }
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status     = n == 0 ? SRRG2_ADAPTOR_INITIALIZING : SRRG2_ADAPTOR_READY;
    out->num_pixels = n;
  }
  if (rows <= 2 * srrg2amd::FEAT_MARGIN || cols <= 2 * srrg2amd::FEAT_MARGIN) return srrg2amd::feat_empty_scene(s);

  FeatImage I[2] = {{static_cast<const unsigned char*>(left), (long long) left_stride, rows, cols},
                    {static_cast<const unsigned char*>(right), (long long) right_stride, rows, cols}};
  FeatDepth D;  // no depth image: the pipelines keep every selected keypoint; the scatter uses the pinhole model
  std::memset(&D, 0, sizeof(D));
  const float fx = cam->camera_matrix[0], fy = cam->camera_matrix[4];
  D.ifx = 1.0f / fx, D.ify = 1.0f / fy;
  D.cx = cam->camera_matrix[2], D.cy = cam->camera_matrix[5];
  D.scale = cam->depth_scale, D.zmin = cam->depth_min, D.zmax = cam->depth_max;
  if (mem == SRRG2_MEM_HOST) {  // rows up to the last pixel of the last row, as they lie
    const size_t bl = (size_t) (rows - 1) * (size_t) left_stride + (size_t) cols;
    const size_t br = (size_t) (rows - 1) * (size_t) right_stride + (size_t) cols;
    const size_t off_r = (bl + 63) / 64 * 64;
    if ((rc = s->staging.reserve(off_r + br + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->staging.p, left, bl, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->staging.p + off_r, right, br, hipMemcpyHostToDevice, st));
    I[0].p = reinterpret_cast<const unsigned char*>(s->staging.p);
    I[1].p = reinterpret_cast<const unsigned char*>(s->staging.p + off_r);
  }
  const size_t padded = srrg2amd::feat_padded_pixels(rows, cols);
  const size_t sums   = (size_t) srrg2amd::scan_num_blocks(n) + 2;
  if ((rc = s->feat_score.reserve(padded)) || (rc = s->feat_box.reserve(padded)) || (rc = s->feat_max.reserve((size_t) n)) ||
      (rc = s->feat_tie.reserve((size_t) n + 1)) || (rc = s->feat_ctr.reserve(srrg2amd::FEAT_C_WORDS)) ||
      (rc = s->flags.reserve((size_t) n + 1)) || (rc = s->scan_sums.reserve(sums)))
    return rc;
  if ((rc = s->st_score.reserve(padded)) || (rc = s->st_box.reserve(padded)) || (rc = s->st_max.reserve((size_t) n)) ||
      (rc = s->st_tie.reserve((size_t) n + 1)) || (rc = s->st_ctr.reserve(srrg2amd::FEAT_C_WORDS)) ||
      (rc = s->st_flags.reserve((size_t) n + 1)) || (rc = s->st_sums.reserve(sums)) || (rc = s->st_counts.reserve(S_WORDS)))
    return rc;
  if ((rc = srrg2amd::feat_pattern_upload(s))) return rc;
  const srrg2amd::FeatWork work[2] = {
      {s->feat_score.p, s->feat_box.p, s->feat_max.p, s->feat_tie.p, s->feat_ctr.p, s->flags.p, s->scan_sums.p},
      {s->st_score.p, s->st_box.p, s->st_max.p, s->st_tie.p, s->st_ctr.p, s->st_flags.p, s->st_sums.p}};
  for (int e = 0; e < 2; ++e) {  // both pipelines, up to the keypoint count, behind one wait
    if ((rc = srrg2amd::feat_queue_select(I[e], D, fp->fast_threshold, fp->max_features, work[e], st))) return rc;
    srrg2amd::launch_exclusive_scan(work[e].flags, n, work[e].scan_sums, work[e].ctr + srrg2amd::FEAT_C_KEPT, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->scalars.p + 8 * e, work[e].ctr, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  const int count[2] = {s->scalars.p[srrg2amd::FEAT_C_KEPT], s->scalars.p[8 + srrg2amd::FEAT_C_KEPT]};
  if (count[0] < 0 || count[0] > n || count[1] < 0 || count[1] > n)
    return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
  if (out) out->num_left = count[0], out->num_right = count[1];
  if (count[0] == 0 || count[1] == 0) return srrg2amd::feat_empty_scene(s);  // nothing to match

  const int nl = count[0], nr = count[1];
  for (int e = 0; e < 2; ++e) {
    const size_t ne = (size_t) count[e];
    if ((rc = s->st_pixel[e].reserve(ne)) || (rc = s->st_desc[e].reserve(2 * ne)) || (rc = s->st_kp[e].reserve(ne)) ||
        (rc = s->st_rows[e].reserve((size_t) rows + 1)) || (rc = s->st_best[e].reserve(ne)))
      return rc;
  }
  if ((rc = s->st_match.reserve((size_t) nl)) || (rc = s->st_z.reserve((size_t) nl))) return rc;
  for (int e = 0; e < 2; ++e) {
    const srrg2amd::FeatOut o{s->st_pixel[e].p, reinterpret_cast<unsigned long long*>(s->st_desc[e].p), s->st_kp[e].p, nullptr, nullptr,
                              nullptr};
    if ((rc = srrg2amd::feat_queue_describe(I[e], D, fp->oriented, work[e], s->feat_pattern.p, count[e], o, st))) return rc;
    srrg2amd::launch_band_rows(s->st_pixel[e].p, count[e], rows, cols, s->st_rows[e].p, nullptr, st);  // (the extractor's pixels)
  }
  // the disparity d = left column - right column in [min, max], as an interval on candidate column - query column:
  // left -> right [-max, -min], right -> left [min, max]
  srrg2amd::launch_band_search(nl, s->st_pixel[0].p, s->st_desc[0].p, s->st_pixel[1].p, s->st_desc[1].p, s->st_rows[1].p, rows, cols,
                               sp->row_tolerance, -sp->max_disparity, -sp->min_disparity, nullptr, s->st_best[0].p, nullptr, nullptr, st);
  if (sp->cross_check)
    srrg2amd::launch_band_search(nr, s->st_pixel[1].p, s->st_desc[1].p, s->st_pixel[0].p, s->st_desc[0].p, s->st_rows[0].p, rows, cols,
                                 sp->row_tolerance, sp->min_disparity, sp->max_disparity, nullptr, s->st_best[1].p, nullptr, nullptr, st);
  HIP_TRY(hipMemsetAsync(s->st_counts.p, 0, S_WORDS * sizeof(int), st));
  // (the left image's keep flags are consumed: s->flags takes the matches')
  hipLaunchKernelGGL(k_stereo_resolve, dim3((nl + 3) / 4), dim3(256), 0, st, I[0], I[1], nl, s->st_pixel[0].p, s->st_pixel[1].p,
                     s->st_best[0].p, sp->cross_check ? s->st_best[1].p : nullptr, sp->max_distance, sp->subpixel, fx * sp->baseline,
                     D.zmin, D.zmax, s->st_match.p, s->st_z.p, s->flags.p);
  const int count_blocks = (nl + 255) / 256;
  hipLaunchKernelGGL(k_stereo_count, dim3(count_blocks < 64 ? count_blocks : 64), dim3(256), 0, st, s->st_match.p, nl, s->st_counts.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->scalars.p + 8, s->st_counts.p, S_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));  // (rides on the scan's wait)
  int total = 0;
  if ((rc = srrg2amd::scene_scan_flags(s, nl, &total))) return rc;
  if (total < 0 || total > nl) return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
  // the content is replaced from here on
  const size_t room = (size_t) (total > 0 ? total : 1);
  s->has_desc = s->has_inten = true;
  if ((rc = srrg2amd::scene_make_room(s, (int) room, 0))) return rc;
  if ((rc = s->gidx.reserve(room)) || (rc = s->feat_kp.reserve(room)) || (rc = s->st_match_out.reserve(room))) return rc;
  s->n = s->ng = total;
  s->has_normals = false;
  if (total > 0) {
    const Feat f{s->st_desc[0].p, nullptr, s->desc.p, nullptr};
    hipLaunchKernelGGL(k_stereo_scatter, dim3(blocks_for(nl)), dim3(256), 0, st, I[0], D, nl, s->flags.p, total, s->st_pixel[0].p,
                       s->st_kp[0].p, s->st_match.p, s->st_z.p, f, s->pts.p, s->nrm.p, s->inten.p, s->gidx.p, s->feat_kp.p, s->st_match_out.p);
    HIP_TRY(hipGetLastError());
    const int kps = keypoints_out ? (total < keypoint_capacity ? total : keypoint_capacity) : 0;
    const int ms  = matches_out ? (total < match_capacity ? total : match_capacity) : 0;
    if (kps > 0) HIP_TRY(hipMemcpyAsync(keypoints_out, s->feat_kp.p, sizeof(srrg2_keypoint) * (size_t) kps, hipMemcpyDeviceToHost, st));
    if (ms > 0)
      HIP_TRY(hipMemcpyAsync(matches_out, s->st_match_out.p, sizeof(srrg2_stereo_match) * (size_t) ms, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // dst, the records and the caller's images are done with
  }
  if (out) {
    out->num_matched  = s->scalars.p[8 + S_MATCHED];
    out->num_mutual   = s->scalars.p[8 + S_MUTUAL];
    out->num_in_range = total;
    out->scene_size   = total;
  }
  return 0;
}
