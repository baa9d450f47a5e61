// features.hip -- srrg2_adapt_image_features: 8-bit intensity image (+ optional depth image) -> a compact scene of keypoints
// with 3-D point, 256-bit descriptor and intensity, on the device.  No reference counterpart (the reference reads such clouds --
// S/mapping/merger_correspondence_homo.h:36-40, multi_loop_detector_hbst_impl.cpp:84-85 -- and leaves their making to OpenCV);
// DESIGN.md section 4 "Image features" is the contract and tests/features_restatement.py its executable form.  All image
// arithmetic is integer: the result is a function of the pixels and the parameters alone, bit for bit.
//   k_feat_score_box   one 64 x 16 tile per workgroup, read ONCE into LDS as U8 (halo 3); a thread owns 4 pixels of a row, takes
//                      its 7 x 12 neighbourhood from LDS in 21 word reads and writes 4 U8 scores and 4 U16 box sums as two stores
//   k_feat_maxima      one thread per pixel: keypoint flag; score histogram of the keypoints in LDS, one global atomic per
//                      non-empty bin and workgroup
//   k_feat_cut         the cut score s* and how many keypoints of that score stay, from the histogram
//   k_feat_tie         flag of the keypoints at s*; their exclusive scan is the raster-order rank inside the class
//   k_feat_select      cap and depth gate -> keep flag per pixel
//   (exclusive scan of the keep flags: the adaptors' compaction, srrg2amd::scene_scan_flags -- the call's one host wait)
//   k_feat_scatter     kept pixel -> its slot's global index
//   k_feat_describe    one wave per keypoint: disc moments lane-strided + wave reduction, 32 projections on 32 lanes + argmax,
//                      4 x 64 comparisons assembled with __ballot; lane 0 writes point, intensity and the keypoint record
// The pipeline is queued in two halves (features_pipeline.h: select, describe) on buffers the caller names, so that stereo.hip
// runs it on two images behind one wait; srrg2_adapt_image_features hands it the scene's own arrays.  pyramid.hip runs it on
// every level of a scale pyramid: k_feat_select and k_feat_describe are templates on LEVEL, and only the <true> instantiations
// read the level map (features_pipeline.h: FeatLevel) -- the single-scale and stereo paths launch <false>, the code as it was.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "features_pipeline.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_state.h"

using srrg2amd::fail;

namespace {

enum { MARGIN = srrg2amd::FEAT_MARGIN, TILE_W = 64, TILE_H = 16, LDS_ROWS = TILE_H + 6, LDS_WORDS = (TILE_W + 8) / 4 };
// counters block (features_pipeline.h)
enum { C_CANDIDATES = srrg2amd::FEAT_C_CANDIDATES, C_MAXIMA = srrg2amd::FEAT_C_MAXIMA, C_SELECTED = srrg2amd::FEAT_C_SELECTED,
       C_CUT = srrg2amd::FEAT_C_CUT, C_QUOTA = srrg2amd::FEAT_C_QUOTA, C_TIES = srrg2amd::FEAT_C_TIES, C_HIST = srrg2amd::FEAT_C_HIST,
       C_WORDS = srrg2amd::FEAT_C_WORDS };

// round(16384 cos(2 pi k / 32)); the sine is the cosine a quarter turn back
#define FEAT_COS_TABLE                                                                                                         \
  {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069, -16384, -16069, \
   -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069}
__constant__ int kCos[32] = FEAT_COS_TABLE;  // the kernels' copy
const int kCosHost[32]    = FEAT_COS_TABLE;  // the pattern's (host)

using Image     = srrg2amd::FeatImage;
using DepthView = srrg2amd::FeatDepth;
using LevelMap  = srrg2amd::FeatLevel;

// byte `off` (-4 .. 7, relative to the thread's first pixel) of a 12-byte row held in three words; off is a constant after unrolling
__device__ __forceinline__ int row_byte(const unsigned (&w)[3], int off) {
  return (int) ((w[(off + 4) >> 2] >> (8 * ((off + 4) & 3))) & 255u);
}

// score and box-sum images of pitch `pitch` (a multiple of TILE_W) and whole tiles of rows: every word of them is written
__global__ __launch_bounds__(256) void k_feat_score_box(Image I, int aligned, unsigned* __restrict__ score, uint2* __restrict__ box,
                                                        int pitch) {
  __shared__ unsigned tile[LDS_ROWS * LDS_WORDS];
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;
  // rows r0 - 3 .. r0 + 18, columns c0 - 4 .. c0 + 67 as words; outside the image: 0
  for (int w = threadIdx.x; w < LDS_ROWS * LDS_WORDS; w += blockDim.x) {
    const int lr = w / LDS_WORDS, lw = w - lr * LDS_WORDS;
    const int r = r0 - 3 + lr, c = c0 - 4 + lw * 4;
    unsigned v = 0;
    if (r >= 0 && r < I.rows) {
      const unsigned char* row = I.p + (long long) r * I.stride;
      if (aligned && c >= 0 && c + 3 < I.cols) {
        v = *reinterpret_cast<const unsigned*>(row + c);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (c + b >= 0 && c + b < I.cols) v |= (unsigned) row[c + b] << (8 * b);
      }
    }
    tile[w] = v;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int r = r0 + ty, c = c0 + tx * 4;  // the thread's pixels: (r, c .. c + 3)
  unsigned W[7][3];                          // rows r - 3 .. r + 3, columns c - 4 .. c + 7
#pragma unroll
  for (int j = 0; j < 7; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) W[j][k] = tile[(ty + j) * LDS_WORDS + tx + k];

  // 5 x 5 box sums: column sums over rows r - 2 .. r + 2 of columns c - 2 .. c + 5, then a window of 5
  int col[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    col[j] = 0;
#pragma unroll
    for (int d = 1; d <= 5; ++d) col[j] += row_byte(W[d], j - 2);
  }
  const bool rows_in_box = r >= 2 && r < I.rows - 2, rows_in_fast = r >= 3 && r < I.rows - 3;
  unsigned bx[4], sc[4];
  constexpr int cdx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int cdy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cq = c + q;
    bx[q] = (rows_in_box && cq >= 2 && cq < I.cols - 2) ? (unsigned) ((((col[q] + col[q + 1]) + col[q + 2]) + col[q + 3]) + col[q + 4]) : 0u;
    // FAST 9/16: the largest window-of-9 minimum of d, and of -d (= minus the smallest window-of-9 maximum of d)
    const int centre = row_byte(W[3], q);
    int d[16], lo[16], hi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = row_byte(W[3 + cdy[i]], q + cdx[i]) - centre;
#pragma unroll
    for (int i = 0; i < 16; ++i) lo[i] = min(d[i], d[(i + 1) & 15]), hi[i] = max(d[i], d[(i + 1) & 15]);
    int lo4[16], hi4[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) lo4[i] = min(lo[i], lo[(i + 2) & 15]), hi4[i] = max(hi[i], hi[(i + 2) & 15]);
    int best = 0, worst = 0;  // (floored at 0: best >= 0, worst <= 0)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int lo9 = min(min(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
      const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
      best  = max(best, lo9);
      worst = min(worst, hi9);
    }
    sc[q] = (rows_in_fast && cq >= 3 && cq < I.cols - 3) ? (unsigned) max(best, -worst) : 0u;
  }
  const size_t at = ((size_t) r * (size_t) pitch + (size_t) c) >> 2;  // (r < padded rows, c + 3 < pitch: the grid is the padded image)
  score[at] = sc[0] | (sc[1] << 8) | (sc[2] << 16) | (sc[3] << 24);
  box[at]   = make_uint2(bx[0] | (bx[1] << 16), bx[2] | (bx[3] << 16));
}

// one thread per pixel in raster order.  The 8 neighbours of a pixel inside the margin lie inside the image.
__global__ __launch_bounds__(256) void k_feat_maxima(const unsigned char* __restrict__ score, int pitch, int rows, int cols, int threshold,
                                                     unsigned char* __restrict__ is_max, int* __restrict__ ctr) {
  __shared__ int hist[256];
  __shared__ int seen[2];
  hist[threadIdx.x] = 0;
  if (threadIdx.x < 2) seen[threadIdx.x] = 0;
  __syncthreads();
  const long long n = (long long) rows * cols;
  const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
  bool cand = false, kp = false;
  int s = 0;
  if (i < n) {
    const int r = (int) i / cols, c = (int) i - r * cols;  // (i < n: 32 bits)
    if (r >= MARGIN && r < rows - MARGIN && c >= MARGIN && c < cols - MARGIN) {
      const unsigned char* at = score + (size_t) r * pitch + c;
      s    = at[0];
      cand = s > threshold;
      if (cand)
        kp = s > at[-pitch - 1] && s > at[-pitch] && s > at[-pitch + 1] && s > at[-1] && s >= at[1] && s >= at[pitch - 1] &&
             s >= at[pitch] && s >= at[pitch + 1];
    }
    is_max[i] = kp ? 1 : 0;
  }
  if (kp) atomicAdd(&hist[s], 1);
  const int nc = __popcll(__ballot(cand)), nk = __popcll(__ballot(kp));
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(&seen[0], nc);
    if (nk) atomicAdd(&seen[1], nk);
  }
  __syncthreads();
  const int h = hist[threadIdx.x];
  if (h) atomicAdd(&ctr[C_HIST + threadIdx.x], h);
  if (threadIdx.x < 2 && seen[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], seen[threadIdx.x]);  // (C_CANDIDATES, C_MAXIMA)
}

// s* = the largest score with count(score >= s*) >= max_features, and how many keypoints of exactly that score stay; no cap
// (max_features == 0 or no more keypoints than that): s* = -1, every keypoint lies above it.  One wave: lane l holds bins
// 4l .. 4l + 3, a suffix sum across the lanes gives every bin its count of keypoints above it.
__global__ __launch_bounds__(64) void k_feat_cut(int max_features, int* __restrict__ ctr) {
  const int lane = threadIdx.x;
  int h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = ctr[C_HIST + 4 * lane + j];
  const int mine = (h[0] + h[1]) + (h[2] + h[3]);
  int incl = mine;  // keypoints in the bins of lanes >= this one
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_down(incl, off);
    if (lane + off < 64) incl += t;
  }
  const int total = __shfl(incl, 0);
  if (max_features <= 0 || total <= max_features) {
    if (lane == 0) ctr[C_CUT] = -1, ctr[C_QUOTA] = 0;
    return;
  }
  int above = incl - mine;  // keypoints with a score above this lane's highest bin
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (above < max_features && above + h[j] >= max_features) ctr[C_CUT] = 4 * lane + j, ctr[C_QUOTA] = max_features - above;
    above += h[j];
  }
}

__global__ __launch_bounds__(256) void k_feat_tie(const unsigned char* __restrict__ score, int pitch, int cols, int n,
                                                  const unsigned char* __restrict__ is_max, const int* __restrict__ ctr,
                                                  int* __restrict__ tie) {
  const int cut = ctr[C_CUT];
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
    int t = 0;
    if (cut >= 0 && is_max[i]) {
      const int r = (int) i / cols, c = (int) i - r * cols;  // (i < n: 32 bits)
      t = score[(size_t) r * pitch + c] == cut ? 1 : 0;
    }
    tie[i] = t;
  }
}

// tie: the exclusive scan of k_feat_tie's flags (n + 1 words).  LEVEL (a pyramid level, L its map): the depth pixel is the
// keypoint's nearest level-0 pixel, and a level whose quota is 0 selects nothing; else L is not read.
template <bool LEVEL>
__global__ __launch_bounds__(256) void k_feat_select(const unsigned char* __restrict__ score, int pitch, int cols, int n,
                                                     const unsigned char* __restrict__ is_max, const int* __restrict__ tie,
                                                     DepthView D, LevelMap L, int* __restrict__ flags, int* __restrict__ ctr) {
  const int cut = ctr[C_CUT], quota = ctr[C_QUOTA];
  int selected = 0;
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
    int keep = 0;
    if (is_max[i]) {
      const int r = (int) i / cols, c = (int) i - r * cols;  // (i < n: 32 bits)
      const int s = score[(size_t) r * pitch + c];
      if ((!LEVEL || !L.keep_none) && (s > cut || (s == cut && tie[i] < quota))) {
        ++selected;
        float z;
        if (LEVEL)
          keep = D.depth_at(LevelMap::nearest(L.q8(r), L.rows0), LevelMap::nearest(L.q8(c), L.cols0), z) ? 1 : 0;
        else
          keep = D.depth_at(r, c, z) ? 1 : 0;
      }
    }
    flags[i] = keep;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) selected += __shfl_xor(selected, off);
  if ((threadIdx.x & 63) == 0 && selected) atomicAdd(&ctr[C_SELECTED], selected);
}

// offset: the exclusive scan of the keep flags (n + 1 words)
__global__ __launch_bounds__(256) void k_feat_scatter(int n, const int* __restrict__ offset, int total, int* __restrict__ gidx) {
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
    const int k = offset[i];
    if (offset[i + 1] != k && k >= 0 && k < total) gidx[k] = (int) i;
  }
}

// One wave per keypoint (4 per workgroup).  pattern: 32 bins x 256 pairs, one word each (ax, ay, bx, by as int8, low byte first).
// Every read stays inside the image: the keypoint is >= 16 pixels from the borders, the disc reaches 15, the rotated pattern 12
// and a box sum there is valid from 2 pixels inside.  LEVEL (a pyramid level, L its map): gidx holds LEVEL pixels; the point is
// taken at the keypoint's level-0 position, pixel0 gets its nearest level-0 pixel and rec the pyramid record (kps is not written);
// else L, pixel0 and rec are not read.
template <bool LEVEL>
__global__ __launch_bounds__(256) void k_feat_describe(Image I, const unsigned char* __restrict__ score,
                                                       const unsigned short* __restrict__ box, int pitch,
                                                       const unsigned* __restrict__ pattern, DepthView D, LevelMap L, int oriented,
                                                       const int* __restrict__ gidx, int total, float4* __restrict__ pts,
                                                       float4* __restrict__ nrm, float* __restrict__ inten,
                                                       unsigned long long* __restrict__ desc, srrg2_keypoint* __restrict__ kps,
                                                       int* __restrict__ pixel0, srrg2_pyramid_keypoint* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int k    = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= total) return;  // (the whole wave)
  const int pixel = gidx[k];
  const int r = pixel / I.cols, c = pixel - r * I.cols;
  int bin = 0;
  if (oriented) {
    int m10 = 0, m01 = 0;  // |m| <= 15 * 255 * 709
    for (int j = lane; j < 31 * 31; j += 64) {
      const int dy = j / 31 - 15, dx = j - (dy + 15) * 31 - 15;
      if (dx * dx + dy * dy <= 225) {
        const int v = I.p[(long long) (r + dy) * I.stride + (c + dx)];
        m10 += dx * v;
        m01 += dy * v;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      m10 += __shfl_xor(m10, off);
      m01 += __shfl_xor(m01, off);
    }
    // lanes 0 .. 31 project on their bin; the largest wins, of equals the lowest bin
    long long proj = lane < 32 ? (long long) m10 * (long long) kCos[lane] + (long long) m01 * (long long) kCos[(lane + 24) & 31]
                               : (long long) 0x8000000000000000ull;
    bin = lane;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const long long p2 = __shfl_xor(proj, off);
      const int b2       = __shfl_xor(bin, off);
      if (p2 > proj || (p2 == proj && b2 < bin)) proj = p2, bin = b2;
    }
  }
  const unsigned short* const B = box + (size_t) r * pitch + c;
  unsigned long long word = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned pr = pattern[bin * 256 + w * 64 + lane];
    const int ax = (int) (signed char) (pr & 255u), ay = (int) (signed char) ((pr >> 8) & 255u);
    const int bx = (int) (signed char) ((pr >> 16) & 255u), by = (int) (signed char) (pr >> 24);
    const unsigned long long m = __ballot(B[ay * pitch + ax] < B[by * pitch + bx]);
    if (lane == w) word = m;
  }
  if (lane < 4) desc[(size_t) k * 4 + lane] = word;
  if (LEVEL) {
    if (lane == 0) {
      const int u = L.q8(c), v = L.q8(r);
      const int r0 = LevelMap::nearest(v, L.rows0), c0 = LevelMap::nearest(u, L.cols0);
      float z = 1.f;
      D.depth_at(r0, c0, z);  // (in range: k_feat_select kept the pixel)
      const float3 q = LevelMap::point_at(D, u, v, z);
      pts[k]   = make_float4(q.x, q.y, q.z, 0.f);
      nrm[k]   = make_float4(0.f, 0.f, 0.f, 0.f);
      inten[k] = (float) I.p[(long long) r * I.stride + c];
      srrg2_pyramid_keypoint kp;
      kp.pixel = r0 * L.cols0 + c0, kp.score = score[(size_t) r * pitch + c], kp.angle_bin = bin, kp.level = L.level;
      kp.level_pixel = pixel, kp.u_q8 = u, kp.v_q8 = v, kp.reserved = 0;
      pixel0[k] = kp.pixel;
      rec[k]    = kp;
    }
    return;
  }
  if (lane == 0) {
    if (pts) {  // (null: the caller makes the point itself, stereo.hip)
      float z = 1.f;
      D.depth_at(r, c, z);  // (in range: k_feat_select kept the pixel)
      const float3 q = D.point_at(r, c, z);
      pts[k]   = make_float4(q.x, q.y, q.z, 0.f);
      nrm[k]   = make_float4(0.f, 0.f, 0.f, 0.f);
      inten[k] = (float) I.p[(long long) r * I.stride + c];
    }
    srrg2_keypoint kp;
    kp.pixel = pixel, kp.score = score[(size_t) r * pitch + c], kp.angle_bin = bin, kp.reserved = 0;
    kps[k] = kp;
  }
}

// ---- the pattern (host) ------------------------------------------------------------------------------------------------
// 256 pairs from a 64-bit linear congruential generator, candidates outside the disc of radius 13 or with a == b rejected
struct Pattern {
  int8_t base[256][4];
  Pattern() {
    unsigned long long x = 0x5352524732ull;
    const auto next = [&x]() -> int {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      return (int) ((x >> 33) % 7ull);
    };
    const auto coord = [&next]() -> int {
      int s = next();
      s += next();
      s += next();
      s += next();
      return s - 12;
    };
    int have = 0;
    while (have < 256) {
      const int ax = coord(), ay = coord(), bx = coord(), by = coord();
      if (ax * ax + ay * ay > 169 || bx * bx + by * by > 169 || (ax == bx && ay == by)) continue;
      base[have][0] = (int8_t) ax, base[have][1] = (int8_t) ay, base[have][2] = (int8_t) bx, base[have][3] = (int8_t) by;
      ++have;
    }
  }
  // x' = floor((x C - y S + 8192) / 16384), y' = floor((x S + y C + 8192) / 16384): arithmetic shifts
  void rotated(int bin, int8_t* out) const {
    const int C = kCosHost[bin], S = kCosHost[(bin + 24) & 31];
    for (int i = 0; i < 256; ++i)
      for (int o = 0; o < 4; o += 2) {
        const int x = base[i][o], y = base[i][o + 1];
        out[i * 4 + o]     = (int8_t) ((x * C - y * S + 8192) >> 14);
        out[i * 4 + o + 1] = (int8_t) ((x * S + y * C + 8192) >> 14);
      }
  }
};

const Pattern& pattern() {
  static const Pattern p;
  return p;
}

int blocks_of(int n) {
  const int b = (n + 255) / 256;
  return b < 1 ? 1 : (b > 1024 ? 1024 : b);
}

bool aligned_to(const void* p, long long stride, int elem) {
  return reinterpret_cast<uintptr_t>(p) % (uintptr_t) elem == 0 && stride % elem == 0;
}

}  // namespace

// dst becomes an empty feature scene (arrays for one point, as the adaptors leave them)
int srrg2amd::feat_empty_scene(srrg2_scene* s) {
  int rc;
  s->has_desc = s->has_inten = true;
  if ((rc = srrg2amd::scene_make_room(s, 1, 0)) || (rc = s->gidx.reserve(1))) return rc;
  s->n = s->ng = 0;
  s->has_normals = false;
  return 0;
}

int srrg2amd::feat_check_params(const std::string& who, const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* p,
                                int keypoint_capacity) {
  if (cam->rows < 0 || cam->cols < 0 || (long long) cam->rows * (long long) cam->cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, who + "rows, cols >= 0 and rows*cols within int32");
  if (p->fast_threshold < 0 || p->fast_threshold > 254) return fail(SRRG2_E_INVALID, who + "fast_threshold 0 .. 254");
  if (p->max_features < 0) return fail(SRRG2_E_INVALID, who + "max_features >= 0");
  if (p->oriented != 0 && p->oriented != 1) return fail(SRRG2_E_INVALID, who + "oriented must be 0 or 1");
  if (p->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  if (keypoint_capacity < 0) return fail(SRRG2_E_INVALID, who + "keypoint_capacity >= 0");
  const float fx = cam->camera_matrix[0], fy = cam->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, who + "fx and fy must be finite and non-zero");
  if (cam->camera_matrix[1] != 0.f) return fail(SRRG2_E_UNSUPPORTED, who + "a camera matrix with skew (K[0][1] != 0)");
  return 0;
}

int srrg2amd::feat_check_images(const std::string& who, srrg2_scene* dst, const void* intensity, int intensity_type,
                                int intensity_stride, const void* depth, int depth_type, int depth_stride, int mem,
                                const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* p, int keypoint_capacity) {
  int rc;
  if (!dst || !cam || !p) return fail(SRRG2_E_INVALID, who + "null scene or params");
  if (dst->dim != 3) return fail(SRRG2_E_INVALID, who + "the scene must have dim 3");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (intensity_type == SRRG2_IMAGE_U16 || intensity_type == SRRG2_IMAGE_F32)
    return fail(SRRG2_E_UNSUPPORTED, who + "the intensity image must be U8 (U16 and F32 are not supported)");
  if (intensity_type != SRRG2_IMAGE_U8) return fail(SRRG2_E_INVALID, who + "intensity_type must be SRRG2_IMAGE_U8");
  if (depth_type != SRRG2_IMAGE_NONE && depth_type != SRRG2_IMAGE_U16 && depth_type != SRRG2_IMAGE_F32)
    return fail(SRRG2_E_INVALID, who + "depth_type must be NONE, U16 or F32");
  if ((depth != nullptr) != (depth_type != SRRG2_IMAGE_NONE) && (depth || cam->rows * (long long) cam->cols > 0))
    return fail(SRRG2_E_INVALID, who + "a depth image needs depth_type U16 or F32, and a depth_type its image");
  if ((rc = srrg2amd::feat_check_params(who, cam, p, keypoint_capacity))) return rc;
  const int de = depth_type == SRRG2_IMAGE_U16 ? 2 : 4;
  if (cam->rows * cam->cols > 0) {
    if (!intensity) return fail(SRRG2_E_INVALID, who + "null image");
    if ((long long) intensity_stride < (long long) cam->cols) return fail(SRRG2_E_INVALID, who + "intensity row stride smaller than a row");
    if (depth && ((long long) depth_stride < (long long) cam->cols * de || !aligned_to(depth, depth_stride, de)))
      return fail(SRRG2_E_INVALID, who + "depth row stride smaller than a row, or image not aligned to its element");
  }
  return 0;
}

int srrg2amd::feat_stage_images(srrg2_scene* s, const void* intensity, int intensity_stride, const void* depth, int depth_type,
                                int depth_stride, int mem, const srrg2_depth_adaptor_params* cam, FeatImage* image, FeatDepth* view) {
  const int rows = cam->rows, cols = cam->cols;
  const bool with_depth = depth != nullptr;
  const int de = depth_type == SRRG2_IMAGE_U16 ? 2 : 4;
  hipStream_t st = s->stream;
  int rc;
  Image I{static_cast<const unsigned char*>(intensity), (long long) intensity_stride, rows, cols};
  DepthView D;
  std::memset(&D, 0, sizeof(D));
  D.p      = static_cast<const unsigned char*>(depth);
  D.stride = depth_stride;
  D.f32    = depth_type == SRRG2_IMAGE_F32;
  D.ifx = 1.0f / cam->camera_matrix[0], D.ify = 1.0f / cam->camera_matrix[4];
  D.cx = cam->camera_matrix[2], D.cy = cam->camera_matrix[5];
  D.scale = cam->depth_scale, D.zmin = cam->depth_min, D.zmax = cam->depth_max;
  if (mem == SRRG2_MEM_HOST) {  // rows up to the last pixel of the last row, as they lie
    const size_t bi    = (size_t) (rows - 1) * (size_t) intensity_stride + (size_t) cols;
    const size_t bd    = with_depth ? (size_t) (rows - 1) * (size_t) depth_stride + (size_t) cols * de : 0;
    const size_t off_d = (bi + 63) / 64 * 64;
    if ((rc = s->staging.reserve(off_d + bd + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->staging.p, intensity, bi, hipMemcpyHostToDevice, st));
    I.p = reinterpret_cast<const unsigned char*>(s->staging.p);
    if (with_depth) {
      HIP_TRY(hipMemcpyAsync(s->staging.p + off_d, depth, bd, hipMemcpyHostToDevice, st));
      D.p = reinterpret_cast<const unsigned char*>(s->staging.p + off_d);
    }
  }
  *image = I, *view = D;
  return 0;
}

size_t srrg2amd::feat_padded_pixels(int rows, int cols) {
  const int tiles_x = (cols + TILE_W - 1) / TILE_W, tiles_y = (rows + TILE_H - 1) / TILE_H;
  return (size_t) (tiles_x * TILE_W) * (size_t) (tiles_y * TILE_H);
}

int srrg2amd::feat_pattern_upload(srrg2_scene* s) {
  if (s->feat_pattern_ready) return 0;
  int rc;
  if ((rc = s->feat_pattern.reserve(32 * 256))) return rc;
  int8_t all[32][1024];
  for (int b = 0; b < 32; ++b) pattern().rotated(b, all[b]);
  HIP_TRY(hipMemcpyAsync(s->feat_pattern.p, all, sizeof(all), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (`all` leaves the stack)
  s->feat_pattern_ready = true;
  return 0;
}

namespace {

// both halves, for the single-scale callers (level null: the identity map, not read) and for a pyramid level
int queue_select(const Image& I, const DepthView& D, const LevelMap* level, int fast_threshold, int max_features,
                 const srrg2amd::FeatWork& w, hipStream_t st) {
  const int rows = I.rows, cols = I.cols, n = rows * cols;
  const int tiles_x = (cols + TILE_W - 1) / TILE_W, tiles_y = (rows + TILE_H - 1) / TILE_H;
  const int pitch = tiles_x * TILE_W;
  int* const ctr  = w.ctr;
  HIP_TRY(hipMemsetAsync(ctr, 0, C_WORDS * sizeof(int), st));
  const int word_reads = reinterpret_cast<uintptr_t>(I.p) % 4 == 0 && I.stride % 4 == 0;
  hipLaunchKernelGGL(k_feat_score_box, dim3(tiles_x, tiles_y), dim3(256), 0, st, I, word_reads, reinterpret_cast<unsigned*>(w.score),
                     reinterpret_cast<uint2*>(w.box), pitch);
  hipLaunchKernelGGL(k_feat_maxima, dim3((unsigned) (((long long) n + 255) / 256)), dim3(256), 0, st, w.score, pitch, rows, cols,
                     fast_threshold, w.is_max, ctr);
  hipLaunchKernelGGL(k_feat_cut, dim3(1), dim3(64), 0, st, max_features, ctr);
  const dim3 grid(blocks_of(n)), block(256);
  hipLaunchKernelGGL(k_feat_tie, grid, block, 0, st, w.score, pitch, cols, n, w.is_max, ctr, w.tie);
  srrg2amd::launch_exclusive_scan(w.tie, n, w.scan_sums, ctr + C_TIES, st);
  if (level)
    hipLaunchKernelGGL(k_feat_select<true>, grid, block, 0, st, w.score, pitch, cols, n, w.is_max, w.tie, D, *level, w.flags, ctr);
  else
    hipLaunchKernelGGL(k_feat_select<false>, grid, block, 0, st, w.score, pitch, cols, n, w.is_max, w.tie, D, LevelMap{}, w.flags, ctr);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

int srrg2amd::feat_queue_select(const FeatImage& I, const FeatDepth& D, int fast_threshold, int max_features, const FeatWork& w,
                                hipStream_t st) {
  return queue_select(I, D, nullptr, fast_threshold, max_features, w, st);
}

int srrg2amd::feat_queue_select_level(const FeatImage& I, const FeatDepth& D, const FeatLevel& L, int fast_threshold,
                                      int max_features, const FeatWork& w, hipStream_t st) {
  return queue_select(I, D, &L, fast_threshold, max_features, w, st);
}

int srrg2amd::feat_queue_describe(const FeatImage& I, const FeatDepth& D, int oriented, const FeatWork& w, const unsigned* pattern,
                                  int total, const FeatOut& o, hipStream_t st) {
  const int n     = I.rows * I.cols;
  const int pitch = (I.cols + TILE_W - 1) / TILE_W * TILE_W;
  hipLaunchKernelGGL(k_feat_scatter, dim3(blocks_of(n)), dim3(256), 0, st, n, w.flags, total, o.gidx);
  hipLaunchKernelGGL(k_feat_describe<false>, dim3((total + 3) / 4), dim3(256), 0, st, I, w.score, w.box, pitch, pattern, D, LevelMap{},
                     oriented, o.gidx, total, o.pts, o.nrm, o.inten, o.desc, o.kps, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  return 0;
}

int srrg2amd::feat_queue_describe_level(const FeatImage& I, const FeatDepth& D, const FeatLevel& L, int oriented, const FeatWork& w,
                                        const unsigned* pattern, int total, int* lpix, const FeatOut& o, srrg2_pyramid_keypoint* rec,
                                        hipStream_t st) {
  const int n     = I.rows * I.cols;
  const int pitch = (I.cols + TILE_W - 1) / TILE_W * TILE_W;
  hipLaunchKernelGGL(k_feat_scatter, dim3(blocks_of(n)), dim3(256), 0, st, n, w.flags, total, lpix);
  hipLaunchKernelGGL(k_feat_describe<true>, dim3((total + 3) / 4), dim3(256), 0, st, I, w.score, w.box, pitch, pattern, D, L, oriented,
                     lpix, total, o.pts, o.nrm, o.inten, o.desc, nullptr, o.gidx, rec);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" void srrg2_adapt_default_feature_params(srrg2_feature_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->fast_threshold = 20;
  p->max_features   = 1000;
  p->oriented       = 1;
}

extern "C" int srrg2_feature_pattern(int angle_bin, int8_t* pairs_out) {
  if (angle_bin < 0 || angle_bin > 31 || !pairs_out) return fail(SRRG2_E_INVALID, "feature_pattern: angle_bin 0 .. 31 and a buffer of 1024");
  pattern().rotated(angle_bin, pairs_out);
  return 0;
}

extern "C" int srrg2_adapt_image_features(srrg2_scene_h dst, const void* intensity, int intensity_type, int intensity_stride,
                                          const void* depth, int depth_type, int depth_stride, int mem,
                                          const srrg2_depth_adaptor_params* cam, const srrg2_feature_params* p,
                                          srrg2_keypoint* keypoints_out, int keypoint_capacity, srrg2_feature_result* out) {
  const std::string who = "adapt_image_features: ";
  int rc;
  if ((rc = srrg2amd::feat_check_images(who, dst, intensity, intensity_type, intensity_stride, depth, depth_type, depth_stride, mem,
                                        cam, p, keypoint_capacity)))
    return rc;
  const int rows = cam->rows, cols = cam->cols;
  const int n = rows * cols;
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
  if (rows <= 2 * MARGIN || cols <= 2 * MARGIN) return srrg2amd::feat_empty_scene(s);  // no pixel 16 away from every border

  Image I;
  DepthView D;
  if ((rc = srrg2amd::feat_stage_images(s, intensity, intensity_stride, depth, depth_type, depth_stride, mem, cam, &I, &D))) return rc;
  const size_t padded = srrg2amd::feat_padded_pixels(rows, cols);
  if ((rc = s->feat_score.reserve(padded)) || (rc = s->feat_box.reserve(padded))) return rc;
  if ((rc = s->feat_max.reserve((size_t) n)) || (rc = s->feat_tie.reserve((size_t) n + 1))) return rc;
  if ((rc = s->flags.reserve((size_t) n + 1)) || (rc = s->feat_ctr.reserve(C_WORDS))) return rc;
  if ((rc = s->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(n) + 2))) return rc;
  if ((rc = srrg2amd::feat_pattern_upload(s))) return rc;  // the 32 rotated patterns, once per scene
  const srrg2amd::FeatWork work{s->feat_score.p, s->feat_box.p, s->feat_max.p, s->feat_tie.p, s->feat_ctr.p, s->flags.p, s->scan_sums.p};
  int* const ctr = s->feat_ctr.p;
  if ((rc = srrg2amd::feat_queue_select(I, D, p->fast_threshold, p->max_features, work, st))) return rc;
  HIP_TRY(hipMemcpyAsync(s->scalars.p + 8, ctr, 4 * sizeof(int), hipMemcpyDeviceToHost, st));  // (rides on the scan's wait)
  int total = 0;
  if ((rc = srrg2amd::scene_scan_flags(s, n, &total))) return rc;
  if (total < 0 || total > n) return fail(SRRG2_E_HIP, who + "the compaction scan returned a total out of range");
  // the content is replaced from here on
  s->has_desc = s->has_inten = true;
  if ((rc = srrg2amd::scene_make_room(s, total > 0 ? total : 1, 0))) return rc;
  if ((rc = s->gidx.reserve((size_t) (total > 0 ? total : 1))) || (rc = s->feat_kp.reserve((size_t) (total > 0 ? total : 1)))) return rc;
  s->n = s->ng = total;
  s->has_normals = false;
  if (total > 0) {
    const srrg2amd::FeatOut o{s->gidx.p, reinterpret_cast<unsigned long long*>(s->desc.p), s->feat_kp.p, s->pts.p, s->nrm.p, s->inten.p};
    if ((rc = srrg2amd::feat_queue_describe(I, D, p->oriented, work, s->feat_pattern.p, total, o, st))) return rc;
    const int copied = keypoints_out ? (total < keypoint_capacity ? total : keypoint_capacity) : 0;
    if (copied > 0)
      HIP_TRY(hipMemcpyAsync(keypoints_out, s->feat_kp.p, sizeof(srrg2_keypoint) * (size_t) copied, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // dst, and the caller's images, are done with
  }
  if (out) {
    out->num_candidates = s->scalars.p[8 + C_CANDIDATES];
    out->num_maxima     = s->scalars.p[8 + C_MAXIMA];
    out->num_selected   = s->scalars.p[8 + C_SELECTED];
    out->num_with_depth = total;
    out->scene_size     = total;
  }
  return 0;
}
