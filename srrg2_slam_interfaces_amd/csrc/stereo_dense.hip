// stereo_dense.hip -- srrg2_adapt_stereo_dense: a rectified pair of 8-bit images -> per-pixel disparity (census cost, semi-global
// aggregation along the four axis directions, uniqueness, left-right check, sub-pixel) -> depth -> the scene of the depth adaptor,
// on the device.  No reference counterpart; DESIGN.md section 4 "Dense stereo" is the contract and
// tests/stereo_dense_restatement.py its executable form.  Everything up to the float disparity is integer arithmetic, the
// disparity and the depth are float32 operations in a fixed order: the result is a function of the pixels and the parameters
// alone, bit for bit.
//   k_sd_census    one thread per pixel of either image: the 62 comparison bits of its 9 x 7 window
//   k_sd_cost      paths == 0 only: one thread per volume element, S = C
//   k_sd_paths     one wave per line (horizontal launch: a row of the rectangle, vertical launch: a column), lanes over d (up to
//                  four per lane), both directions one after the other.  The cost is the popcount of two census words, computed
//                  where it is used -- there is no cost volume; the d-1 / d+1 neighbours and the minimum over d come through
//                  cross-lane operations.  The first direction of the horizontal launch stores S, the other three add to it:
//                  every element is touched by one lane per launch and the two launches are ordered by the stream.
//   k_sd_best      one wave per pixel of the rectangle: smallest (S, d), the runner-up beyond d* +- 1, the sub-pixel disparity
//   k_sd_right     one wave per right-image pixel the rectangle's rows can point at: smallest (S, d) along the diagonal
//   k_sd_finish    one thread per image pixel: left-right check, disparity, Z and the flag byte
//   k_sd_count     the three counters from the flag bytes: grid-stride sums, one atomic per wave and counter
//   (srrg2_adapt_depth_image on Z and the left image, from device memory, on the same stream)
// Every index into the volume is 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "host_util.h"
#include "scene_state.h"

using srrg2amd::fail;

namespace {

typedef unsigned long long u64;
enum { F_EVALUATED = 1, F_UNIQUE = 2, F_CONSISTENT = 4 };
enum { C_EVALUATED = 0, C_UNIQUE = 1, C_CONSISTENT = 2, C_WORDS = 3 };
enum { HOST_COUNTERS = 12 };  // where the counters land in the scene's pinned words (8, 9: the depth adaptor's)
constexpr int BIG = 1 << 20;  // above every aggregated cost (<= 4 * (62 + 255)), and BIG + 255 is still an int

// the processed rectangle inside the image, and the volume over it: [H][W][ND], d fastest
struct SdGeom {
  int rows, cols;
  int r0, c0, H, W;  // first row / column, height, width (0 x 0 when empty)
  int dmin, ND;
  int Wr;            // right-image columns 4 .. 4 + Wr - 1 are what the rectangle's pixels can point at: W + ND - 1
};

struct SdImage {
  const unsigned char* p;
  long long stride;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

__global__ __launch_bounds__(256) void k_sd_census(SdImage L, SdImage R, int rows, int cols, u64* __restrict__ out) {
  const long long n = (long long) rows * cols;
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += (long long) gridDim.x * blockDim.x) {
    const bool right  = i >= n;
    const long long q = right ? i - n : i;
    const int r = (int) (q / cols), c = (int) (q - (long long) r * cols);
    u64 bits = 0;
    if (r >= 3 && r < rows - 3 && c >= 4 && c < cols - 4) {  // (the window stays inside the image)
      const SdImage I        = right ? R : L;
      const unsigned char* p = I.p + (long long) r * I.stride + c;
      const int v            = p[0];
      int bit                = 0;
#pragma unroll
      for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
        for (int dx = -4; dx <= 4; ++dx) {
          if (dy == 0 && dx == 0) continue;
          bits |= (u64) ((int) p[(long long) dy * I.stride + dx] < v ? 1 : 0) << bit;
          ++bit;
        }
      }
    }
    out[i] = bits;
  }
}

// paths == 0: S = C
__global__ __launch_bounds__(256) void k_sd_cost(const u64* __restrict__ cl, const u64* __restrict__ cr, SdGeom g,
                                                 unsigned short* __restrict__ vol) {
  const long long total = (long long) g.H * g.W * g.ND;
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x) {
    const long long pix = i / g.ND;
    const int k = (int) (i - pix * g.ND);
    const int y = (int) (pix / g.W), x = (int) (pix - (long long) y * g.W);
    const long long at = (long long) (g.r0 + y) * g.cols + (g.c0 + x);
    vol[i] = (unsigned short) __popcll(cl[at] ^ cr[at - (g.dmin + k)]);  // (column c - d >= 4: c >= 4 + max_disparity)
  }
}

// One wave per line, 4 lines per workgroup; lane l holds the disparities of index l + 64 j, j < NJ (ND <= 64 NJ); slots beyond
// ND hold BIG, so the terms the contract omits at the ends of the range lose every minimum by themselves.
template <int NJ>
__global__ __launch_bounds__(256) void k_sd_paths(const u64* __restrict__ cl, const u64* __restrict__ cr, SdGeom g, int p1, int p2,
                                                  int vertical, unsigned short* __restrict__ vol) {
  const int lane  = threadIdx.x & 63;
  const int line  = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lines = vertical ? g.W : g.H, len = vertical ? g.H : g.W;
  if (line >= lines) return;  // (the whole wave)
  for (int dir = 0; dir < 2; ++dir) {
    const bool store = !vertical && dir == 0;
    int prev[NJ];
    int M = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) prev[j] = BIG;
    // what a step reads from memory -- the left census word, the right ones, the S elements it adds to -- is loaded one step
    // ahead: with one wave per SIMD nothing else hides that latency, and nobody writes the next pixel's elements before then
    u64 a_next = 0, c_next[NJ];
    int old_next[NJ];
    long long at_next = 0, base_next = 0;
    const auto fetch = [&](int t) {
      const int s = dir ? len - 1 - t : t;
      const int y = vertical ? s : line, x = vertical ? line : s;
      at_next   = (long long) (g.r0 + y) * g.cols + (g.c0 + x);
      base_next = ((long long) y * g.W + x) * g.ND;
      a_next    = cl[at_next];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = lane + 64 * j;
        c_next[j]   = k < g.ND ? cr[at_next - (g.dmin + k)] : 0;  // (column c - d >= 4)
        old_next[j] = !store && k < g.ND ? (int) vol[base_next + k] : 0;
      }
    };
    fetch(0);
    for (int t = 0; t < len; ++t) {
      const long long base = base_next;
      const u64 a          = a_next;
      u64 c[NJ];
      int old[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) c[j] = c_next[j], old[j] = old_next[j];
      if (t + 1 < len) fetch(t + 1);
      int cur[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = lane + 64 * j;
        // the neighbours' values of the previous pixel: index k - 1 and k + 1 (every lane takes part in the exchange)
        int lo = __shfl_up(prev[j], 1), hi = __shfl_down(prev[j], 1);
        const int from_below = j > 0 ? __shfl(prev[j > 0 ? j - 1 : 0], 63) : BIG;
        const int from_above = j < NJ - 1 ? __shfl(prev[j < NJ - 1 ? j + 1 : j], 0) : BIG;
        if (lane == 0) lo = from_below;
        if (lane == 63) hi = from_above;
        int v = BIG;
        if (k < g.ND) {
          v = __popcll(a ^ c[j]);
          if (t > 0) v += min(min(prev[j], lo + p1), min(hi + p1, M + p2)) - M;
        }
        cur[j] = v;
      }
      int m = cur[0];
#pragma unroll
      for (int j = 1; j < NJ; ++j) m = min(m, cur[j]);
      M = wave_min(m);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int k = lane + 64 * j;
        if (k < g.ND) vol[base + k] = (unsigned short) (old[j] + cur[j]);
        prev[j] = cur[j];
      }
    }
  }
}

// (S << 16 | index): the smallest key is the smallest S and, of equal S, the smallest d.  S <= 1268, index < 256.
template <int NJ>
__global__ __launch_bounds__(256) void k_sd_best(const unsigned short* __restrict__ vol, SdGeom g, int u, int subpixel,
                                                 int* __restrict__ best, float* __restrict__ sub) {
  const int lane      = threadIdx.x & 63;
  const long long pix = (long long) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= (long long) g.H * g.W) return;  // (the whole wave)
  const long long base = pix * g.ND;
  int s[NJ];
  int key = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = lane + 64 * j;
    s[j]        = k < g.ND ? (int) vol[base + k] : BIG;
    if (k < g.ND) key = min(key, (s[j] << 16) | k);
  }
  key = wave_min(key);
  const int kb = key & 0xffff, sb = key >> 16;
  int s2 = BIG;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = lane + 64 * j;
    if (k < g.ND && abs(k - kb) > 1) s2 = min(s2, s[j]);
  }
  s2 = wave_min(s2);
  if (lane != 0) return;
  const bool unique = u == 0 || s2 == BIG || s2 * (100 - u) > 100 * sb;
  float d = (float) (g.dmin + kb);
  if (subpixel && kb > 0 && kb < g.ND - 1) {
    const int a = vol[base + kb - 1], cc = vol[base + kb + 1];
    const int D = a - 2 * sb + cc;
    if (D > 0) d = d + (float) (a - cc) / (float) (2 * D);
  }
  best[pix] = kb | (unique ? 1 << 16 : 0);
  sub[pix]  = d;
}

// right pixel (row r0 + y, column 4 + xi): the smallest (S, d) over the d whose left pixel (column 4 + xi + d) lies in the rectangle
template <int NJ>
__global__ __launch_bounds__(256) void k_sd_right(const unsigned short* __restrict__ vol, SdGeom g, unsigned short* __restrict__ right) {
  const int lane      = threadIdx.x & 63;
  const long long pix = (long long) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= (long long) g.H * g.Wr) return;  // (the whole wave)
  const int y = (int) (pix / g.Wr), xi = (int) (pix - (long long) y * g.Wr);
  int key = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = lane + 64 * j;
    const int x = 4 + xi + g.dmin + k - g.c0;  // the left pixel's column inside the rectangle
    if (k < g.ND && x >= 0 && x < g.W) key = min(key, ((int) vol[((long long) y * g.W + x) * g.ND + k] << 16) | k);
  }
  key = wave_min(key);
  if (lane == 0) right[pix] = (unsigned short) (key & 0xffff);
}

__global__ __launch_bounds__(256) void k_sd_finish(SdGeom g, const int* __restrict__ best, const float* __restrict__ sub,
                                                   const unsigned short* __restrict__ right, int lr_check, int lr_tolerance, float fb,
                                                   float* __restrict__ z, unsigned char* __restrict__ flags, unsigned char* disparity,
                                                   long long disparity_stride) {
  const long long n = (long long) g.rows * g.cols;
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
    const int r = (int) (i / g.cols), c = (int) (i - (long long) r * g.cols);
    const int y = r - g.r0, x = c - g.c0;
    float d = 0.f;
    int f   = 0;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
      const long long pix = (long long) y * g.W + x;
      const int b = best[pix], kb = b & 0xffff;
      bool ok = (b >> 16) != 0;
      f       = F_EVALUATED | (ok ? F_UNIQUE : 0);
      if (ok && lr_check) {
        const int xi = c - (g.dmin + kb) - 4;  // in [0, Wr): c >= c0 = 4 + dmin + ND - 1
        ok           = abs((int) right[(long long) y * g.Wr + xi] - kb) <= lr_tolerance;
      }
      if (ok) {
        f |= F_CONSISTENT;
        d = sub[pix];
      }
    }
    z[i]     = (f & F_CONSISTENT) ? fb / d : __int_as_float(0x7fc00000);
    flags[i] = (unsigned char) f;
    if (disparity) *reinterpret_cast<float*>(disparity + (long long) r * disparity_stride + (long long) c * 4) = d;
  }
}

// the counters from the per-pixel flag bytes: a grid-stride sum, reduced across the wave, one atomic per wave and counter -- not
// three per pixel on the same three words
__global__ __launch_bounds__(256) void k_sd_count(const unsigned char* __restrict__ flags, long long n, int* __restrict__ counts) {
  int ev = 0, un = 0, co = 0;
  for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
    const int f = flags[i];
    ev += f & 1;
    un += (f >> 1) & 1;
    co += (f >> 2) & 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    ev += __shfl_xor(ev, off);
    un += __shfl_xor(un, off);
    co += __shfl_xor(co, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (ev) atomicAdd(&counts[C_EVALUATED], ev);
    if (un) atomicAdd(&counts[C_UNIQUE], un);
    if (co) atomicAdd(&counts[C_CONSISTENT], co);
  }
}

int blocks_of(long long work, int cap) {
  const long long b = (work + 255) / 256;
  return (int) (b < 1 ? 1 : (b > cap ? cap : b));
}

struct SceneDeleter {
  void operator()(srrg2_scene* s) const { (void) srrg2_scene_destroy(s); }
};

// everything between the checks and the depth adaptor; the images are on the device
template <int NJ>
void queue_volume(srrg2_scene* s, const SdGeom& g, const srrg2_dense_stereo_params& sp) {
  hipStream_t st = s->stream;
  const u64 *cl = s->sd_census.p, *cr = s->sd_census.p + (size_t) g.rows * (size_t) g.cols;
  if (sp.paths == 0) {
    hipLaunchKernelGGL(k_sd_cost, dim3(blocks_of((long long) g.H * g.W * g.ND, 4096)), dim3(256), 0, st, cl, cr, g, s->sd_vol.p);
  } else {
    hipLaunchKernelGGL(k_sd_paths<NJ>, dim3((g.H + 3) / 4), dim3(256), 0, st, cl, cr, g, sp.p1, sp.p2, 0, s->sd_vol.p);
    hipLaunchKernelGGL(k_sd_paths<NJ>, dim3((g.W + 3) / 4), dim3(256), 0, st, cl, cr, g, sp.p1, sp.p2, 1, s->sd_vol.p);
  }
  const long long np = (long long) g.H * g.W, nr = (long long) g.H * g.Wr;
  hipLaunchKernelGGL(k_sd_best<NJ>, dim3((unsigned) ((np + 3) / 4)), dim3(256), 0, st, s->sd_vol.p, g, sp.uniqueness_ratio, sp.subpixel,
                     s->sd_best.p, s->sd_sub.p);
  if (sp.lr_check)
    hipLaunchKernelGGL(k_sd_right<NJ>, dim3((unsigned) ((nr + 3) / 4)), dim3(256), 0, st, s->sd_vol.p, g, s->sd_right.p);
}

}  // namespace

extern "C" void srrg2_adapt_default_dense_stereo_params(srrg2_dense_stereo_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_disparity    = 1;
  p->max_disparity    = 64;
  p->paths            = 4;
  p->p1               = 8;   // untuned
  p->p2               = 48;  // untuned
  p->uniqueness_ratio = 10;  // untuned
  p->lr_check         = 1;
  p->lr_tolerance     = 1;
  p->subpixel         = 1;
}

extern "C" int srrg2_adapt_stereo_dense(srrg2_scene_h dst, const void* left, int left_stride, const void* right, int right_stride, int mem,
                                        const srrg2_depth_adaptor_params* cam, const srrg2_dense_stereo_params* sp, float* disparity_out,
                                        int disparity_stride, srrg2_dense_stereo_result* out) {
  const std::string who = "adapt_stereo_dense: ";
  if (!cam || !sp) return fail(SRRG2_E_INVALID, who + "null params");
  if (!dst && !disparity_out) return fail(SRRG2_E_INVALID, who + "dst and disparity_out are both null");
  if (dst && dst->dim != 3) return fail(SRRG2_E_INVALID, who + "the scene must have dim 3");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  // what the depth adaptor refuses for cam, so that it cannot refuse once the scene's scratch has been written
  if (cam->rows < 0 || cam->cols < 0 || (long long) cam->rows * (long long) cam->cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, who + "rows, cols >= 0 and rows*cols within int32");
  if (4LL * cam->cols > 0x7fffffffLL) return fail(SRRG2_E_INVALID, who + "a row of floats beyond int32 bytes");  // (Z's row stride)
  if (cam->normal_col_gap < 0 || cam->normal_row_gap < 0 || (cam->normal_col_gap == 0) != (cam->normal_row_gap == 0))
    return fail(SRRG2_E_INVALID, who + "normal gaps >= 0, and both or neither 0");
  const float fx = cam->camera_matrix[0], fy = cam->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, who + "fx and fy must be finite and non-zero");
  if (cam->camera_matrix[1] != 0.f) return fail(SRRG2_E_UNSUPPORTED, who + "a camera matrix with skew (K[0][1] != 0)");
  if (!std::isfinite(sp->baseline) || !(sp->baseline > 0.f)) return fail(SRRG2_E_INVALID, who + "baseline must be finite and > 0");
  if (sp->min_disparity < 1 || sp->max_disparity < sp->min_disparity)
    return fail(SRRG2_E_INVALID, who + "1 <= min_disparity <= max_disparity");
  if (sp->paths != 0 && sp->paths != 4) return fail(SRRG2_E_INVALID, who + "paths must be 0 or 4");
  if (sp->p1 < 0 || sp->p2 < sp->p1 || sp->p2 > 255) return fail(SRRG2_E_INVALID, who + "0 <= p1 <= p2 <= 255");
  if (sp->uniqueness_ratio < 0 || sp->uniqueness_ratio > 99) return fail(SRRG2_E_INVALID, who + "uniqueness_ratio 0 .. 99");
  if ((sp->lr_check != 0 && sp->lr_check != 1) || (sp->subpixel != 0 && sp->subpixel != 1))
    return fail(SRRG2_E_INVALID, who + "lr_check and subpixel must be 0 or 1");
  if (sp->lr_tolerance < 0 || sp->lr_tolerance > 16) return fail(SRRG2_E_INVALID, who + "lr_tolerance 0 .. 16");
  if (sp->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  const int rows = cam->rows, cols = cam->cols;
  const long long n = (long long) rows * cols;
  if (n > 0) {
    if (!left || !right) return fail(SRRG2_E_INVALID, who + "null image");
    if ((long long) left_stride < (long long) cols || (long long) right_stride < (long long) cols)
      return fail(SRRG2_E_INVALID, who + "row stride smaller than a row");
    if (disparity_out && ((long long) disparity_stride < 4LL * cols || disparity_stride % 4 != 0 ||
                          reinterpret_cast<uintptr_t>(disparity_out) % 4 != 0))
      return fail(SRRG2_E_INVALID, who + "disparity row stride smaller than a row or no multiple of 4, or disparity_out misaligned");
  }
  const long long nd = (long long) sp->max_disparity - (long long) sp->min_disparity + 1;
  if (nd > 256) return fail(SRRG2_E_UNSUPPORTED, who + "more than 256 disparities");
  SdGeom g;
  std::memset(&g, 0, sizeof(g));
  g.rows = rows, g.cols = cols;
  g.dmin = sp->min_disparity, g.ND = (int) nd;
  const long long H = (long long) rows - 6, W = (long long) cols - 8 - (long long) sp->max_disparity;
  if (n > 0 && H > 0 && W > 0) {
    if (H * W > 0x7fffffffLL / nd) return fail(SRRG2_E_UNSUPPORTED, who + "a cost volume of more than 2^31 - 1 elements");
    g.r0 = 3, g.c0 = 4 + sp->max_disparity;
    g.H = (int) H, g.W = (int) W;
    g.Wr = g.W + g.ND - 1;
  }
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status     = n == 0 ? SRRG2_ADAPTOR_INITIALIZING : SRRG2_ADAPTOR_READY;
    out->num_pixels = (int) n;
  }
  int rc;
  // without a scene of the caller's the call works on one of its own, on the current device; it retires (and waits) on return
  std::unique_ptr<srrg2_scene, SceneDeleter> own;
  srrg2_scene* s = dst;
  if (!s) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    srrg2_scene_h h = nullptr;
    if ((rc = srrg2_scene_create(3, device, &h))) return rc;
    own.reset(h);
    s = h;
  }
  if (n == 0) {  // nothing to compute: the depth adaptor leaves the empty scene
    if (!dst) return 0;
    srrg2_adapt_result ar;
    if ((rc = srrg2_adapt_depth_image(dst, nullptr, SRRG2_IMAGE_F32, 0, nullptr, SRRG2_IMAGE_U8, 0, SRRG2_MEM_DEVICE, cam, out ? &ar : nullptr)))
      return rc;
    return 0;
  }
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->stream;
  SdImage I[2] = {{static_cast<const unsigned char*>(left), (long long) left_stride},
                  {static_cast<const unsigned char*>(right), (long long) right_stride}};
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
  const bool host_disparity = disparity_out && mem == SRRG2_MEM_HOST;
  if ((rc = s->sd_z.reserve((size_t) n)) || (rc = s->sd_flags.reserve((size_t) n)) || (rc = s->sd_counts.reserve(C_WORDS)) ||
      (host_disparity && (rc = s->sd_disp.reserve((size_t) n))))
    return rc;
  if (g.H > 0) {
    const size_t np = (size_t) g.H * (size_t) g.W;
    if ((rc = s->sd_census.reserve(2 * (size_t) n)) || (rc = s->sd_vol.reserve(np * (size_t) g.ND)) || (rc = s->sd_best.reserve(np)) ||
        (rc = s->sd_sub.reserve(np)) || (rc = s->sd_right.reserve((size_t) g.H * (size_t) g.Wr)))
      return rc;
    hipLaunchKernelGGL(k_sd_census, dim3(blocks_of(2 * n, 4096)), dim3(256), 0, st, I[0], I[1], rows, cols, s->sd_census.p);
    if (g.ND <= 64)
      queue_volume<1>(s, g, *sp);
    else if (g.ND <= 128)
      queue_volume<2>(s, g, *sp);
    else
      queue_volume<4>(s, g, *sp);
  }
  unsigned char* dev_disparity = reinterpret_cast<unsigned char*>(host_disparity ? s->sd_disp.p : disparity_out);
  const long long dev_stride   = host_disparity ? 4LL * cols : (long long) disparity_stride;
  hipLaunchKernelGGL(k_sd_finish, dim3(blocks_of(n, 2048)), dim3(256), 0, st, g, s->sd_best.p, s->sd_sub.p, s->sd_right.p, sp->lr_check,
                     sp->lr_tolerance, fx * sp->baseline, s->sd_z.p, s->sd_flags.p, dev_disparity, dev_stride);
  HIP_TRY(hipGetLastError());
  if (host_disparity)
    HIP_TRY(hipMemcpy2DAsync(disparity_out, (size_t) disparity_stride, s->sd_disp.p, 4 * (size_t) cols, 4 * (size_t) cols, (size_t) rows,
                             hipMemcpyDeviceToHost, st));
  if (out) {
    HIP_TRY(hipMemsetAsync(s->sd_counts.p, 0, C_WORDS * sizeof(int), st));
    hipLaunchKernelGGL(k_sd_count, dim3(blocks_of(n, 64)), dim3(256), 0, st, s->sd_flags.p, n, s->sd_counts.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->scalars.p + HOST_COUNTERS, s->sd_counts.p, C_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  // the one wait, at the end: the depth adaptor's own when it has a result to fill (always in compact mode), else here
  const bool wait = out || host_disparity;
  srrg2_adapt_result ar;
  std::memset(&ar, 0, sizeof(ar));
  if (dst) {
    if ((rc = srrg2_adapt_depth_image(dst, s->sd_z.p, SRRG2_IMAGE_F32, 4 * cols, I[0].p, SRRG2_IMAGE_U8, (int) I[0].stride,
                                      SRRG2_MEM_DEVICE, cam, wait ? &ar : nullptr)))
      return rc;
  } else if (wait) {
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (out) {
    out->num_evaluated  = s->scalars.p[HOST_COUNTERS + C_EVALUATED];
    out->num_unique     = s->scalars.p[HOST_COUNTERS + C_UNIQUE];
    out->num_consistent = s->scalars.p[HOST_COUNTERS + C_CONSISTENT];
    out->num_in_range   = ar.num_in_range;
    out->num_valid      = ar.num_valid;
    out->scene_size     = ar.scene_size;
  }
  return 0;
}
