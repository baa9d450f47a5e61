// gridmap.hip -- srrg2_gridmap_*: occupancy grid maps from laser scans and poses, on the device.  No reference counterpart;
// DESIGN.md section 4 "Occupancy grid" is the contract and tests/gridmap_restatement.py its executable form.  A beam's float work
// (its bearing's sine / cosine in float64 -- scan_beam.h, the scan adaptor's expression --, the pose composed with the sensor's
// mount, the float32 divide that makes a cell of a point) happens once per beam; everything behind it is integer, so the planes
// are a function of the inputs alone, bit for bit, whatever the scheduling, the scan order or the split into calls.
//   k_gridmap_integrate  one lane per beam, adjacent lanes adjacent beams, grid-stride over num_scans * num_beams.  A lane walks
//                        its ray step by step: at a given step a wave's 64 cells are neighbours on an arc, so the no-return
//                        32-bit atomic adds of one wave-instruction land in a few rows.  The closed form of the contract,
//                        (2 i |d| + n) / (2 n), is carried as quotient and remainder: +2|d| per step and at most one carry, no
//                        division in the loop.  The result's counters are summed per lane, then per workgroup (block_add), ONE
//                        64-bit atomic per workgroup and counter.  <true>, what the library runs: the wave walks its 64 rays in
//                        step and a run of adjacent lanes on one cell adds once (see SRRG2_GRIDMAP_WAVE_MERGE).
//   k_gridmap_render     a thread owns 4 adjacent cells of a row: one 32-bit store where the four bytes exist and lie aligned
//   k_gridmap_flag       keep flag per cell for the scene export; srrg2amd::scene_compact_into (the clippers' tail) scans them
//   k_gridmap_scatter    ... and this moves a kept cell's centre to its slot
// Render and export read the planes behind the integrate kernel in stream order: no flags, no polling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "det_math.h"
#include "device_util.h"
#include "gridmap_state.h"
#include "host_util.h"
#include "scan_beam.h"
#include "scene_state.h"

using srrg2amd::fail;
using srrg2amd::gridmap_check_scan_call;
using srrg2amd::gridmap_ready;

namespace {

enum { MAX_SIDE = 32768, MAX_RAY = GRIDMAP_MAX_RAY, MAX_BLOCKS = 1024 };
enum { C_RETURNS = 0, C_CLEARED, C_HITS, C_MISSES, C_WORDS };

struct GridArgs {
  int* hits;
  int* misses;
  int rows, cols;
  float ox, oy, res;
};

struct BeamArgs {
  const float* ranges;  // total
  const float* poses;   // 9 per scan
  long long total;
  int nb;
  double amin, ainc;
  float rmin, rmax;
  float S[9];
  int clear, weight;
};

// a beam ready to be walked: start cell, direction, 2|dx|, 2|dy|, n (-1: the beam adds nothing), and whether step n is a hit
struct Ray {
  int x0, y0, sx, sy, ax2, ay2, n;
  bool hit;
};

// the float work of beam i, once: its class (counted), the pose composed with the mount, the end point, the four cells
__device__ __forceinline__ Ray beam_ray(const GridArgs& G, const BeamArgs& B, long long i, unsigned long long& returns,
                                        unsigned long long& cleared) {
  Ray R;
  R.x0 = R.y0 = R.sx = R.sy = R.ax2 = R.ay2 = 0, R.n = -1, R.hit = false;
  const int scan = (int) (i / B.nb), k = (int) (i - (long long) scan * B.nb);
  const float r = B.ranges[i];
  float reach;
  if (isfinite(r) && B.rmin <= r && r <= B.rmax) {
    reach = r, R.hit = true;
    ++returns;
  } else if (r > B.rmax && B.clear) {  // (+inf as well; a NaN compares false)
    reach = B.rmax;
    ++cleared;
  } else {
    return R;
  }
  float T[9];
  dm::se2_compose(B.poses + 9 * (long long) scan, B.S, T);
  const float2 b = scan_beam_point(B.amin, B.ainc, k, reach);
  const float ex = (T[0] * b.x + T[1] * b.y) + T[2];
  const float ey = (T[3] * b.x + T[4] * b.y) + T[5];
  int x1, y1;
  if (!cell_of(T[2], G.ox, G.res, R.x0) || !cell_of(T[5], G.oy, G.res, R.y0) || !cell_of(ex, G.ox, G.res, x1) ||
      !cell_of(ey, G.oy, G.res, y1))
    return R;
  const int dx = x1 - R.x0, dy = y1 - R.y0;  // (|coordinates| <= 2^30: the differences fit)
  const int ax = abs(dx), ay = abs(dy), n = max(ax, ay);
  if (n > MAX_RAY) return R;
  R.sx = dx < 0 ? -1 : 1, R.sy = dy < 0 ? -1 : 1;
  R.ax2 = 2 * ax, R.ay2 = 2 * ay, R.n = n;
  return R;
}

// MERGE: the wave walks its 64 rays in step and adjacent lanes that hold the same cell of the same plane add ONCE -- the first
// lane of a run adds the run's length (near the sensor every beam of a scan crosses the same few cells).  Integer adds: the
// planes are the same bits either way.  The library runs the merged walk, 4.6 times faster on a full re-draw; the plain walk is
// what it was measured against (make EXTRA=-DSRRG2_GRIDMAP_WAVE_MERGE=0 OUT=... and SRRG2_AMD_LIB; DESIGN.md section 4 has
// both timings).
#ifndef SRRG2_GRIDMAP_WAVE_MERGE
#define SRRG2_GRIDMAP_WAVE_MERGE 1
#endif

template <bool MERGE>
__global__ __launch_bounds__(256) void k_gridmap_integrate(GridArgs G, BeamArgs B, unsigned long long* __restrict__ ctr) {
  unsigned long long returns = 0, cleared = 0, hits = 0, misses = 0;
  const long long stride = (long long) gridDim.x * 256;
  const long long cells  = (long long) G.rows * G.cols;  // (the planes are one block: misses = hits + cells)
  if (!MERGE) {
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < B.total; i += stride) {
      const Ray R = beam_ray(G, B, i, returns, cleared);
      if (R.n < 0) continue;
      // step i: quotient and remainder of (2 i a + n) / (2 n), from (0, n) at i = 0; 2 a <= 2 n: at most one carry per step
      int cx = R.x0, cy = R.y0, rx = R.n, ry = R.n;
      const int n2 = 2 * R.n;
      for (int s = 0; s < R.n; ++s) {
        if ((unsigned) cx < (unsigned) G.cols && (unsigned) cy < (unsigned) G.rows) {
          atomicAdd(&G.misses[(long long) cy * G.cols + cx], B.weight);
          ++misses;
        }
        rx += R.ax2, ry += R.ay2;
        if (rx >= n2) rx -= n2, cx += R.sx;
        if (ry >= n2) ry -= n2, cy += R.sy;
      }
      if (R.hit && (unsigned) cx < (unsigned) G.cols && (unsigned) cy < (unsigned) G.rows) {  // (step n: the end cell)
        atomicAdd(&G.hits[(long long) cy * G.cols + cx], B.weight);
        ++hits;
      }
    }
  } else {
    const int lane = threadIdx.x & 63;
    // every lane of a wave takes every trip and every step (the shuffles need them all): the wave's first beam decides
    for (long long i0 = (long long) blockIdx.x * 256 + (threadIdx.x & ~63); i0 < B.total; i0 += stride) {
      const long long i = i0 + lane;
      Ray R = {0, 0, 0, 0, 0, 0, -1, false};
      if (i < B.total) R = beam_ray(G, B, i, returns, cleared);
      int longest = R.n;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) longest = max(longest, __shfl_xor(longest, off));
      int cx = R.x0, cy = R.y0, rx = R.n, ry = R.n;
      const int n2 = 2 * R.n;
      for (int s = 0; s <= longest; ++s) {
        // the word of the planes block this lane adds to at this step, or -1
        long long word = -1;
        if (s <= R.n && (s < R.n || R.hit) && (unsigned) cx < (unsigned) G.cols && (unsigned) cy < (unsigned) G.rows) {
          word = (long long) cy * G.cols + cx + (s < R.n ? cells : 0);
          if (s < R.n)
            ++misses;
          else
            ++hits;
        }
        const long long before = __shfl_up(word, 1);
        const bool head = word >= 0 && (lane == 0 || before != word);
        const unsigned long long edges = __ballot(head || word < 0);  // where a run ends: the next head, or a lane without a word
        if (head) {
          const unsigned long long rest = lane == 63 ? 0ull : edges >> (lane + 1);
          const int run = rest ? __ffsll((long long) rest) : 64 - lane;
          atomicAdd(&G.hits[word], B.weight * run);
        }
        if (s < R.n) {
          rx += R.ax2, ry += R.ay2;
          if (rx >= n2) rx -= n2, cx += R.sx;
          if (ry >= n2) ry -= n2, cy += R.sy;
        }
      }
    }
  }
  block_add(returns, &ctr[C_RETURNS]);
  block_add(cleared, &ctr[C_CLEARED]);
  block_add(hits, &ctr[C_HITS]);
  block_add(misses, &ctr[C_MISSES]);
}

// a thread: cells (r, c .. c + 3); quads = ceil(cols / 4)
__global__ __launch_bounds__(256) void k_gridmap_render(GridArgs G, long long need, int quads, unsigned char* __restrict__ dst,
                                                        long long stride) {
  const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long) G.rows * quads) return;
  const int r = (int) (t / quads), c = (int) (t - (long long) r * quads) * 4;
  const int left = min(4, G.cols - c);
  const long long at = (long long) r * G.cols + c;
  unsigned v[4], word = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = q < left ? cell_value(G.hits[at + q], G.misses[at + q], need) : 0u;
    word |= v[q] << (8 * q);
  }
  unsigned char* out = dst + (long long) r * stride + c;
  if (left == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
    *reinterpret_cast<unsigned*>(out) = word;
  } else {  // the row's tail, or a row that does not start on a word
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < left) out[q] = (unsigned char) v[q];
  }
}

__global__ __launch_bounds__(256) void k_gridmap_flag(GridArgs G, long long need, unsigned occupied, int n, int* __restrict__ flags) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned v = cell_value(G.hits[i], G.misses[i], need);
    flags[i] = (v >= occupied && v <= 100u) ? 1 : 0;
  }
}

// behind the scan of the flags: a kept cell i goes to slot offset[i]; the k >= cap guard is the clippers'
__global__ __launch_bounds__(256) void k_gridmap_scatter(GridArgs G, int n, const int* __restrict__ offset, float4* __restrict__ out_pts,
                                                         float4* __restrict__ out_nrm, int* __restrict__ gidx, int cap) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int k = offset[i];
    if (offset[i + 1] == k || k >= cap) continue;
    const int iy = i / G.cols, ix = i - iy * G.cols;
    out_pts[k] = make_float4(G.ox + ((float) ix + 0.5f) * G.res, G.oy + ((float) iy + 0.5f) * G.res, 0.f, 0.f);
    out_nrm[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    gidx[k]    = i;
  }
}

int blocks_of(long long n) { return (int) std::min<long long>((n + 255) / 256, 1 << 20); }

GridArgs grid_args(const srrg2_gridmap_s* h) {
  const long long n = h->cells();
  return GridArgs{h->planes.p, h->planes.p + n, h->p.rows, h->p.cols, h->p.origin[0], h->p.origin[1], h->p.resolution};
}

int check_grid_params(const std::string& who, const srrg2_gridmap_params* p) {
  if (!p) return fail(SRRG2_E_INVALID, who + "null params");
  if (p->rows < 0 || p->cols < 0 || p->rows > MAX_SIDE || p->cols > MAX_SIDE)
    return fail(SRRG2_E_INVALID, who + "rows and cols must lie in 0 .. 32768");
  if (!std::isfinite(p->resolution) || !(p->resolution > 0.f)) return fail(SRRG2_E_INVALID, who + "resolution must be finite and > 0");
  if (!std::isfinite(p->origin[0]) || !std::isfinite(p->origin[1])) return fail(SRRG2_E_INVALID, who + "origin must be finite");
  return 0;
}

}  // namespace

// what srrg2_gridmap_integrate_scans refuses without looking at its handle (srrg2_gridmap_match_scans refuses the same)
int srrg2amd::gridmap_check_scan_call(const std::string& who, const float* ranges, int num_scans, const float* poses, int mem,
                                      const srrg2_gridmap_scan_params* p, int weight) {
  if (!p) return fail(SRRG2_E_INVALID, who + "null params");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (weight != 1 && weight != -1) return fail(SRRG2_E_INVALID, who + "weight must be +1 or -1");
  if (num_scans < 0 || p->num_beams < 0) return fail(SRRG2_E_INVALID, who + "num_scans, num_beams >= 0");
  if (p->clear_beyond_max != 0 && p->clear_beyond_max != 1) return fail(SRRG2_E_INVALID, who + "clear_beyond_max must be 0 or 1");
  // the scan model, as srrg2_scene_clip_scan checks it
  const double TWO_PI = 6.283185307179586;
  const double inc    = std::fabs(p->angle_increment);
  if (!std::isfinite(p->angle_increment) || p->angle_increment == 0.0)
    return fail(SRRG2_E_INVALID, who + "angle_increment must be finite and non-zero");
  if (!std::isfinite(p->angle_min) || std::fabs(p->angle_min) > TWO_PI)
    return fail(SRRG2_E_INVALID, who + "angle_min must be finite and within [-2 pi, 2 pi]");
  if (inc * (double) p->num_beams > (TWO_PI + inc) * (1.0 + 0x1p-20))
    return fail(SRRG2_E_INVALID, who + "|angle_increment| * num_beams beyond 2 pi plus one increment");
  if (!(p->range_min > 0.f) || !(p->range_max >= p->range_min)) return fail(SRRG2_E_INVALID, who + "0 < range_min <= range_max");
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(p->sensor_in_robot[i])) return fail(SRRG2_E_INVALID, who + "sensor_in_robot must be finite");
  if ((long long) num_scans * p->num_beams > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "num_scans * num_beams beyond int32");
  if (num_scans > 0 && p->num_beams > 0 &&
      (!ranges || !poses || reinterpret_cast<uintptr_t>(ranges) % 4 != 0 || reinterpret_cast<uintptr_t>(poses) % 4 != 0))
    return fail(SRRG2_E_INVALID, who + "null or misaligned ranges or poses");
  return 0;
}

int srrg2amd::gridmap_ready(const std::string& who, srrg2_gridmap_s* h) {
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  if (!h->is_set) return fail(SRRG2_E_INVALID, who + "no grid (srrg2_gridmap_reset)");
  return 0;
}

extern "C" int srrg2_gridmap_create(int device, srrg2_gridmap_h* out) {
  if (!out) return fail(SRRG2_E_INVALID, "gridmap_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "gridmap_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "gridmap_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<srrg2_gridmap_s> h(new srrg2_gridmap_s());  // (a failure below deletes it)
  h->device = device;
  srrg2_gridmap_default_params(&h->p);
  int rc;
  if ((rc = srrg2_scene_create(2, device, &h->work))) return rc;
  HIP_TRY(hipEventCreateWithFlags(&h->uploaded, hipEventDisableTiming));
  if ((rc = h->ctr.reserve(C_WORDS)) || (rc = h->ctr_host.reserve(C_WORDS))) return rc;
  *out = h.release();
  return 0;
}

extern "C" int srrg2_gridmap_destroy(srrg2_gridmap_h h) {
  delete h;  // (null: nothing to do)
  return 0;
}

extern "C" void srrg2_gridmap_default_params(srrg2_gridmap_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->resolution = 0.05f;
}

extern "C" void srrg2_gridmap_default_scan_params(srrg2_gridmap_scan_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->range_min = 0.05f;
  p->range_max = 30.f;
  p->sensor_in_robot[0] = p->sensor_in_robot[4] = p->sensor_in_robot[8] = 1.f;
  p->clear_beyond_max = 1;
}

extern "C" int srrg2_gridmap_reset(srrg2_gridmap_h h, const srrg2_gridmap_params* p) {
  const std::string who = "gridmap_reset: ";
  int rc;
  if ((rc = check_grid_params(who, p))) return rc;  // (the parameters first: what they are refused for needs no handle)
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t) p->rows * (size_t) p->cols;
  HIP_TRY(hipStreamSynchronize(h->stream()));  // (queued work still adds into the old planes)
  h->is_set = false, h->stale_field();  // (the likelihood field of the old planes is nobody's, and so are its bound planes)
  if ((rc = h->planes.reserve(2 * n + 4))) return rc;
  if (n > 0) HIP_TRY(hipMemsetAsync(h->planes.p, 0, 2 * n * sizeof(int), h->stream()));
  h->p      = *p;
  h->is_set = true;
  return 0;
}

extern "C" int srrg2_gridmap_integrate_scans(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* robot_in_world, int mem,
                                             const srrg2_gridmap_scan_params* p, int weight, srrg2_gridmap_result* out) {
  const std::string who = "gridmap_integrate_scans: ";
  int rc;
  if ((rc = gridmap_check_scan_call(who, ranges, num_scans, robot_in_world, mem, p, weight))) return rc;
  if ((rc = gridmap_ready(who, h))) return rc;
  // (float32, as the rays are: NaN -- an infinite range_max -- is refused too)
  if (!(p->range_max / h->p.resolution <= GRIDMAP_MAX_STEPS))
    return fail(SRRG2_E_INVALID, who + "range_max / resolution beyond 32000 cells");
  h->stale_field();  // every accepted call: the likelihood field (and its bound planes) has to be built again before the next match
  const long long total = (long long) num_scans * p->num_beams;
  srrg2_gridmap_result res;
  std::memset(&res, 0, sizeof(res));
  res.num_beams_total = total;
  if (total == 0) {
    if (out) *out = res;
    return 0;
  }
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  BeamArgs B;
  std::memset(&B, 0, sizeof(B));
  B.ranges = ranges, B.poses = robot_in_world;
  if (mem == SRRG2_MEM_HOST) {  // ONE upload: the ranges, then the poses, through the pinned block
    const size_t br = (size_t) total * 4, bp = (size_t) num_scans * 36;
    if (h->upload_pending) {
      HIP_TRY(hipEventSynchronize(h->uploaded));
      h->upload_pending = false;
    }
    if ((rc = h->host_stage.reserve(br + bp, (br + bp) / 8)) || (rc = h->stage.reserve(br + bp))) return rc;
    std::memcpy(h->host_stage.p, ranges, br);
    std::memcpy(h->host_stage.p + br, robot_in_world, bp);
    HIP_TRY(hipMemcpyAsync(h->stage.p, h->host_stage.p, br + bp, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(h->uploaded, st));
    h->upload_pending = true;
    B.ranges = reinterpret_cast<const float*>(h->stage.p);
    B.poses  = reinterpret_cast<const float*>(h->stage.p + br);
  }
  B.total = total, B.nb = p->num_beams;
  B.amin = p->angle_min, B.ainc = p->angle_increment;
  B.rmin = p->range_min, B.rmax = p->range_max;
  std::memcpy(B.S, p->sensor_in_robot, sizeof(B.S));
  B.clear = p->clear_beyond_max, B.weight = weight;
  HIP_TRY(hipMemsetAsync(h->ctr.p, 0, C_WORDS * sizeof(unsigned long long), st));
  const int blocks = (int) std::min<long long>((total + 255) / 256, MAX_BLOCKS);
  hipLaunchKernelGGL(k_gridmap_integrate<SRRG2_GRIDMAP_WAVE_MERGE != 0>, dim3(blocks), dim3(256), 0, st, grid_args(h), B, h->ctr.p);
  HIP_TRY(hipGetLastError());
  if (!out) return 0;
  HIP_TRY(hipMemcpyAsync(h->ctr_host.p, h->ctr.p, C_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait
  h->upload_pending = false;
  const unsigned long long* c = h->ctr_host.p;
  res.num_returns      = (int64_t) c[C_RETURNS];
  res.num_cleared_only = (int64_t) c[C_CLEARED];
  res.num_skipped      = total - res.num_returns - res.num_cleared_only;
  res.num_hits_in_grid = (int64_t) c[C_HITS];
  res.num_miss_updates = (int64_t) c[C_MISSES];
  *out = res;
  return 0;
}

extern "C" int srrg2_gridmap_get_counts(srrg2_gridmap_h h, int32_t* hits, int32_t* misses, int mem) {
  const std::string who = "gridmap_get_counts: ";
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  int rc;
  if ((rc = gridmap_ready(who, h))) return rc;
  const size_t n = (size_t) h->cells();
  if (n == 0 || (!hits && !misses)) return 0;
  HIP_TRY(hipSetDevice(h->device));
  const hipMemcpyKind kind = mem == SRRG2_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (hits) HIP_TRY(hipMemcpyAsync(hits, h->planes.p, n * sizeof(int), kind, h->stream()));
  if (misses) HIP_TRY(hipMemcpyAsync(misses, h->planes.p + n, n * sizeof(int), kind, h->stream()));
  HIP_TRY(hipStreamSynchronize(h->stream()));
  h->upload_pending = false;
  return 0;
}

extern "C" int srrg2_gridmap_device_arrays(srrg2_gridmap_h h, const int32_t** hits, const int32_t** misses) {
  const std::string who = "gridmap_device_arrays: ";
  if (!hits || !misses) return fail(SRRG2_E_INVALID, who + "null output");
  int rc;
  if ((rc = gridmap_ready(who, h))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream()));  // (the arrays go to another stream: queued work has to be done)
  h->upload_pending = false;
  *hits   = h->planes.p;
  *misses = h->planes.p + h->cells();
  return 0;
}

extern "C" int srrg2_gridmap_render(srrg2_gridmap_h h, int min_observations, uint8_t* dst, int row_stride_bytes, int mem) {
  const std::string who = "gridmap_render: ";
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  int rc;
  if ((rc = gridmap_ready(who, h))) return rc;
  const int rows = h->p.rows, cols = h->p.cols;
  if (h->cells() == 0) return 0;
  if (!dst) return fail(SRRG2_E_INVALID, who + "null image");
  if (row_stride_bytes < cols) return fail(SRRG2_E_INVALID, who + "row stride smaller than a row");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  unsigned char* target = dst;
  long long stride      = row_stride_bytes;
  const size_t packed   = ((size_t) cols + 3) / 4 * 4;  // rows of a staged image: packed up to a word
  if (mem == SRRG2_MEM_HOST) {
    if ((rc = h->image.reserve(packed * (size_t) rows))) return rc;
    target = h->image.p, stride = (long long) packed;
  }
  const int quads = (cols + 3) / 4;
  const long long need = std::max(min_observations, 1);
  hipLaunchKernelGGL(k_gridmap_render, dim3(blocks_of((long long) rows * quads)), dim3(256), 0, st, grid_args(h), need, quads, target,
                     stride);
  HIP_TRY(hipGetLastError());
  if (mem == SRRG2_MEM_HOST)
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t) row_stride_bytes, target, packed, (size_t) cols, (size_t) rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  h->upload_pending = false;
  return 0;
}

extern "C" int srrg2_gridmap_to_scene(srrg2_gridmap_h h, int min_observations, int occupied_percent, srrg2_scene_h dst) {
  const std::string who = "gridmap_to_scene: ";
  if (occupied_percent < 0 || occupied_percent > 100) return fail(SRRG2_E_INVALID, who + "occupied_percent 0 .. 100");
  int rc;
  if ((rc = gridmap_ready(who, h))) return rc;
  if (!dst) return fail(SRRG2_E_INVALID, who + "null scene");
  if (!srrg2amd::scene_clip_pair(h->work, dst)) return fail(SRRG2_E_INVALID, who + "dst must be a 2-D scene on the grid's device");
  srrg2_scene* const s = h->work;
  if ((rc = srrg2amd::scene_clip_begin(s, dst))) return rc;  // (dst: no normals, no features, empty until the call has succeeded)
  // (arrays even for an empty result, as the clippers leave them)
  if ((rc = srrg2amd::scene_make_room(dst, 1, 0)) || (rc = dst->gidx.reserve(1))) return rc;
  const long long cells = h->cells();
  if (cells == 0) return 0;
  const int n = (int) cells;  // (<= 2^30)
  if ((rc = s->flags.reserve((size_t) n + 1))) return rc;
  hipStream_t st   = h->stream();
  const GridArgs G = grid_args(h);
  const dim3 grid(blocks_of(n)), block(256);
  hipLaunchKernelGGL(k_gridmap_flag, grid, block, 0, st, G, (long long) std::max(min_observations, 1), (unsigned) occupied_percent, n,
                     s->flags.p);
  HIP_TRY(hipGetLastError());
  const auto scatter = [&](int cap) {
    hipLaunchKernelGGL(k_gridmap_scatter, grid, block, 0, st, G, n, s->flags.p, dst->pts.p, dst->nrm.p, dst->gidx.p, cap);
  };
  rc = srrg2amd::scene_compact_into(s, dst, n, scatter, nullptr);
  h->upload_pending = false;
  return rc;
}
