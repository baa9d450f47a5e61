// scene.hip -- scene slices kept in HBM between frames: ball, projective, scan and spherical clipping, correspondence-based merging
// (SURVEY.md section 8f row 2).  Replaces, behind the C ABI of include/srrg2_slam_amd.h:
//   MergerCorrespondenceHomo_::compute()   S/mapping/merger_correspondence_homo_impl.cpp:11-125
//   SceneClipper_::compute() (interface)   S/mapping/scene_clipper.h:17-122
//   the index flip + local->global mapping of TrackerSliceProcessor_::merge()
//                                          S/trackers/tracker_slice_processor_impl.cpp:160-186
// A scene is two float4 arrays (points {x, y, z, 0}, normals) with spare capacity and, for the clouds of a visual pipeline
// (PointIntensityDescriptor2f / 3f, the second instantiation of the merger: merger_correspondence_homo.h:36-40), a 256-bit
// descriptor (two uint4) and a float intensity per point, each allocated only when present.  The features travel with the point:
// the kernels that move points (k_scatter_kept, merge_one, k_append_scatter) have a feature-carrying instantiation, chosen on the
// host, so a scene without features runs the code it ran before they existed.  All kernels are one thread per
// point or correspondence, coalesced, HBM bound: clip = 2 passes over the scene (flag+count, scatter) around an
// exclusive scan (the view clips -- camera, scanner, lidar: ONE set of kernels over a View per sensor -- with occlusion: one more
// in front, the per-bin depth / range minimum); merge = one pass over the correspondences + (if the merge target was not reached) flag/scan/scatter
// of the measurement.  The reference merges sequentially; results are identical because
//   - a scene point hit by ONE correspondence is independent of all others (the common case: the tracker's
//     correspondences come through an injective local->global map),
//   - scene points hit by several correspondences are replayed in correspondence order by one thread per scene point
//     (k_merge_dups: the duplicates are grouped by a radix sort),
//   - appends keep measurement order (stable compaction by exclusive scan).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "det_math.h"
#include "device_types.h"
#include "device_util.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_device.h"
#include "scene_state.h"
#include "spherical.h"

using srrg2amd::DevBuf;
using srrg2amd::fail;

namespace {

struct Xf {  // rows of [R|t]; SE(2) spread into the same slots
  float m[12];
};

Xf load_transform(int dim, const float* T) {
  Xf x;
  if (dim == 3) {
    std::memcpy(x.m, T, sizeof(x.m));
  } else {
    const float v[12] = {T[0], T[1], 0.f, T[2], T[3], T[4], 0.f, T[5], 0.f, 0.f, 1.f, 0.f};
    std::memcpy(x.m, v, sizeof(v));
  }
  return x;
}

__device__ __forceinline__ bool valid_point(int dim, const float4 p) {
  return isfinite(p.x) && isfinite(p.y) && (dim == 2 || isfinite(p.z));
}

__device__ __forceinline__ float4 xform_point(int dim, const Xf& M, const float4 p) {
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (dim == 3) {
    q.x = ((M.m[0] * p.x + M.m[1] * p.y) + M.m[2] * p.z) + M.m[3];
    q.y = ((M.m[4] * p.x + M.m[5] * p.y) + M.m[6] * p.z) + M.m[7];
    q.z = ((M.m[8] * p.x + M.m[9] * p.y) + M.m[10] * p.z) + M.m[11];
  } else {
    q.x = (M.m[0] * p.x + M.m[1] * p.y) + M.m[3];
    q.y = (M.m[4] * p.x + M.m[5] * p.y) + M.m[7];
  }
  return q;
}

__device__ __forceinline__ float4 rotate_normal(int dim, const Xf& M, const float4 n) {
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (dim == 3) {
    r.x = (M.m[0] * n.x + M.m[1] * n.y) + M.m[2] * n.z;
    r.y = (M.m[4] * n.x + M.m[5] * n.y) + M.m[6] * n.z;
    r.z = (M.m[8] * n.x + M.m[9] * n.y) + M.m[10] * n.z;
  } else {
    r.x = M.m[0] * n.x + M.m[1] * n.y;
    r.y = M.m[4] * n.x + M.m[5] * n.y;
  }
  return r;
}

// ---- clip ---------------------------------------------------------------------------------------------------
// words of a scene's dscalars a clip uses: what the projective and the scan clip's flag kernels count, and behind them the
// scan's total, so that ONE copy brings all three to the host (compact_into)
enum { CLIP_VALID = 0, CLIP_IN_VIEW = 1, CLIP_TOTAL = 2 };

__device__ __forceinline__ bool clip_keep(int dim, const Xf& L, float range2, const float4 p) {
  if (!valid_point(dim, p)) return false;
  const float4 q = xform_point(dim, L, p);
  const float d2 = (q.x * q.x + q.y * q.y) + q.z * q.z;
  return d2 <= range2;
}

__global__ void k_clip_flag(int dim, Xf L, float range2, const float4* __restrict__ pts, int n, int* __restrict__ flags) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    flags[i] = clip_keep(dim, L, range2, pts[i]) ? 1 : 0;
}

// the points the scan kept (offset[i + 1] != offset[i]: the scan leaves its total in offset[n]) into the robot frame, in scene
// order: the scatter of all four clippers.  It evaluates no predicate, so whatever a flag kernel decided is what moves.
template <bool FEAT, int DIM>
__device__ __forceinline__ void scatter_kept(const Xf& L, const float4* __restrict__ pts, const float4* __restrict__ nrm, int n,
                                             const int* __restrict__ offset, float4* __restrict__ out_pts,
                                             float4* __restrict__ out_nrm, int* __restrict__ gidx, int cap, const Feat& f) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int k = offset[i];
    // not kept / no room yet (a scatter launched before the host knew the total: compact_into repeats it with room for all)
    if (offset[i + 1] == k || k >= cap) continue;
    out_pts[k] = xform_point(DIM, L, pts[i]);
    out_nrm[k] = nrm ? rotate_normal(DIM, L, nrm[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
    gidx[k]    = i;
    if (FEAT) move_features(f, i, k);
  }
}

template <bool FEAT>
__global__ void k_scatter_kept(int dim, Xf L, const float4* __restrict__ pts, const float4* __restrict__ nrm, int n,
                               const int* __restrict__ offset, float4* __restrict__ out_pts, float4* __restrict__ out_nrm,
                               int* __restrict__ gidx, int cap, Feat f) {
  if (dim == 3)
    scatter_kept<FEAT, 3>(L, pts, nrm, n, offset, out_pts, out_nrm, gidx, cap, f);
  else
    scatter_kept<FEAT, 2>(L, pts, nrm, n, offset, out_pts, out_nrm, gidx, cap, f);
}

// ---- view clips (no reference counterpart: SceneClipper_ is an interface; DESIGN.md section 4 "Projective clipping", "Scan
// clipping", "Lidar sweeps") --------------------------------------------------------------------------------------------------
// keep the Valid points a sensor at sensor_in_robot sees: inside its depth / range interval and its image or sector, and --
// margin >= 0 -- no further than `margin` behind the nearest point of their bin (a camera's or a lidar's pixel, a scanner's beam).
// A sensor is a View: L, S, the geometry and the margin, by value as the first kernel argument, and ONE device function,
// project(): point -> bin, or -1 when not in view, plus `valid` and the depth / range (written when it was computed).  RING_WORDS
// doubles of LDS are the view's to fill once per workgroup (stage()) and to read in project().  The kernels over a view:
//   k_view_min         per bin the minimum depth / range of the in-view points: positive floats order like their bit patterns,
//                      so ONE 32-bit atomicMin per in-view point (no return value, order-free: deterministic)
//   k_view_min_lds     the same through a workgroup's private LDS table (the scan clip, below)
//   k_view_flag        keep flag per point + the Valid / in-view counts (one atomic per block and count)
//   k_view_min_staged  k_view_min that also counts and leaves (bin, depth bits) per point for k_spclip_flag_staged (the lidar, below)
// and k_scatter_kept moves what the scan kept: the same L and xform_point as for the ball clip, so the same bits; it reads the
// scan's neighbouring offsets and never projects
struct ViewBase {  // what every view has; no ring table
  Xf L, S;
  static constexpr int RING_WORDS = 1;
  __device__ __forceinline__ void stage(double*) const {}
};

// -- pinhole camera
struct ProjCam {
  float K0, K2, K4, K5, depth_min, depth_max, margin;
  int rows, cols;
};

// steps 1-4 of the contract: Valid, r = L p, c = S r, project_point of the projective finder (kernels.hip).  -1: not in view
__device__ __forceinline__ int pclip_project(const Xf& L, const Xf& S, const ProjCam& C, const float4 p, bool& valid, float& cz) {
  valid = valid_point(3, p);
  if (!valid) return -1;
  const float4 c = xform_point(3, S, xform_point(3, L, p));
  if (!(isfinite(c.x) && isfinite(c.y) && isfinite(c.z))) return -1;
  if (!(c.z >= C.depth_min) || !(c.z <= C.depth_max)) return -1;
  const float u  = (C.K0 * c.x) / c.z + C.K2;
  const float v  = (C.K4 * c.y) / c.z + C.K5;
  const float uf = u + 0.5f, vf = v + 0.5f;
  if (!(uf >= 0.f) || !(uf < (float) C.cols) || !(vf >= 0.f) || !(vf < (float) C.rows)) return -1;
  cz = c.z;
  return (int) floorf(vf) * C.cols + (int) floorf(uf);
}

struct PinholeView : ViewBase {
  ProjCam C;
  __device__ __forceinline__ float margin() const { return C.margin; }
  __device__ __forceinline__ int project(const double*, const float4 p, bool& valid, float& cz) const {
    return pclip_project(L, S, C, p, valid, cz);
  }
};

// -- planar laser scanner (2-D): the bins are the beams of its angular sector.
// A scan has ~10^3 beams, a map 10^5..10^6 points: hundreds of points per word, and same-address global atomics serialise
// (block_add, device_util.h).  So with occlusion every workgroup takes the minimum in a private LDS table of num_beams words first
// (k_view_min_lds: ds atomics, no return value) and sends ONE global atomicMin per bin it touched.  k_view_min, straight into
// global memory, remains for tables beyond SRRG2_SCLIP_LDS_BINS and maps too small to give SRRG2_SCLIP_LDS_MIN_WORKGROUPS
// workgroups their share.  A minimum does not depend on who took it: both give the same bits.
struct ScanGeom {
  double angle_min, angle_increment, wrap;  // wrap = copysign(2 pi, angle_increment)
  float range_min, range_max, margin;
  int num_beams;
};

// 8192 bins = 32 KB: four workgroups of 256 threads still share a CU's 160 KB of LDS, and every planar scanner in use
// (360 .. 2 x 1440 beams) fits several times over
#ifndef SRRG2_SCLIP_LDS_BINS
#define SRRG2_SCLIP_LDS_BINS 8192
#endif
// points per workgroup and bin under which the table's initialisation and flush outweigh what it saves
#ifndef SRRG2_SCLIP_POINTS_PER_BIN
#define SRRG2_SCLIP_POINTS_PER_BIN 4
#endif
// ... and the workgroups that rule must leave for the table to pay: with fewer, the few that remain walk their points one
// float64 atan2 after the other while most of the chip idles (measured, 1081 beams: 11 workgroups 0.067 ms against 0.060 ms
// of global atomics for the whole clip, 23 workgroups equal, 46 and more ahead)
#ifndef SRRG2_SCLIP_LDS_MIN_WORKGROUPS
#define SRRG2_SCLIP_LDS_MIN_WORKGROUPS 20
#endif

// steps 1-5 of the contract: Valid, r = L p, c = S r, range, beam.  -1: not in view
__device__ __forceinline__ int sclip_beam(const Xf& L, const Xf& S, const ScanGeom& G, const float4 p, bool& valid, float& rho) {
  valid = valid_point(2, p);
  if (!valid) return -1;
  const float4 c = xform_point(2, S, xform_point(2, L, p));
  if (!(isfinite(c.x) && isfinite(c.y))) return -1;
  rho = sqrtf(c.x * c.x + c.y * c.y);
  if (!(rho >= G.range_min) || !(rho <= G.range_max)) return -1;
  const double beta = dm::atan2((double) c.y, (double) c.x);
  const double d    = beta - G.angle_min;
  double t          = d / G.angle_increment;
  if (t < -0.5)
    t = (d + G.wrap) / G.angle_increment;
  else if (t >= (double) G.num_beams - 0.5)
    t = (d - G.wrap) / G.angle_increment;
  const double tf = t + 0.5;
  if (!(tf >= 0.0) || !(tf < (double) G.num_beams)) return -1;
  return (int) floor(tf);  // in [0, num_beams)
}

struct BeamView : ViewBase {
  ScanGeom G;
  __device__ __forceinline__ float margin() const { return G.margin; }
  __device__ __forceinline__ int project(const double*, const float4 p, bool& valid, float& rho) const {
    return sclip_beam(L, S, G, p, valid, rho);
  }
};

// -- spinning lidar (3-D): the bins are the pixels of the rows x cols range image of its spherical model (spherical.h, shared
// with the sweep adaptor).  The image of a 64 x 2048 sensor has 131072 words, sixteen times SRRG2_SCLIP_LDS_BINS, and a map puts
// a handful of points on each, so there is no LDS table.  With occlusion the minimum pass is k_view_min_staged and the flag pass
// reads what it left -- the projection is two float64 atan2, a square root and four divisions, more than the 16 bytes per point
// of writing it down and reading it back (docs/HISTORY.md has both timings).  Without, k_view_flag projects and counts itself.
// RINGS: the rows of a ring table (B: the boundaries in LDS, sph::stage_rings) instead of the model's uniform rows
template <bool RINGS>
__device__ __forceinline__ int spclip_project(const Xf& L, const Xf& S, const sph::Geom& G, const double* B, int descending,
                                              const float4 p, bool& valid, float& rho) {
  valid = valid_point(3, p);
  if (!valid) return -1;
  const float4 c = xform_point(3, S, xform_point(3, L, p));
  if (!(isfinite(c.x) && isfinite(c.y) && isfinite(c.z))) return -1;
  double tf;
  return sph::project_t<RINGS>(G, B, descending, c.x, c.y, c.z, rho, tf);
}

struct LidarView : ViewBase {  // the model's uniform rows: no 2 KB table in the kernel arguments
  sph::Geom G;
  float occlusion_margin;
  __device__ __forceinline__ float margin() const { return occlusion_margin; }
  __device__ __forceinline__ int project(const double*, const float4 p, bool& valid, float& rho) const {
    return spclip_project<false>(L, S, G, nullptr, 0, p, valid, rho);
  }
};

// a sensor with a ring table (srrg2_scene_clip_spherical_rings): the boundaries travel by value and are staged into LDS once per
// workgroup
struct RingLidarView : LidarView {
  sph::Rings T;
  static constexpr int RING_WORDS = sph::MAX_RING_ROWS + 1;
  __device__ __forceinline__ void stage(double* B) const { sph::stage_rings(T, B); }
  __device__ __forceinline__ int project(const double* B, const float4 p, bool& valid, float& rho) const {
    return spclip_project<true>(L, S, G, B, T.descending, p, valid, rho);
  }
};

// -- the kernels over a view (a view without a ring table leaves `rings` unused: the compiler drops it)
template <typename V>
__global__ void k_view_min(V v, const float4* __restrict__ pts, int n, unsigned* __restrict__ dmin) {
  __shared__ double rings[V::RING_WORDS];
  v.stage(rings);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool valid;
    float d;
    const int bin = v.project(rings, pts[i], valid, d);
    if (bin >= 0) atomicMin(&dmin[bin], __float_as_uint(d));  // (bin < the table's size: project's bounds)
  }
}

// dynamic LDS: `bins` words (the host launches it only with bins <= SRRG2_SCLIP_LDS_BINS)
template <typename V>
__global__ void k_view_min_lds(V v, int bins, const float4* __restrict__ pts, int n, unsigned* __restrict__ dmin) {
  extern __shared__ unsigned table[];
  __shared__ double rings[V::RING_WORDS];
  v.stage(rings);
  const unsigned INF = 0x7f800000u;
  for (int b = threadIdx.x; b < bins; b += blockDim.x) table[b] = INF;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool valid;
    float d;
    const int bin = v.project(rings, pts[i], valid, d);
    if (bin >= 0) atomicMin(&table[bin], __float_as_uint(d));
  }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += blockDim.x) {
    const unsigned m = table[b];
    if (m != INF) atomicMin(&dmin[b], m);
  }
}

// counters: [CLIP_VALID], [CLIP_IN_VIEW]
template <typename V, bool OCCLUSION>
__global__ void k_view_flag(V v, const float4* __restrict__ pts, int n, const unsigned* __restrict__ dmin, int* __restrict__ flags,
                            int* __restrict__ counters) {
  __shared__ double rings[V::RING_WORDS];
  v.stage(rings);
  int nvalid = 0, nview = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool valid;
    float d;
    const int bin = v.project(rings, pts[i], valid, d);
    bool keep     = bin >= 0;
    nvalid += valid ? 1 : 0;
    nview += keep ? 1 : 0;
    if (OCCLUSION && keep) keep = d <= __uint_as_float(dmin[bin]) + v.margin();
    flags[i] = keep ? 1 : 0;
  }
  block_add(nvalid, &counters[CLIP_VALID]);
  block_add(nview, &counters[CLIP_IN_VIEW]);
}

// counters: [CLIP_VALID], [CLIP_IN_VIEW]
template <typename V>
__global__ void k_view_min_staged(V v, const float4* __restrict__ pts, int n, unsigned* __restrict__ dmin, uint2* __restrict__ stage,
                                  int* __restrict__ counters) {
  __shared__ double rings[V::RING_WORDS];
  v.stage(rings);
  int nvalid = 0, nview = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    bool valid;
    float d       = 0.f;
    const int bin = v.project(rings, pts[i], valid, d);
    nvalid += valid ? 1 : 0;
    nview += bin >= 0 ? 1 : 0;
    if (bin >= 0) atomicMin(&dmin[bin], __float_as_uint(d));  // (bin < the table's size: project's bounds)
    stage[i] = make_uint2((unsigned) bin, __float_as_uint(d));
  }
  block_add(nvalid, &counters[CLIP_VALID]);
  block_add(nview, &counters[CLIP_IN_VIEW]);
}

// the flag pass behind k_view_min_staged: reads what that pass left per point
__global__ void k_spclip_flag_staged(const uint2* __restrict__ stage, int n, const unsigned* __restrict__ rmin, float margin,
                                     int* __restrict__ flags) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint2 s = stage[i];
    const int pix = (int) s.x;
    flags[i]      = pix >= 0 && __uint_as_float(s.y) <= __uint_as_float(rmin[pix]) + margin ? 1 : 0;
  }
}


// ---- merge --------------------------------------------------------------------------------------------------
// one correspondence: merger_correspondence_homo_impl.cpp:55-76.  Returns true if merged.
template <bool FEAT>
__device__ __forceinline__ bool merge_one(int dim, const Xf& M, float max_response, float max_d2, float4* scene_pts,
                                          float4* scene_nrm, const float4* meas_pts, const float4* meas_nrm, int s, int m,
                                          float response, const Feat& f) {
  if (!(response < max_response)) return false;  // :60
  const float4 ps = scene_pts[s];
  const float4 q  = xform_point(dim, M, meas_pts[m]);  // :62-63
  const float dx = q.x - ps.x, dy = q.y - ps.y, dz = q.z - ps.z;
  const float d2 = (dx * dx + dy * dy) + dz * dz;  // :66-67
  if (!(d2 < max_d2)) return false;                // :69
  // :71 point_scene = point_meas (all fields: the normal stays in the measurement frame), :74 mean coordinates
  if (scene_nrm) scene_nrm[s] = meas_nrm ? meas_nrm[m] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 r = make_float4((q.x + ps.x) * 0.5f, (q.y + ps.y) * 0.5f, dim == 3 ? (q.z + ps.z) * 0.5f : 0.f, 0.f);
  scene_pts[s] = r;
  if (FEAT) move_features(f, m, s);  // :71 again: descriptor and intensity are fields of the measurement point
  return true;
}

__global__ void k_merge_count(const srrg2_correspondence* __restrict__ corr, int ncorr, int n_scene, int n_meas,
                              int* __restrict__ counts, int* __restrict__ scalars) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncorr; c += gridDim.x * blockDim.x) {
    const srrg2_correspondence k = corr[c];
    if (k.fixed_idx < 0 || k.fixed_idx >= n_scene || k.moving_idx < 0 || k.moving_idx >= n_meas) {
      scalars[2] = 1;  // the reference asserts (:53-54); here: error
      continue;
    }
    if (atomicAdd(&counts[k.fixed_idx], 1) >= 1) scalars[3] = 1;  // some scene point is hit more than once
  }
}

// scene points hit exactly once: independent of every other correspondence
template <bool FEAT>
__global__ void k_merge_apply(int dim, Xf M, float max_response, float max_d2, const srrg2_correspondence* __restrict__ corr,
                              int ncorr, const int* __restrict__ counts, float4* scene_pts, float4* scene_nrm,
                              const float4* __restrict__ meas_pts, const float4* __restrict__ meas_nrm,
                              unsigned char* __restrict__ merged, int* __restrict__ dup_flags, Feat f) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncorr; c += gridDim.x * blockDim.x) {
    const srrg2_correspondence k = corr[c];
    const bool dup               = counts[k.fixed_idx] > 1;
    if (dup_flags) dup_flags[c] = dup ? 1 : 0;
    if (dup) continue;
    if (merge_one<FEAT>(dim, M, max_response, max_d2, scene_pts, scene_nrm, meas_pts, meas_nrm, k.fixed_idx, k.moving_idx, k.response, f))
      merged[k.moving_idx] = 1;
  }
}

__global__ void k_compact_dups(const int* __restrict__ dup_flags_scanned, const srrg2_correspondence* __restrict__ corr,
                               int ncorr, const int* __restrict__ counts, int* __restrict__ dup_list) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncorr; c += gridDim.x * blockDim.x)
    if (counts[corr[c].fixed_idx] > 1) dup_list[dup_flags_scanned[c]] = c;
}

// scene points hit several times: replay their correspondences in order (:51 "for all correspondences").  Different
// scene points do not interact, so the duplicates are grouped by scene point -- a radix sort of the keys
// (scene index << 32 | correspondence index): groups come out contiguous, each in correspondence order -- and ONE THREAD
// PER DISTINCT SCENE POINT replays its group (a single thread walking the whole list paid one memory latency per entry).
__global__ void k_dup_keys(const srrg2_correspondence* __restrict__ corr, const int* __restrict__ dup_list, int ndup,
                           unsigned long long* __restrict__ keys) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ndup; t += gridDim.x * blockDim.x) {
    const int c = dup_list[t];
    keys[t]     = ((unsigned long long) (unsigned) corr[c].fixed_idx << 32) | (unsigned) c;
  }
}

template <bool FEAT>
__global__ void k_merge_dups(int dim, Xf M, float max_response, float max_d2, const srrg2_correspondence* __restrict__ corr,
                             const unsigned long long* __restrict__ keys, int ndup, float4* scene_pts, float4* scene_nrm,
                             const float4* __restrict__ meas_pts, const float4* __restrict__ meas_nrm,
                             unsigned char* __restrict__ merged, Feat f) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ndup; t += gridDim.x * blockDim.x) {
    const unsigned s = (unsigned) (keys[t] >> 32);
    if (t > 0 && (unsigned) (keys[t - 1] >> 32) == s) continue;  // not the first of its group
    for (int j = t; j < ndup && (unsigned) (keys[j] >> 32) == s; ++j) {
      const srrg2_correspondence k = corr[(unsigned) keys[j]];
      if (merge_one<FEAT>(dim, M, max_response, max_d2, scene_pts, scene_nrm, meas_pts, meas_nrm, k.fixed_idx, k.moving_idx, k.response, f))
        merged[k.moving_idx] = 1;
    }
  }
}

// the tracker's path: correspondences straight from the aligner's per-point arrays (sorted order of its moving cloud =
// the clipped scene), flipped and mapped to the global scene (tracker_slice_processor_impl.cpp:175-181).  The map is
// injective, so every scene point is hit at most once: no ordering to respect.
template <bool FEAT>
__global__ void k_merge_from_aligner(int dim, Xf M, float max_response, float max_d2, const float4* __restrict__ moving_sorted,
                                     const int* __restrict__ corr_fixed, const float* __restrict__ corr_resp,
                                     const unsigned char* __restrict__ corr_stat, int prune, int nm,
                                     const int* __restrict__ gidx, int n_scene, int n_meas, float4* scene_pts,
                                     float4* scene_nrm, const float4* __restrict__ meas_pts,
                                     const float4* __restrict__ meas_nrm, unsigned char* __restrict__ merged,
                                     int* __restrict__ scalars, Feat f) {
  int ncorr = 0, nmerged = 0;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < nm; g += gridDim.x * blockDim.x) {
    const int m = corr_fixed[g];  // aligner "fixed" = the measurement
    if (m < 0) continue;
    if (prune && corr_stat[g] != SRRG2_FACTOR_INLIER) continue;  // as srrg2_aligner_get_correspondences
    const int local = __float_as_int(moving_sorted[g].w);        // aligner "moving" = the clipped scene
    const int s     = gidx[local];
    if (m >= n_meas || s < 0 || s >= n_scene) {
      scalars[2] = 1;
      continue;
    }
    ++ncorr;
    if (merge_one<FEAT>(dim, M, max_response, max_d2, scene_pts, scene_nrm, meas_pts, meas_nrm, s, m, corr_resp[g], f)) {
      // (several scene points may merge into one measurement point: its flag byte is set through an atomic OR on the word that
      // holds it, and whoever finds it clear counts it -- the number of DISTINCT merged points without a second pass over the
      // flags, k_count_merged, and its launch, copy and wait: a tracker's merge 0.088 -> ~0.07 ms)
      unsigned* w        = reinterpret_cast<unsigned*>(merged) + (m >> 2);
      const unsigned bit = 1u << ((m & 3) * 8);
      if (!(atomicOr(w, bit) & bit)) ++nmerged;
    }
  }
  block_add(ncorr, &scalars[4]);
  block_add(nmerged, &scalars[1]);
}

__global__ void k_count_merged(const unsigned char* __restrict__ merged, int n, int* __restrict__ scalars) {
  int c = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) c += merged[i] ? 1 : 0;
  block_add(c, &scalars[1]);
}

// append: flags (unmerged && Valid) -> exclusive scan -> scatter in measurement order (:100-114, :33-40)
__global__ void k_append_flag(int dim, const float4* __restrict__ meas_pts, const unsigned char* __restrict__ merged, int n,
                              int* __restrict__ flags) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    flags[i] = (!(merged && merged[i]) && valid_point(dim, meas_pts[i])) ? 1 : 0;
}

template <bool FEAT>
__global__ void k_append_scatter(int dim, Xf M, const float4* __restrict__ meas_pts, const float4* __restrict__ meas_nrm,
                                 const unsigned char* __restrict__ merged, int n, const int* __restrict__ offset, int base,
                                 float4* __restrict__ scene_pts, float4* __restrict__ scene_nrm, Feat f) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = meas_pts[i];
    if ((merged && merged[i]) || !valid_point(dim, p)) continue;
    const int k  = base + offset[i];
    scene_pts[k] = xform_point(dim, M, p);  // transformInPlace: coordinates and normal
    scene_nrm[k] = meas_nrm ? rotate_normal(dim, M, meas_nrm[i]) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (FEAT) move_features(f, i, k);  // (descriptors and intensities are frame-free: appended unchanged)
  }
}

// set_features: descriptor rows of any stride and alignment -> two uint4 per point.  One thread per 32-bit word, read as bytes.
__global__ void k_ingest_descriptors(const unsigned char* __restrict__ src, size_t stride, int n, unsigned* __restrict__ dst) {
  const size_t words = (size_t) n * 8;
  for (size_t w = (size_t) blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (size_t) gridDim.x * blockDim.x) {
    const unsigned char* b = src + (w >> 3) * stride + (w & 7) * 4;
    dst[w] = (unsigned) b[0] | ((unsigned) b[1] << 8) | ((unsigned) b[2] << 16) | ((unsigned) b[3] << 24);
  }
}

__global__ void k_ingest_intensity(const float* __restrict__ src, size_t stride_floats, int n, float* __restrict__ dst) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[(size_t) i * stride_floats];
}

// the device of the scene made current, and whatever an adaptor left queued on its stream finished: every entry point that reads
// or rewrites a scene starts here (several of them read it on another scene's stream or through the null stream)
int scene_device(srrg2_scene* s) {
  HIP_TRY(hipSetDevice(s->device));
  if (s->pending) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->pending = false;
  }
  return 0;
}

// the feature-carrying instantiation of a kernel when the call moves features, else the plain one
#define LAUNCH_FEAT(kernel, feat, grid, stream, ...)                                    \
  do {                                                                                  \
    if (feat)                                                                           \
      hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, stream, __VA_ARGS__);        \
    else                                                                                \
      hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, stream, __VA_ARGS__);       \
  } while (0)

// features of `src` points written into `dst` (the fields `dst` carries; the callers have made both agree)
Feat feat_of(const srrg2_scene* src, const srrg2_scene* dst) {
  return Feat{dst->has_desc ? src->desc.p : nullptr, dst->has_inten ? src->inten.p : nullptr,
              dst->has_desc ? dst->desc.p : nullptr, dst->has_inten ? dst->inten.p : nullptr};
}

bool moves_features(const Feat& f) { return f.dst_desc || f.dst_inten; }

// a feature array follows the capacity of the point arrays (per_point elements each), keeping the first `keep` points' entries
template <typename T>
int grow_feature(srrg2_scene* s, DevBuf<T>& buf, size_t per_point, int keep) {
  return buf.grow(s->pts.cap * per_point, std::min((size_t) (keep > 0 ? keep : 0) * per_point, buf.cap), s->stream);
}

int features_reserve(srrg2_scene* s, int keep) {
  int rc;
  if (s->has_desc && (rc = grow_feature(s, s->desc, 2, keep))) return rc;
  if (s->has_inten && (rc = grow_feature(s, s->inten, 1, keep))) return rc;
  return 0;
}

// "homo": scene and measurement are clouds of ONE point type.  An empty scene takes the measurement's; otherwise the fields
// must agree.  Called before a merge changes anything.
int bind_features(srrg2_scene* scene, const srrg2_scene* meas, const char* who) {
  if (scene->n == 0) {
    scene->has_desc  = meas->has_desc;
    scene->has_inten = meas->has_inten;
    return features_reserve(scene, 0);
  }
  if (scene->has_desc != meas->has_desc || scene->has_inten != meas->has_inten)
    return fail(SRRG2_E_STATE, std::string(who) + ": scene and measurement disagree on descriptors / intensity (one point type "
                                                  "per merger: merger_correspondence_homo.h:36-40)");
  return 0;
}

// grow the point arrays (and the feature arrays that are present) to hold n points, keeping the first `keep`
int scene_reserve(srrg2_scene* s, int n, int keep) {
  s->pyr_levels = 0;  // (the content is about to be rewritten: it is no pyramid adaptor's any more)
  if ((size_t) n <= s->pts.cap && (size_t) n <= s->nrm.cap) return features_reserve(s, keep);
  int rc;
  const size_t want = (size_t) n + (size_t) n / 2 + 1024, kept = (size_t) (keep > 0 ? keep : 0);
  if ((rc = s->pts.grow(want, kept, s->stream)) || (rc = s->nrm.grow(want, kept, s->stream))) return rc;
  return features_reserve(s, keep);
}

// flags[0..n) -> exclusive scan in place; total in scalars[0] (host value returned)
int scan_flags(srrg2_scene* s, int n, int* total) {
  int rc;
  if ((rc = s->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(n) + 2))) return rc;
  srrg2amd::launch_exclusive_scan(s->flags.p, n, s->scan_sums.p, s->scan_sums.p + s->scan_sums.cap - 1, s->stream);
  HIP_TRY(hipMemcpyAsync(&s->scalars.p[0], s->scan_sums.p + s->scan_sums.cap - 1, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *total = s->scalars.p[0];
  return 0;
}

int read_scalars(srrg2_scene* s, const int* from = nullptr) {
  HIP_TRY(hipMemcpyAsync(s->scalars.p, from ? from : s->dscalars.p, 16 * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

// two distinct scenes of one dim on one device: what a clipper reads and what it writes
bool clip_pair(const srrg2_scene* full, const srrg2_scene* clipped) {
  return full && clipped && full != clipped && full->dim == clipped->dim && full->device == clipped->device;
}

// both scenes current and quiet; `clipped` takes the fields of `full` and is empty until the clip has succeeded
int clip_begin(srrg2_scene* full, srrg2_scene* clipped) {
  int rc;
  if ((rc = scene_device(clipped)) || (rc = scene_device(full))) return rc;
  clipped->has_normals = full->has_normals;
  clipped->has_desc    = full->has_desc;
  clipped->has_inten   = full->has_inten;
  clipped->n = clipped->ng = 0;
  return 0;
}

void launch_scatter_kept(srrg2_scene* full, srrg2_scene* clipped, const Xf& L, int n, int cap) {
  const Feat f = feat_of(full, clipped);
  LAUNCH_FEAT(k_scatter_kept, moves_features(f), dim3(blocks_for(n)), full->stream, full->dim, L, full->pts.p,
              full->has_normals ? full->nrm.p : nullptr, n, full->flags.p, clipped->pts.p, clipped->nrm.p, clipped->gidx.p, cap, f);
}

// The tail of every clipper: the n > 0 keep flags a flag kernel has queued in full->flags (n + 1 words reserved) -> `clipped`,
// the kept points by L in scene order; full->scalars[CLIP_VALID .. CLIP_TOTAL] on the host when it returns.
// A clipped scene that has room from the call before (a tracker clips around a pose that moves a little per frame): the scatter
// is launched BEHIND the scan without the host having seen the total -- one wait per clip instead of two (0.046 -> ~0.03 ms for a
// 100 k-point map); the kernel's k >= cap guard keeps it inside the room, and a total beyond the room repeats it with room for
// all (the scan runs once: its offsets still stand).
int compact_scatter(srrg2_scene* full, srrg2_scene* clipped, int n, const std::function<void(int cap)>& scatter,
                    const std::function<int()>& before_wait) {
  int rc;
  hipStream_t st = full->stream;
  if ((rc = full->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(n)))) return rc;
  srrg2amd::launch_exclusive_scan(full->flags.p, n, full->scan_sums.p, full->dscalars.p + CLIP_TOTAL, st);
  if ((rc = features_reserve(clipped, 0))) return rc;  // (room for features wherever there is room for points)
  const int room = (int) std::min({clipped->pts.cap, clipped->nrm.cap, clipped->gidx.cap});
  if (room > 0) scatter(room);
  if (before_wait && (rc = before_wait())) return rc;
  HIP_TRY(hipMemcpyAsync(full->scalars.p, full->dscalars.p, (CLIP_TOTAL + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  const int total = full->scalars.p[CLIP_TOTAL];
  if (total > room) {
    if ((rc = scene_reserve(clipped, total, 0)) || (rc = clipped->gidx.reserve((size_t) total))) return rc;
    scatter(total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
  }
  clipped->n = clipped->ng = total;
  return 0;
}

int compact_into(srrg2_scene* full, srrg2_scene* clipped, const Xf& L, int n) {
  return compact_scatter(full, clipped, n, [&](int cap) { launch_scatter_kept(full, clipped, L, n, cap); }, nullptr);
}

// The three view clippers between their validation and their return.  `passes(grid, counters)` queues on full->stream what
// leaves the n keep flags in full->flags and the Valid / in-view counts in counters[CLIP_VALID], [CLIP_IN_VIEW] (cleared here).
// `dmin`: the table of `bins` per-bin minima, reserved and filled with +inf here; null without occlusion.
template <typename Passes>
int clip_view(srrg2_scene* full, srrg2_scene* clipped, const Xf& L, DevBuf<unsigned>* dmin, size_t bins, srrg2_clip_result* out,
              const Passes& passes) {
  int rc;
  if ((rc = clip_begin(full, clipped))) return rc;
  const int n = full->n;
  // (arrays even for an empty result, as srrg2_scene_set leaves them: srrg2_scene_device_arrays then shows the normals' presence)
  if ((rc = scene_reserve(clipped, 1, 0)) || (rc = clipped->gidx.reserve(1))) return rc;
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status = n == 0 ? SRRG2_CLIPPER_READY : SRRG2_CLIPPER_SUCCESSFUL;
  }
  if (n == 0) return 0;
  hipStream_t st = full->stream;
  if ((rc = full->flags.reserve((size_t) n + 1))) return rc;
  int* const counters = full->dscalars.p;  // (compact_into brings them to the host with the scan's total)
  HIP_TRY(hipMemsetAsync(counters, 0, CLIP_TOTAL * sizeof(int), st));
  if (dmin) {
    if ((rc = dmin->reserve(bins))) return rc;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) dmin->p, 0x7f800000, bins, st));  // +inf
  }
  if ((rc = passes(dim3(blocks_for(n)), counters))) return rc;
  if ((rc = compact_into(full, clipped, L, n))) return rc;
  if (out) {
    out->num_valid   = full->scalars.p[CLIP_VALID];
    out->num_in_view = full->scalars.p[CLIP_IN_VIEW];
    out->num_kept    = full->scalars.p[CLIP_TOTAL];
  }
  return 0;
}

// the projecting flag pass of a view: behind a minimum pass that filled `dmin`, or -- null -- on its own
template <typename V>
void launch_view_flag(const V& view, srrg2_scene* full, dim3 grid, const unsigned* dmin, int* counters) {
  if (dmin)
    hipLaunchKernelGGL((k_view_flag<V, true>), grid, dim3(256), 0, full->stream, view, full->pts.p, full->n, dmin, full->flags.p, counters);
  else
    hipLaunchKernelGGL((k_view_flag<V, false>), grid, dim3(256), 0, full->stream, view, full->pts.p, full->n, dmin, full->flags.p, counters);
}

int check_params(const srrg2_merger_params* p) {
  if (!p) return fail(SRRG2_E_INVALID, "scene_merge: null params");
  if (p->target_number_of_merges < 0) return fail(SRRG2_E_INVALID, "scene_merge: target_number_of_merges < 0");
  return 0;
}

// the tail shared by both merge entry points: count merged points, append if the target was not reached
// (counted: scalars[1] already holds the number of merged measurement points -- k_merge_from_aligner counts them on its way)
// (merged_flags: where the flags of this call lie when not at the head of scene->merged)
int finish_merge(srrg2_scene* scene, srrg2_scene* meas, const Xf& M, bool have_corr, const srrg2_merger_params* p,
                 srrg2_merge_result* out, bool counted = false, const unsigned char* merged_flags = nullptr) {
  int rc;
  const int n_meas = meas->n;
  int num_merged   = 0;
  if (counted) {
    num_merged = scene->scalars.p[1];
  } else if (have_corr && n_meas > 0) {
    hipLaunchKernelGGL(k_count_merged, dim3(std::min(blocks_for(n_meas), 64)), dim3(256), 0, scene->stream, scene->merged.p, n_meas,
                       scene->dscalars.p);
    if ((rc = read_scalars(scene))) return rc;
    num_merged = scene->scalars.p[1];
  }
  out->num_merged = num_merged;
  if (!have_corr || (unsigned) num_merged < (unsigned) p->target_number_of_merges) {  // :92
    if (n_meas > 0) {
      if ((rc = scene->flags.reserve((size_t) n_meas + 1))) return rc;
      const unsigned char* mg = have_corr ? (merged_flags ? merged_flags : scene->merged.p) : nullptr;
      hipLaunchKernelGGL(k_append_flag, dim3(blocks_for(n_meas)), dim3(256), 0, scene->stream, scene->dim, meas->pts.p, mg,
                         n_meas, scene->flags.p);
      int total = 0;
      if ((rc = scan_flags(scene, n_meas, &total))) return rc;
      if (total > 0) {
        if ((rc = scene_reserve(scene, scene->n + total, scene->n))) return rc;
        const Feat f = feat_of(meas, scene);
        LAUNCH_FEAT(k_append_scatter, moves_features(f), dim3(blocks_for(n_meas)), scene->stream, scene->dim, M, meas->pts.p,
                    meas->has_normals ? meas->nrm.p : nullptr, mg, n_meas, scene->flags.p, scene->n, scene->pts.p,
                    scene->nrm.p, f);
        scene->n += total;
      }
      out->num_added = total;
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(scene->stream));
  out->scene_size = scene->n;
  out->status     = SRRG2_MERGER_SUCCESS;  // :122
  return 0;
}

}  // namespace

extern "C" {

int srrg2_merger_default_params(srrg2_merger_params* p) {
  if (!p) return fail(SRRG2_E_INVALID, "merger_default_params: null");
  p->maximum_response                  = 50.f;   // merger_correspondence_homo.h:22-26
  p->maximum_distance_geometry_squared = 0.25f;  // :27-31
  p->target_number_of_merges           = 200;    // merger.h:126-131
  return 0;
}

int srrg2_scene_create(int dim, int device, srrg2_scene_h* out) {
  if ((dim != 2 && dim != 3) || !out) return fail(SRRG2_E_INVALID, "scene_create: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "scene_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "scene_create: bad device index");
  std::unique_ptr<srrg2_scene> s(new srrg2_scene());  // (a failure below deletes it: stream and buffers go with it)
  s->dim    = dim;
  s->device = device;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  int rc;
  if ((rc = s->scalars.reserve(16))) return rc;
  std::memset(s->scalars.p, 0, 16 * sizeof(int));
  if ((rc = s->dscalars.reserve(16))) return rc;
  HIP_TRY(hipMemset(s->dscalars.p, 0, 16 * sizeof(int)));
  *out = s.release();
  return 0;
}

int srrg2_scene_destroy(srrg2_scene_h s) {
  delete s;  // (null: nothing to do)
  return 0;
}

int srrg2_scene_set(srrg2_scene_h s, const float* coords, int cs, const float* normals, int ns, int n, int mem) {
  if (!s || n < 0 || (n > 0 && !coords)) return fail(SRRG2_E_INVALID, "scene_set: bad arguments");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, "scene_set: bad mem");
  if (n > 0 && (cs < s->dim * 4 || cs % 4 || (normals && (ns < s->dim * 4 || ns % 4))))
    return fail(SRRG2_E_INVALID, "scene_set: strides must be multiples of 4 bytes and >= dim floats");
  int rc;
  if ((rc = scene_device(s))) return rc;
  s->has_desc = s->has_inten = false;  // the content is replaced: features of the old points go with them
  if ((rc = scene_reserve(s, n > 0 ? n : 1, 0))) return rc;
  s->n           = n;
  s->ng          = 0;
  s->has_normals = normals != nullptr;
  if (n == 0) return 0;
  const float* dc = coords;
  const float* dn = normals;
  if (mem == SRRG2_MEM_HOST) {
    const size_t bc = (size_t) (n - 1) * cs + (size_t) s->dim * 4, bn = normals ? (size_t) (n - 1) * ns + (size_t) s->dim * 4 : 0;
    const size_t off_n = (bc + 63) / 64 * 64;
    if ((rc = s->staging.reserve(off_n + bn + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->staging.p, coords, bc, hipMemcpyHostToDevice, s->stream));
    dc = (const float*) s->staging.p;
    if (normals) {
      HIP_TRY(hipMemcpyAsync(s->staging.p + off_n, normals, bn, hipMemcpyHostToDevice, s->stream));
      dn = (const float*) (s->staging.p + off_n);
    }
  }
  srrg2amd::launch_ingest(dc, cs / 4, n, s->dim, s->pts.p, nullptr, 0, s->stream);
  if (normals) {
    srrg2amd::launch_ingest(dn, ns / 4, n, s->dim, s->nrm.p, nullptr, 0, s->stream);
  } else {
    HIP_TRY(hipMemsetAsync(s->nrm.p, 0, sizeof(float4) * (size_t) n, s->stream));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

int srrg2_scene_size(srrg2_scene_h s, int* n) {
  if (!s || !n) return fail(SRRG2_E_INVALID, "scene_size: bad arguments");
  *n = s->n;
  return 0;
}

int srrg2_scene_get(srrg2_scene_h s, float* coords_out, float* normals_out, int capacity, int* n) {
  if (!s || !n || capacity < 0) return fail(SRRG2_E_INVALID, "scene_get: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;
  const int m = s->n < capacity ? s->n : capacity;
  if (m > 0 && (coords_out || normals_out)) {
    std::vector<float4> h((size_t) m);
    if (coords_out) {
      HIP_TRY(hipMemcpy(h.data(), s->pts.p, sizeof(float4) * (size_t) m, hipMemcpyDeviceToHost));
      for (int i = 0; i < m; ++i) {
        const float v[3] = {h[(size_t) i].x, h[(size_t) i].y, h[(size_t) i].z};
        for (int d = 0; d < s->dim; ++d) coords_out[(size_t) i * s->dim + d] = v[d];
      }
    }
    if (normals_out) {
      HIP_TRY(hipMemcpy(h.data(), s->nrm.p, sizeof(float4) * (size_t) m, hipMemcpyDeviceToHost));
      for (int i = 0; i < m; ++i) {
        const float v[3] = {h[(size_t) i].x, h[(size_t) i].y, h[(size_t) i].z};
        for (int d = 0; d < s->dim; ++d) normals_out[(size_t) i * s->dim + d] = v[d];
      }
    }
  }
  *n = s->n;
  return 0;
}

int srrg2_scene_device_arrays(srrg2_scene_h s, const float** coords, const float** normals, int* n) {
  if (!s || !coords || !n) return fail(SRRG2_E_INVALID, "scene_device_arrays: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;  // (the arrays go to another stream: an adaptor's queued work has to be done)
  *coords = (const float*) s->pts.p;
  if (normals) *normals = s->has_normals ? (const float*) s->nrm.p : nullptr;
  *n = s->n;
  return 0;
}

int srrg2_scene_set_features(srrg2_scene_h s, const uint8_t* descriptors, int ds, const float* intensity, int is, int n,
                             int mem) {
  if (!s) return fail(SRRG2_E_INVALID, "scene_set_features: null scene");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, "scene_set_features: bad mem");
  if (n != s->n) return fail(SRRG2_E_INVALID, "scene_set_features: n differs from the scene's size");
  if ((descriptors && ds < SRRG2_DESCRIPTOR_BYTES) || (intensity && (is < 4 || is % 4)))
    return fail(SRRG2_E_INVALID, "scene_set_features: descriptor stride >= 32 bytes, intensity stride a multiple of 4 bytes, >= 4");
  int rc;
  if ((rc = scene_device(s))) return rc;
  s->has_desc  = descriptors != nullptr;
  s->has_inten = intensity != nullptr;
  if ((rc = features_reserve(s, 0))) return rc;
  if (n == 0 || (!descriptors && !intensity)) return 0;
  const unsigned char* dd = descriptors;
  const float* di         = intensity;
  if (mem == SRRG2_MEM_HOST) {
    const size_t bd    = descriptors ? (size_t) (n - 1) * ds + SRRG2_DESCRIPTOR_BYTES : 0;
    const size_t bi    = intensity ? (size_t) (n - 1) * is + 4 : 0;
    const size_t off_i = (bd + 63) / 64 * 64;
    if ((rc = s->staging.reserve(off_i + bi + 64))) return rc;
    if (descriptors) {
      HIP_TRY(hipMemcpyAsync(s->staging.p, descriptors, bd, hipMemcpyHostToDevice, s->stream));
      dd = (const unsigned char*) s->staging.p;
    }
    if (intensity) {
      HIP_TRY(hipMemcpyAsync(s->staging.p + off_i, intensity, bi, hipMemcpyHostToDevice, s->stream));
      di = (const float*) (s->staging.p + off_i);
    }
  }
  if (descriptors)
    hipLaunchKernelGGL(k_ingest_descriptors, dim3(blocks_for(n)), dim3(256), 0, s->stream, dd, (size_t) ds, n,
                       reinterpret_cast<unsigned*>(s->desc.p));
  if (intensity)
    hipLaunchKernelGGL(k_ingest_intensity, dim3(blocks_for(n)), dim3(256), 0, s->stream, di, (size_t) (is / 4), n, s->inten.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return 0;
}

int srrg2_scene_has_features(srrg2_scene_h s, int* has_descriptors, int* has_intensity) {
  if (!s) return fail(SRRG2_E_INVALID, "scene_has_features: null scene");
  if (has_descriptors) *has_descriptors = s->has_desc ? 1 : 0;
  if (has_intensity) *has_intensity = s->has_inten ? 1 : 0;
  return 0;
}

int srrg2_scene_get_features(srrg2_scene_h s, uint8_t* descriptors_out, float* intensity_out, int capacity, int* n) {
  if (!s || !n || capacity < 0) return fail(SRRG2_E_INVALID, "scene_get_features: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;
  const int m = s->n < capacity ? s->n : capacity;
  if (m > 0 && descriptors_out && s->has_desc)
    HIP_TRY(hipMemcpy(descriptors_out, s->desc.p, (size_t) m * SRRG2_DESCRIPTOR_BYTES, hipMemcpyDeviceToHost));
  if (m > 0 && intensity_out && s->has_inten)
    HIP_TRY(hipMemcpy(intensity_out, s->inten.p, (size_t) m * sizeof(float), hipMemcpyDeviceToHost));
  *n = s->n;
  return 0;
}

int srrg2_scene_device_features(srrg2_scene_h s, const uint8_t** descriptors, const float** intensity, int* n) {
  if (!s || !n) return fail(SRRG2_E_INVALID, "scene_device_features: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;
  if (descriptors) *descriptors = s->has_desc ? (const uint8_t*) s->desc.p : nullptr;
  if (intensity) *intensity = s->has_inten ? s->inten.p : nullptr;
  *n = s->n;
  return 0;
}

int srrg2_scene_clip_ball(srrg2_scene_h full, const float* robot_in_local_map, float range, srrg2_scene_h clipped,
                          int* status) {
  if (!clip_pair(full, clipped) || !robot_in_local_map) return fail(SRRG2_E_INVALID, "scene_clip_ball: bad arguments");
  int rc;
  if ((rc = clip_begin(full, clipped))) return rc;
  float Linv[12];
  if (full->dim == 3)
    dm::se3_inverse(robot_in_local_map, Linv);  // scene_clipper.h:64-68
  else
    dm::se2_inverse(robot_in_local_map, Linv);
  const Xf L  = load_transform(full->dim, Linv);
  const int n = full->n;
  if (status) *status = n == 0 ? SRRG2_CLIPPER_READY : SRRG2_CLIPPER_SUCCESSFUL;  // :24-28
  if (n == 0) return 0;
  if ((rc = full->flags.reserve((size_t) n + 1))) return rc;
  hipLaunchKernelGGL(k_clip_flag, dim3(blocks_for(n)), dim3(256), 0, full->stream, full->dim, L, range * range, full->pts.p, n,
                     full->flags.p);
  if ((rc = compact_into(full, clipped, L, n))) return rc;
  // (no arrays up front: a fresh handle has them only from here on, after a clip that kept nothing too)
  if ((rc = scene_reserve(clipped, 1, 0)) || (rc = clipped->gidx.reserve(1))) return rc;
  return 0;
}

void srrg2_clip_default_projective_params(srrg2_projective_clip_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->camera_matrix[0] = p->camera_matrix[4] = p->camera_matrix[8] = 1.f;
  p->depth_min = 0.4f;
  p->depth_max = 8.f;
  p->sensor_in_robot[0] = p->sensor_in_robot[5] = p->sensor_in_robot[10] = 1.f;
  p->occlusion_margin = -1.f;
}

int srrg2_scene_clip_projective(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_projective_clip_params* p,
                                srrg2_scene_h clipped, srrg2_clip_result* out) {
  if (!full || !clipped || !robot_in_local_map || !p) return fail(SRRG2_E_INVALID, "scene_clip_projective: null argument");
  if (!clip_pair(full, clipped))
    return fail(SRRG2_E_INVALID, "scene_clip_projective: full and clipped must be two scenes of one dim on one device");
  if (full->dim != 3)
    return fail(SRRG2_E_UNSUPPORTED, "scene_clip_projective: 2-D scenes (a laser scanner's view: srrg2_scene_clip_scan)");
  if (p->image_rows <= 0 || p->image_cols <= 0 || (long long) p->image_rows * (long long) p->image_cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, "scene_clip_projective: image_rows, image_cols > 0 and rows*cols within int32");
  if (!(p->depth_min > 0.f) || !(p->depth_max >= p->depth_min))
    return fail(SRRG2_E_INVALID, "scene_clip_projective: 0 < depth_min <= depth_max");
  const float fx = p->camera_matrix[0], fy = p->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, "scene_clip_projective: fx and fy must be finite and non-zero");
  if (std::isnan(p->occlusion_margin)) return fail(SRRG2_E_INVALID, "scene_clip_projective: occlusion_margin is NaN");
  if (p->camera_matrix[1] != 0.f)
    return fail(SRRG2_E_UNSUPPORTED, "scene_clip_projective: a camera matrix with skew (K[0][1] != 0)");
  float Linv[12], Sinv[12];
  dm::se3_inverse(robot_in_local_map, Linv);
  dm::se3_inverse(p->sensor_in_robot, Sinv);
  const PinholeView view{{load_transform(3, Linv), load_transform(3, Sinv)},
                         {fx, p->camera_matrix[2], fy, p->camera_matrix[5], p->depth_min, p->depth_max, p->occlusion_margin,
                          p->image_rows, p->image_cols}};
  const bool occlusion = p->occlusion_margin >= 0.f;
  return clip_view(full, clipped, view.L, occlusion ? &full->zmin : nullptr, (size_t) p->image_rows * (size_t) p->image_cols, out,
                   [&](dim3 grid, int* counters) {
                     if (occlusion)
                       hipLaunchKernelGGL(k_view_min<PinholeView>, grid, dim3(256), 0, full->stream, view, full->pts.p, full->n,
                                          full->zmin.p);
                     launch_view_flag(view, full, grid, occlusion ? full->zmin.p : nullptr, counters);
                     return 0;
                   });
}

void srrg2_clip_default_scan_params(srrg2_scan_clip_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->range_min = 0.05f;
  p->range_max = 30.f;
  p->sensor_in_robot[0] = p->sensor_in_robot[4] = p->sensor_in_robot[8] = 1.f;
  p->occlusion_margin = -1.f;
}

int srrg2_scene_clip_scan(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_scan_clip_params* p,
                          srrg2_scene_h clipped, srrg2_clip_result* out) {
  if (!full || !clipped || !robot_in_local_map || !p) return fail(SRRG2_E_INVALID, "scene_clip_scan: null argument");
  if (!clip_pair(full, clipped))
    return fail(SRRG2_E_INVALID, "scene_clip_scan: full and clipped must be two scenes of one dim on one device");
  if (full->dim != 2)
    return fail(SRRG2_E_UNSUPPORTED, "scene_clip_scan: 3-D scenes (lidar rings are not built; a camera: srrg2_scene_clip_projective)");
  const double TWO_PI = 6.283185307179586;
  const double inc    = std::fabs(p->angle_increment);
  if (p->num_beams <= 0) return fail(SRRG2_E_INVALID, "scene_clip_scan: num_beams > 0");
  if (!std::isfinite(p->angle_increment) || p->angle_increment == 0.0)
    return fail(SRRG2_E_INVALID, "scene_clip_scan: angle_increment must be finite and non-zero");
  if (!std::isfinite(p->angle_min) || std::fabs(p->angle_min) > TWO_PI)
    return fail(SRRG2_E_INVALID, "scene_clip_scan: angle_min must be finite and within [-2 pi, 2 pi]");
  // (a sector may close on itself once -- 361 beams over 360 degrees; the slack of 2^-20 admits an increment that went through
  // float32 on its way here)
  if (inc * (double) p->num_beams > (TWO_PI + inc) * (1.0 + 0x1p-20))
    return fail(SRRG2_E_INVALID, "scene_clip_scan: |angle_increment| * num_beams beyond 2 pi plus one increment");
  if (!(p->range_min > 0.f) || !(p->range_max >= p->range_min)) return fail(SRRG2_E_INVALID, "scene_clip_scan: 0 < range_min <= range_max");
  if (std::isnan(p->occlusion_margin)) return fail(SRRG2_E_INVALID, "scene_clip_scan: occlusion_margin is NaN");
  float Linv[9], Sinv[9];
  dm::se2_inverse(robot_in_local_map, Linv);
  dm::se2_inverse(p->sensor_in_robot, Sinv);
  const BeamView view{{load_transform(2, Linv), load_transform(2, Sinv)},
                      {p->angle_min, p->angle_increment, std::copysign(TWO_PI, p->angle_increment), p->range_min, p->range_max,
                       p->occlusion_margin, p->num_beams}};
  const bool occlusion = p->occlusion_margin >= 0.f;
  const int nb         = p->num_beams;
  return clip_view(full, clipped, view.L, occlusion ? &full->rmin : nullptr, (size_t) nb, out, [&](dim3 grid, int* counters) {
    hipStream_t st = full->stream;
    const int n    = full->n;
    // every workgroup initialises and flushes num_beams words: give each at least SRRG2_SCLIP_POINTS_PER_BIN points per bin
    const long long share = (long long) SRRG2_SCLIP_POINTS_PER_BIN * nb;
    if (occlusion && nb <= SRRG2_SCLIP_LDS_BINS && n / share >= SRRG2_SCLIP_LDS_MIN_WORKGROUPS) {
      const int blocks = (int) std::min<long long>(grid.x, n / share);
      hipLaunchKernelGGL(k_view_min_lds<BeamView>, dim3(blocks), dim3(256), (size_t) nb * sizeof(unsigned), st, view, nb, full->pts.p,
                         n, full->rmin.p);
    } else if (occlusion) {
      hipLaunchKernelGGL(k_view_min<BeamView>, grid, dim3(256), 0, st, view, full->pts.p, n, full->rmin.p);
    }
    launch_view_flag(view, full, grid, occlusion ? full->rmin.p : nullptr, counters);
    return 0;
  });
}

}  // extern "C"

// srrg2_scene_clip_spherical (ring_elevations == nullptr) and srrg2_scene_clip_spherical_rings; `who` opens every message
static int clip_spherical(const std::string& who, srrg2_scene_h full, const float* robot_in_local_map,
                          const srrg2_spherical_clip_params* p, const double* ring_elevations, srrg2_scene_h clipped,
                          srrg2_clip_result* out) {
  if (!full || !clipped || !robot_in_local_map || !p) return fail(SRRG2_E_INVALID, who + "null argument");
  if (!clip_pair(full, clipped))
    return fail(SRRG2_E_INVALID, who + "full and clipped must be two scenes of one dim on one device");
  if (full->dim != 3) return fail(SRRG2_E_UNSUPPORTED, who + "2-D scenes (a laser scanner's view: srrg2_scene_clip_scan)");
  if (const char* why = sph::invalid(p->model, ring_elevations != nullptr)) return fail(SRRG2_E_INVALID, who + why);
  if (std::isnan(p->occlusion_margin)) return fail(SRRG2_E_INVALID, who + "occlusion_margin is NaN");
  if (p->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  sph::Rings table;
  table.rows = table.descending = 0;
  if (ring_elevations) {
    bool unsupported;
    if (const char* why = sph::rings_of(p->model, ring_elevations, table, &unsupported))
      return fail(unsupported ? SRRG2_E_UNSUPPORTED : SRRG2_E_INVALID, who + why);
  }
  float Linv[12], Sinv[12];
  dm::se3_inverse(robot_in_local_map, Linv);
  dm::se3_inverse(p->sensor_in_robot, Sinv);
  const float margin = p->occlusion_margin;
  const LidarView view{{load_transform(3, Linv), load_transform(3, Sinv)}, sph::geom_of(p->model), margin};
  const bool occlusion = margin >= 0.f;
  // the lidar's passes over either view: staged minimum -> staged flag, or one projecting flag
  const auto passes = [&](const auto& v, dim3 grid, int* counters) {
    using V        = std::decay_t<decltype(v)>;
    hipStream_t st = full->stream;
    const int n    = full->n;
    if (!occlusion) {
      hipLaunchKernelGGL((k_view_flag<V, false>), grid, dim3(256), 0, st, v, full->pts.p, n, (const unsigned*) nullptr, full->flags.p,
                         counters);
      return 0;
    }
    if (int rc = full->sph_stage.reserve((size_t) n)) return rc;
    hipLaunchKernelGGL(k_view_min_staged<V>, grid, dim3(256), 0, st, v, full->pts.p, n, full->rmin.p, full->sph_stage.p, counters);
    hipLaunchKernelGGL(k_spclip_flag_staged, grid, dim3(256), 0, st, full->sph_stage.p, n, full->rmin.p, margin, full->flags.p);
    return 0;
  };
  return clip_view(full, clipped, view.L, occlusion ? &full->rmin : nullptr, (size_t) p->model.rows * (size_t) p->model.cols, out,
                   [&](dim3 grid, int* counters) {
                     return ring_elevations ? passes(RingLidarView{view, table}, grid, counters) : passes(view, grid, counters);
                   });
}

extern "C" {

void srrg2_clip_default_spherical_params(srrg2_spherical_clip_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->model.range_min = 0.5f;
  p->model.range_max = 120.f;
  p->sensor_in_robot[0] = p->sensor_in_robot[5] = p->sensor_in_robot[10] = 1.f;
  p->occlusion_margin = -1.f;
}

int srrg2_scene_clip_spherical(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_spherical_clip_params* p,
                               srrg2_scene_h clipped, srrg2_clip_result* out) {
  return clip_spherical("scene_clip_spherical: ", full, robot_in_local_map, p, nullptr, clipped, out);
}

int srrg2_scene_clip_spherical_rings(srrg2_scene_h full, const float* robot_in_local_map, const srrg2_spherical_clip_params* p,
                                     const double* ring_elevations, srrg2_scene_h clipped, srrg2_clip_result* out) {
  return clip_spherical("scene_clip_spherical_rings: ", full, robot_in_local_map, p, ring_elevations, clipped, out);
}

int srrg2_scene_global_indices(srrg2_scene_h s, int32_t* buf, int* n_inout) {
  if (!s || !n_inout) return fail(SRRG2_E_INVALID, "scene_global_indices: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;
  const int m = s->ng < *n_inout ? s->ng : *n_inout;
  if (buf && m > 0) HIP_TRY(hipMemcpy(buf, s->gidx.p, sizeof(int) * (size_t) m, hipMemcpyDeviceToHost));
  *n_inout = s->ng;
  return 0;
}

int srrg2_scene_merge(srrg2_scene_h scene, srrg2_scene_h meas, const float* measurement_in_scene,
                      const srrg2_correspondence* correspondences, int ncorr, const srrg2_merger_params* p,
                      srrg2_merge_result* out) {
  if (!scene || !meas || !measurement_in_scene || !out || scene == meas || scene->dim != meas->dim ||
      scene->device != meas->device)
    return fail(SRRG2_E_INVALID, "scene_merge: bad arguments");
  if (ncorr > 0 && !correspondences) return fail(SRRG2_E_INVALID, "scene_merge: null correspondences");
  int rc;
  if ((rc = check_params(p))) return rc;
  if ((rc = scene_device(meas)) || (rc = scene_device(scene))) return rc;
  if ((rc = bind_features(scene, meas, "scene_merge"))) return rc;
  std::memset(out, 0, sizeof(*out));
  out->status  = SRRG2_MERGER_INITIALIZING;  // :15
  const Xf M   = load_transform(scene->dim, measurement_in_scene);
  const int n_scene = scene->n, n_meas = meas->n;
  if (scene->n == 0 && meas->has_normals) scene->has_normals = true;  // a fresh scene takes the measurement's fields
  hipStream_t st = scene->stream;
  if (ncorr >= 0) {
    out->num_correspondences = ncorr;
    if ((rc = scene->merged.reserve((size_t) n_meas + 1))) return rc;
    HIP_TRY(hipMemsetAsync(scene->merged.p, 0, (size_t) n_meas + 1, st));
    HIP_TRY(hipMemsetAsync(scene->dscalars.p, 0, 16 * sizeof(int), st));
    if (ncorr > 0) {
      if ((rc = scene->corr.reserve((size_t) ncorr))) return rc;
      if ((rc = scene->counts.reserve((size_t) n_scene + 1))) return rc;
      HIP_TRY(hipMemcpyAsync(scene->corr.p, correspondences, sizeof(srrg2_correspondence) * (size_t) ncorr,
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemsetAsync(scene->counts.p, 0, sizeof(int) * ((size_t) n_scene + 1), st));
      hipLaunchKernelGGL(k_merge_count, dim3(blocks_for(ncorr)), dim3(256), 0, st, scene->corr.p, ncorr, n_scene, n_meas,
                         scene->counts.p, scene->dscalars.p);
      if ((rc = read_scalars(scene))) return rc;
      if (scene->scalars.p[2]) return fail(SRRG2_E_INVALID, "scene_merge: correspondence index out of range");
      const bool dups = scene->scalars.p[3] != 0;
      if (dups && (rc = scene->flags.reserve((size_t) ncorr + 1))) return rc;
      float4* snrm       = scene->nrm.p;  // (always allocated; written like the oracle's)
      const float4* mnrm = meas->has_normals ? meas->nrm.p : nullptr;
      const Feat f       = feat_of(meas, scene);
      const bool feat    = moves_features(f);
      LAUNCH_FEAT(k_merge_apply, feat, dim3(blocks_for(ncorr)), st, scene->dim, M, p->maximum_response,
                  p->maximum_distance_geometry_squared, scene->corr.p, ncorr, scene->counts.p, scene->pts.p, snrm, meas->pts.p,
                  mnrm, scene->merged.p, dups ? scene->flags.p : nullptr, f);
      if (dups) {
        int ndup = 0;
        if ((rc = scan_flags(scene, ncorr, &ndup))) return rc;
        if ((rc = scene->dup_list.reserve((size_t) ndup + 1))) return rc;
        hipLaunchKernelGGL(k_compact_dups, dim3(blocks_for(ncorr)), dim3(256), 0, st, scene->flags.p, scene->corr.p, ncorr,
                           scene->counts.p, scene->dup_list.p);
        if (ndup > 0) {
          if ((rc = scene->dup_keys.reserve(2 * (size_t) ndup))) return rc;
          unsigned long long* kin  = scene->dup_keys.p;
          unsigned long long* kout = scene->dup_keys.p + ndup;
          hipLaunchKernelGGL(k_dup_keys, dim3(blocks_for(ndup)), dim3(256), 0, st, scene->corr.p, scene->dup_list.p, ndup, kin);
          size_t tmp_bytes = 0;
          HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, kin, kout, ndup, 0, 64, st));
          if ((rc = scene->sort_tmp.reserve(std::max<size_t>(tmp_bytes, 1)))) return rc;
          HIP_TRY(hipcub::DeviceRadixSort::SortKeys(scene->sort_tmp.p, tmp_bytes, kin, kout, ndup, 0, 64, st));
          LAUNCH_FEAT(k_merge_dups, feat, dim3(blocks_for(ndup)), st, scene->dim, M, p->maximum_response,
                      p->maximum_distance_geometry_squared, scene->corr.p, kout, ndup, scene->pts.p, snrm, meas->pts.p, mnrm,
                      scene->merged.p, f);
        }
      }
    }
  }
  return finish_merge(scene, meas, M, ncorr >= 0, p, out);
}

int srrg2_scene_merge_from_aligner(srrg2_scene_h scene, srrg2_scene_h meas, const float* measurement_in_scene,
                                   srrg2_aligner_h aligner, int slice_idx, srrg2_scene_h clipped,
                                   const srrg2_merger_params* p, srrg2_merge_result* out) {
  if (!scene || !meas || !measurement_in_scene || !aligner || !clipped || !out || scene == meas ||
      scene->dim != meas->dim || scene->device != meas->device || clipped->device != scene->device)
    return fail(SRRG2_E_INVALID, "scene_merge_from_aligner: bad arguments");
  int rc;
  if ((rc = check_params(p))) return rc;
  if ((rc = scene_device(meas)) || (rc = scene_device(clipped)) || (rc = scene_device(scene))) return rc;
  srrg2amd::AlignerSliceView v;
  if ((rc = srrg2amd::aligner_slice_view(aligner, slice_idx, &v))) return rc;
  if (v.device != scene->device) return fail(SRRG2_E_INVALID, "scene_merge_from_aligner: aligner lives on another device");
  if (v.nm != clipped->ng || v.nm != clipped->n)
    return fail(SRRG2_E_STATE, "scene_merge_from_aligner: the aligner's moving cloud is not the clipped scene");
  if (v.nf != meas->n) return fail(SRRG2_E_STATE, "scene_merge_from_aligner: the aligner's fixed cloud is not the measurement");
  if ((rc = bind_features(scene, meas, "scene_merge_from_aligner"))) return rc;
  if (v.ready_event) HIP_TRY(hipStreamWaitEvent(scene->stream, (hipEvent_t) v.ready_event, 0));  // (no host wait in between)
  std::memset(out, 0, sizeof(*out));
  out->status = SRRG2_MERGER_INITIALIZING;
  const Xf M  = load_transform(scene->dim, measurement_in_scene);
  const int n_scene = scene->n, n_meas = meas->n;
  hipStream_t st = scene->stream;
  // (the call's sixteen counters in FRONT of the flags, in one allocation: one memset instead of two; whole words: the flags are set
  // through 32-bit atomics)
  if ((rc = scene->merged.reserve((size_t) n_meas + 8 + 64))) return rc;
  HIP_TRY(hipMemsetAsync(scene->merged.p, 0, 64 + ((size_t) n_meas + 4) / 4 * 4, st));
  int* const counters         = reinterpret_cast<int*>(scene->merged.p);
  unsigned char* const flags_ = scene->merged.p + 64;
  if (v.nm > 0) {
    const Feat f = feat_of(meas, scene);
    LAUNCH_FEAT(k_merge_from_aligner, moves_features(f), dim3(std::min(blocks_for(v.nm), 256)), st, scene->dim, M,
                p->maximum_response, p->maximum_distance_geometry_squared, v.moving_sorted, v.corr_fixed, v.corr_resp,
                v.corr_stat, v.prune ? 1 : 0, v.nm, clipped->gidx.p, n_scene, n_meas, scene->pts.p, scene->nrm.p, meas->pts.p,
                meas->has_normals ? meas->nrm.p : nullptr, flags_, counters, f);
    if ((rc = read_scalars(scene, counters))) return rc;
    if (scene->scalars.p[2]) return fail(SRRG2_E_STATE, "scene_merge_from_aligner: index out of range");
  }
  else if ((rc = read_scalars(scene, counters)))
    return rc;
  out->num_correspondences = scene->scalars.p[4];
  return finish_merge(scene, meas, M, true, p, out, /*counted=*/true, flags_);
}

}  // extern "C"

int srrg2amd::scene_make_room(srrg2_scene* s, int n, int keep) { return scene_reserve(s, n, keep); }

int srrg2amd::scene_scan_flags(srrg2_scene* s, int n, int* total) { return scan_flags(s, n, total); }

bool srrg2amd::scene_clip_pair(const srrg2_scene* full, const srrg2_scene* clipped) { return clip_pair(full, clipped); }

int srrg2amd::scene_clip_begin(srrg2_scene* full, srrg2_scene* clipped) { return clip_begin(full, clipped); }

int srrg2amd::scene_compact_into(srrg2_scene* full, srrg2_scene* clipped, int n, const std::function<void(int cap)>& scatter,
                                 const std::function<int()>& before_wait) {
  return compact_scatter(full, clipped, n, scatter, before_wait);
}

// what descriptors.hip sees of a scene (srrg2_descriptor_db_add_scene / _match_scene)
int srrg2amd::scene_feature_view(srrg2_scene* s, srrg2amd::SceneFeatureView* v) {
  if (!s || !v) return fail(SRRG2_E_INVALID, "scene_feature_view: bad arguments");
  int rc;
  if ((rc = scene_device(s))) return rc;
  v->pts    = s->pts.p;
  v->desc   = s->has_desc ? s->desc.p : nullptr;
  v->n      = s->n;
  v->dim    = s->dim;
  v->device = s->device;
  v->stream = s->stream;
  return 0;
}
