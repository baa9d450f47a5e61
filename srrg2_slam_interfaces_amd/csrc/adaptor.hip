// adaptor.hip -- measurement adaptors: raw sensor data -> measurement scene, on the device (srrg2_adapt_*).
// Replaces, behind the C ABI of include/srrg2_slam_amd.h, the adapt step of a tracker's frame:
//   MultiTrackerBase_::compute() -> proc->adapt()     S/trackers/multi_tracker_impl.cpp:57-80
//   TrackerSliceProcessorBase_::adapt()               S/trackers/tracker_slice_processor_base_impl.cpp:32-49
//   RawDataPreprocessor_::compute() (interface)       S/raw_data_preprocessors/raw_data_preprocessor.h:13-88
// The reference ships the interface only; the adaptors here (depth image -> organised PointNormal3f cloud, laser scan ->
// PointNormal2f cloud, lidar sweep -> PointNormal3f cloud through a range image) are defined from first principles: DESIGN.md
// section 4 "Measurement adaptors" and "Lidar sweeps" are the arithmetic contract, tests/adaptor_restatement.py,
// tests/lidar_restatement.py and tests/lidar_motion_restatement.py restate it in numpy and the library must give the same bits.
// Kernels: one thread per pixel / beam, grid-stride.  A thread reads its own raw value and its four (two) neighbours' and
// RECOMPUTES the neighbours' points from them -- the same expression gives the same bits as the neighbour's own thread, so
// there is no second pass and no dependency between threads -- and writes point and normal as 16-byte records, coalesced.
// The two image sources (depth image, lidar range image) take the normal from ONE image_normal over the four neighbours' points.
// Organised output is one kernel; compact output is flag -> exclusive scan -> scatter like the ball clipper, the points
// recomputed in the scatter rather than staged.  The counters of srrg2_adapt_result are summed per workgroup and added with
// ONE 64-bit atomic per workgroup (both counts in one word), and read back only when the caller asks for them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>

#include "det_math.h"
#include "device_util.h"
#include "host_util.h"
#include "kernels.h"
#include "scan_beam.h"
#include "scene_state.h"
#include "spherical.h"

using srrg2amd::fail;

namespace {

enum { PX_IN_RANGE = 1, PX_VALID = 2 };

__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ float sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }

// the normal of the image pixel whose point is q, from its right / left / lower / upper neighbours' points: the cross product of
// the two central differences (neither longer than sqrt(maxd2)), normalised, facing the sensor.  false: the pixel has none
__device__ __forceinline__ bool image_normal(const float3 q, const float3 pr, const float3 pl, const float3 pd, const float3 pu,
                                             float maxd2, float4& n) {
  const float dcx = pr.x - pl.x, dcy = pr.y - pl.y, dcz = pr.z - pl.z;
  const float drx = pd.x - pu.x, dry = pd.y - pu.y, drz = pd.z - pu.z;
  if (sq3(dcx, dcy, dcz) > maxd2 || sq3(drx, dry, drz) > maxd2) return false;
  float nx = dcy * drz - dcz * dry;
  float ny = dcz * drx - dcx * drz;
  float nz = dcx * dry - dcy * drx;
  const float len = sqrtf(sq3(nx, ny, nz));
  if (!(len > 0.f)) return false;
  nx = nx / len;
  ny = ny / len;
  nz = nz / len;
  if ((nx * q.x + ny * q.y) + nz * q.z > 0.f) {  // normals face the sensor
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  n = make_float4(nx, ny, nz, 0.f);
  return true;
}

// ---- depth image -----------------------------------------------------------------------------------------------------
struct DepthArgs {
  const unsigned char* depth;
  const unsigned char* inten;  // null: no intensity
  long long depth_stride, inten_stride;  // bytes per row
  int inten_f32;                         // intensity is F32 (else U8)
  int rows, cols;
  int gc, gr;  // gaps; gc == 0: no normals
  float ifx, ify, cx, cy, scale, zmin, zmax, maxd2;
  int drop;
};

template <typename D>
struct DepthSource {
  DepthArgs a;

  __device__ __forceinline__ bool depth_at(int r, int c, float& z) const {
    const D raw = *reinterpret_cast<const D*>(a.depth + (long long) r * a.depth_stride + (long long) c * (long long) sizeof(D));
    if (sizeof(D) == 2) {
      if (raw == (D) 0) return false;
      z = (float) raw * a.scale;
    } else {
      z = (float) raw;
    }
    return isfinite(z) && a.zmin <= z && z <= a.zmax;
  }
  __device__ __forceinline__ float3 point_at(int r, int c, float z) const {
    return make_float3((((float) c - a.cx) * a.ifx) * z, (((float) r - a.cy) * a.ify) * z, z);
  }
  // point and normal of pixel i as they are stored; returns PX_* bits
  __device__ __forceinline__ int eval(int i, float4& p, float4& n) const {
    const int r = i / a.cols, c = i - r * a.cols;
    const float qn = quiet_nan();
    p = make_float4(qn, qn, qn, 0.f);
    n = a.gc > 0 ? make_float4(qn, qn, qn, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    float z;
    if (!depth_at(r, c, z)) return 0;
    const float3 q = point_at(r, c, z);
    bool has_normal = false;
    if (a.gc > 0 && c >= a.gc && c < a.cols - a.gc && r >= a.gr && r < a.rows - a.gr) {
      float zl, zr, zu, zd;
      const bool okl = depth_at(r, c - a.gc, zl), okr = depth_at(r, c + a.gc, zr);
      const bool oku = depth_at(r - a.gr, c, zu), okd = depth_at(r + a.gr, c, zd);
      if (okl && okr && oku && okd)
        has_normal = image_normal(q, point_at(r, c + a.gc, zr), point_at(r, c - a.gc, zl), point_at(r + a.gr, c, zd),
                                  point_at(r - a.gr, c, zu), a.maxd2, n);
    }
    const bool valid = a.gc == 0 || has_normal || !a.drop;
    if (valid) p = make_float4(q.x, q.y, q.z, 0.f);
    return PX_IN_RANGE | (valid ? PX_VALID : 0);
  }
  __device__ __forceinline__ float intensity(int i) const {
    const int r = i / a.cols, c = i - r * a.cols;
    const unsigned char* row = a.inten + (long long) r * a.inten_stride;
    return a.inten_f32 ? reinterpret_cast<const float*>(row)[c] : (float) row[c];
  }
};

// ---- laser scan ------------------------------------------------------------------------------------------------------
struct ScanSource {
  const float* ranges;
  int n, w;  // w == 0: no normals
  double amin, ainc;
  float rmin, rmax, maxd2;
  int drop;

  __device__ __forceinline__ bool range_at(int k, float& r) const {
    r = ranges[k];
    return isfinite(r) && rmin <= r && r <= rmax;
  }
  __device__ __forceinline__ float2 point_at(int k, float r) const { return scan_beam_point(amin, ainc, k, r); }
  __device__ __forceinline__ int eval(int k, float4& p, float4& nrm) const {
    const float qn = quiet_nan();
    p   = make_float4(qn, qn, 0.f, 0.f);
    nrm = w > 0 ? make_float4(qn, qn, 0.f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    float r;
    if (!range_at(k, r)) return 0;
    const float2 q  = point_at(k, r);
    bool has_normal = false;
    if (w > 0 && k >= w && k < n - w) {
      float ra, rb;
      const bool oka = range_at(k - w, ra), okb = range_at(k + w, rb);
      if (oka && okb) {
        const float2 pa = point_at(k - w, ra), pb = point_at(k + w, rb);
        const float tx = pb.x - pa.x, ty = pb.y - pa.y;
        const float t2 = tx * tx + ty * ty;
        if (t2 <= maxd2) {
          const float len = sqrtf(t2);
          if (len > 0.f) {
            float nx = ty / len, ny = -tx / len;
            if (nx * q.x + ny * q.y > 0.f) {
              nx = -nx;
              ny = -ny;
            }
            nrm        = make_float4(nx, ny, 0.f, 0.f);
            has_normal = true;
          }
        }
      }
    }
    const bool valid = w == 0 || has_normal || !drop;
    if (valid) p = make_float4(q.x, q.y, 0.f, 0.f);
    return PX_IN_RANGE | (valid ? PX_VALID : 0);
  }
  __device__ __forceinline__ float intensity(int) const { return 0.f; }
};

// ---- lidar sweep (DESIGN.md section 4 "Lidar sweeps") ------------------------------------------------------------------
// A sweep arrives as a list of points; the range image that organises it is built first: k_lidar_bin projects every point
// (spherical.h) and takes, per pixel, the minimum of (range bits << 32 | input index) -- positive floats order like their bit
// patterns, so the nearest point wins and, of equal ranges, the lowest index, whoever comes first.  ONE 64-bit atomicMin without
// return value per in-view point, straight into global memory: the table of a 64 x 2048 sensor is 1 MB, far beyond a
// workgroup's LDS, and a sweep puts about one point on each word, so there is nothing for a private table to combine.
// (It is k_lidar_bin_ex<false, false> written out: launched through that template, with the 2.3 KB of table and de-skew block
// it never reads in its kernel arguments, the plain adapt measured 1-2 us slower -- profiles/view_clip_refactor_ab.txt.)
__global__ __launch_bounds__(256) void k_lidar_bin(const unsigned char* __restrict__ pts, long long stride, int n, sph::Geom G,
                                                   unsigned long long* __restrict__ winner) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* q = reinterpret_cast<const float*>(pts + (long long) i * stride);
    const float x = q[0], y = q[1], z = q[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    float rho;
    const int pix = sph::project(G, x, y, z, rho);  // (pix < rows * cols: project's bounds)
    if (pix >= 0) atomicMin(&winner[pix], ((unsigned long long) __float_as_uint(rho) << 32) | (unsigned long long) (unsigned) i);
  }
}

// ---- ring tables and motion de-skew (srrg2_adapt_lidar_sweep_ex; DESIGN.md section 4 "Lidar sweeps", contracts 1 and 2) ----
// what the de-skew of one point needs, prepared on the host in float64 (deskew_of): the sweep's motion as an angle about a
// fixed axis plus a translation linear in s, the rotation at s = reference (Rref, row-major) and reference * t
struct Deskew {
  const unsigned char* times;  // null: s from the raw azimuth (tf / cols)
  long long time_stride;
  double t0, dt;  // time_begin, time_end - time_begin
  double theta, a[3], t[3], rt[3], Rref[9];
};

// p (raw, sensor frame at its firing time s) -> the sensor frame at s = reference; each component rounded to float32 once
__device__ __forceinline__ float4 deskew_point(const Deskew& K, double s, float x, float y, float z) {
  const double px = (double) x, py = (double) y, pz = (double) z;
  double sn, cs;
  dm::sincos(s * K.theta, sn, cs);
  const double omc = 1.0 - cs;
  const double cx = K.a[1] * pz - K.a[2] * py, cy = K.a[2] * px - K.a[0] * pz, cz = K.a[0] * py - K.a[1] * px;
  const double k  = ((K.a[0] * px + K.a[1] * py) + K.a[2] * pz) * omc;
  const double qx = ((px * cs + cx * sn) + K.a[0] * k) + s * K.t[0];
  const double qy = ((py * cs + cy * sn) + K.a[1] * k) + s * K.t[1];
  const double qz = ((pz * cs + cz * sn) + K.a[2] * k) + s * K.t[2];
  const double vx = qx - K.rt[0], vy = qy - K.rt[1], vz = qz - K.rt[2];
  return make_float4((float) ((K.Rref[0] * vx + K.Rref[3] * vy) + K.Rref[6] * vz),
                     (float) ((K.Rref[1] * vx + K.Rref[4] * vy) + K.Rref[7] * vz),
                     (float) ((K.Rref[2] * vx + K.Rref[5] * vy) + K.Rref[8] * vz), 0.f);
}

// k_lidar_bin with a ring table (RINGS: staged into LDS once per workgroup) and / or the de-skew fused in (DESKEW): the point
// is binned from its RAW coordinates -- the image stays the sensor's firing grid -- and what the image will read as its
// coordinates, the de-skewed point, is written to dsk[i], 16 bytes per in-view point (only winners are ever read, and only
// in-view points can win).  A point whose time is not finite is a point with a non-finite coordinate.
template <bool RINGS, bool DESKEW>
__global__ __launch_bounds__(256) void k_lidar_bin_ex(const unsigned char* __restrict__ pts, long long stride, int n, sph::Geom G,
                                                      sph::Rings T, Deskew K, unsigned long long* __restrict__ winner,
                                                      float4* __restrict__ dsk) {
  __shared__ double sB[RINGS ? sph::MAX_RING_ROWS + 1 : 1];
  if (RINGS) sph::stage_rings(T, sB);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* q = reinterpret_cast<const float*>(pts + (long long) i * stride);
    const float x = q[0], y = q[1], z = q[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    double s = 0.0;
    if (DESKEW && K.times) {
      const float tm = *reinterpret_cast<const float*>(K.times + (long long) i * K.time_stride);
      if (!isfinite(tm)) continue;
      s = ((double) tm - K.t0) / K.dt;
    }
    float rho;
    double tf;
    const int pix = sph::project_t<RINGS>(G, sB, T.descending, x, y, z, rho, tf);  // (pix < rows * cols: project's bounds)
    if (pix < 0) continue;
    atomicMin(&winner[pix], ((unsigned long long) __float_as_uint(rho) << 32) | (unsigned long long) (unsigned) i);
    if (DESKEW) {
      if (!K.times) s = tf / (double) G.cols;
      dsk[i] = deskew_point(K, s, x, y, z);
    }
  }
}

// the range image as a source of run_adapt: pixel -> its winner's input point, normals from the four neighbouring winners
struct LidarSource {
  const unsigned char* pts;
  const unsigned char* inten;  // null: no intensity
  long long pts_stride, inten_stride;
  const unsigned long long* winner;
  int rows, cols;
  int gc, gr;  // gaps; gc == 0: no normals
  int wrap;    // the columns close the circle
  float maxd2;
  int drop;

  // the input index of the pixel's winner (< n by construction); false: the pixel is empty
  __device__ __forceinline__ bool winner_at(int r, int c, unsigned& idx) const {
    const unsigned long long w = winner[(long long) r * cols + c];
    idx                        = (unsigned) w;
    return w != ~0ull;
  }
  __device__ __forceinline__ float3 point_of(unsigned idx) const {
    const float* q = reinterpret_cast<const float*>(pts + (long long) idx * pts_stride);
    return make_float3(q[0], q[1], q[2]);
  }
  __device__ __forceinline__ int eval(int i, float4& p, float4& n) const {
    const int r = i / cols, c = i - r * cols;
    const float qn = quiet_nan();
    p = make_float4(qn, qn, qn, 0.f);
    n = gc > 0 ? make_float4(qn, qn, qn, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned iq;
    if (!winner_at(r, c, iq)) return 0;
    const float3 q  = point_of(iq);
    bool has_normal = false;
    if (gc > 0 && r >= gr && r < rows - gr && (wrap || (c >= gc && c < cols - gc))) {
      int cl = c - gc, cr = c + gc;
      if (wrap) {  // (gaps beyond one turn: modulo cols, like any other)
        const int g = gc % cols;
        cl          = c - g < 0 ? c - g + cols : c - g;
        cr          = c + g >= cols ? c + g - cols : c + g;
      }
      unsigned il, ir, iu, id;
      const bool okl = winner_at(r, cl, il), okr = winner_at(r, cr, ir);
      const bool oku = winner_at(r - gr, c, iu), okd = winner_at(r + gr, c, id);
      if (okl && okr && oku && okd) has_normal = image_normal(q, point_of(ir), point_of(il), point_of(id), point_of(iu), maxd2, n);
    }
    const bool valid = gc == 0 || has_normal || !drop;
    if (valid) p = make_float4(q.x, q.y, q.z, 0.f);
    return PX_IN_RANGE | (valid ? PX_VALID : 0);
  }
  __device__ __forceinline__ float intensity(int i) const {
    const unsigned long long w = winner[i];
    if (w == ~0ull) return 0.f;
    return *reinterpret_cast<const float*>(inten + (long long) (unsigned) w * inten_stride);
  }
};

// ---- kernels ---------------------------------------------------------------------------------------------------------
// both counts of a workgroup in one word (low: in range, high: Valid): ONE block_add, so one atomic per workgroup
__device__ __forceinline__ unsigned long long pack_counts(int in_range, int valid) {
  return (unsigned long long) (unsigned) in_range | ((unsigned long long) (unsigned) valid << 32);
}

template <typename S>
__global__ __launch_bounds__(256) void k_adapt_organised(S src, int n, float4* __restrict__ pts, float4* __restrict__ nrm,
                                                         float* __restrict__ inten, unsigned long long* __restrict__ counters) {
  int in_range = 0, valid = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float4 p, q;
    const int f = src.eval(i, p, q);
    pts[i] = p;
    nrm[i] = q;
    if (inten) inten[i] = src.intensity(i);
    in_range += f & 1;
    valid += f >> 1;
  }
  block_add(pack_counts(in_range, valid), counters);
}

template <typename S>
__global__ __launch_bounds__(256) void k_adapt_flag(S src, int n, int* __restrict__ flags, unsigned long long* __restrict__ counters) {
  int in_range = 0, valid = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float4 p, q;
    const int f = src.eval(i, p, q);
    flags[i]    = f >> 1;
    in_range += f & 1;
    valid += f >> 1;
  }
  block_add(pack_counts(in_range, valid), counters);
}

template <typename S>
__global__ __launch_bounds__(256) void k_adapt_scatter(S src, int n, const int* __restrict__ offset, int total,
                                                       float4* __restrict__ pts, float4* __restrict__ nrm,
                                                       float* __restrict__ inten, int* __restrict__ gidx) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float4 p, q;
    if (!(src.eval(i, p, q) & PX_VALID)) continue;
    const int k = offset[i];
    if (k < 0 || k >= total) continue;  // (cannot happen: flags and scatter evaluate the same expression)
    pts[k]  = p;
    nrm[k]  = q;
    gidx[k] = i;
    if (inten) inten[k] = src.intensity(i);
  }
}

// few, fat workgroups: the work per pixel is a handful of flops and the counters cost one atomic per workgroup
int adapt_blocks(int n) {
  int b = (n + 255) / 256;
  return b < 1 ? 1 : (b > 512 ? 512 : b);
}

// raw data in pageable or pinned host memory -> the scene's staging buffer at `offset`, on the scene's stream
int stage(srrg2_scene* s, const void* host, size_t bytes, size_t offset, const unsigned char** dev) {
  HIP_TRY(hipMemcpyAsync(s->staging.p + offset, host, bytes, hipMemcpyHostToDevice, s->stream));
  *dev = reinterpret_cast<const unsigned char*>(s->staging.p + offset);
  return 0;
}

// the part the adaptors share.  The source's device pointers are valid on the scene's stream; nothing of `s` has changed yet.
template <typename S>
int run_adapt(srrg2_scene* s, const S& src, int n, bool normals, bool intensity, bool compact, srrg2_adapt_result* out) {
  int rc;
  s->has_desc  = false;  // the content is replaced: features of the old points go with them
  s->has_inten = intensity;
  if (out) {
    std::memset(out, 0, sizeof(*out));
    out->status  = n == 0 ? SRRG2_ADAPTOR_INITIALIZING : SRRG2_ADAPTOR_READY;
    out->num_raw = n;
  }
  if (n == 0) {
    if ((rc = srrg2amd::scene_make_room(s, 1, 0))) return rc;
    s->n = s->ng = 0;
    s->has_normals = normals;
    return 0;
  }
  hipStream_t st = s->stream;
  unsigned long long* counters = reinterpret_cast<unsigned long long*>(s->dscalars.p + 8);
  HIP_TRY(hipMemsetAsync(counters, 0, sizeof(unsigned long long), st));
  const dim3 grid(adapt_blocks(n)), block(256);
  if (!compact) {
    if ((rc = srrg2amd::scene_make_room(s, n, 0))) return rc;
    s->n           = n;
    s->ng          = 0;
    s->has_normals = normals;
    hipLaunchKernelGGL(k_adapt_organised<S>, grid, block, 0, st, src, n, s->pts.p, s->nrm.p, intensity ? s->inten.p : nullptr,
                       counters);
    HIP_TRY(hipGetLastError());
    s->pending = true;
    if (!out) return 0;  // (queued: whoever reads the scene next from another stream or from the host settles it)
  } else {
    if ((rc = s->flags.reserve((size_t) n + 1))) return rc;
    hipLaunchKernelGGL(k_adapt_flag<S>, grid, block, 0, st, src, n, s->flags.p, counters);
    int total = 0;
    if ((rc = srrg2amd::scene_scan_flags(s, n, &total))) return rc;
    if (total < 0 || total > n) return fail(SRRG2_E_HIP, "adapt: the compaction scan returned a total out of range");
    if ((rc = srrg2amd::scene_make_room(s, total > 0 ? total : 1, 0))) return rc;
    if ((rc = s->gidx.reserve((size_t) (total > 0 ? total : 1)))) return rc;
    s->n = s->ng = total;
    s->has_normals = normals;
    if (total > 0)
      hipLaunchKernelGGL(k_adapt_scatter<S>, grid, block, 0, st, src, n, s->flags.p, total, s->pts.p, s->nrm.p,
                         intensity ? s->inten.p : nullptr, s->gidx.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(&s->scalars.p[8], counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  s->pending = false;
  if (out) {
    out->num_in_range = s->scalars.p[8];
    out->num_valid    = s->scalars.p[9];
    out->scene_size   = s->n;
  }
  return 0;
}

bool aligned_to(const void* p, long long stride, int elem) {
  return reinterpret_cast<uintptr_t>(p) % (uintptr_t) elem == 0 && stride % elem == 0;
}

// the host side of the de-skew, float64 with det_math.h only: motion = [R|t] -> angle about a fixed axis (through the unit
// quaternion, w >= 0), the rotation at s = reference by the per-point formula applied to the three unit vectors, reference * t
void deskew_of(const srrg2_lidar_sweep_extras& x, Deskew& K) {
  double R[9], q[4];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (double) x.motion[i * 4 + j];
    K.t[i] = (double) x.motion[i * 4 + 3];
  }
  dm::R_to_quat(R, q);
  const double vn = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
  if (vn == 0.0) {
    K.theta = 0.0;
    K.a[0] = 0.0, K.a[1] = 0.0, K.a[2] = 1.0;
  } else {
    K.theta = 2.0 * dm::atan2(vn, q[0]);
    K.a[0] = q[1] / vn, K.a[1] = q[2] / vn, K.a[2] = q[3] / vn;
  }
  double sn, cs;
  dm::sincos(x.reference * K.theta, sn, cs);
  const double omc = 1.0 - cs;
  for (int j = 0; j < 3; ++j) {  // column j = the rotation of e_j
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    const double c[3] = {K.a[1] * e[2] - K.a[2] * e[1], K.a[2] * e[0] - K.a[0] * e[2], K.a[0] * e[1] - K.a[1] * e[0]};
    const double k    = ((K.a[0] * e[0] + K.a[1] * e[1]) + K.a[2] * e[2]) * omc;
    for (int i = 0; i < 3; ++i) K.Rref[i * 3 + j] = (e[i] * cs + c[i] * sn) + K.a[i] * k;
  }
  for (int i = 0; i < 3; ++i) K.rt[i] = x.reference * K.t[i];
}

// up to three strided host arrays -> the scene's staging buffer; arrays whose byte ranges touch or overlap (interleaved XYZI /
// XYZIT records) travel together, once.  b[k] .. e[k] in, the device address of b[k] out (a null b[k] is skipped).
int stage_ranges(srrg2_scene* s, int count, const unsigned char** b, const unsigned char* const* e) {
  int order[3], m = 0;
  for (int k = 0; k < count; ++k)
    if (b[k]) order[m++] = k;
  for (int i = 1; i < m; ++i)
    for (int j = i; j > 0 && b[order[j]] < b[order[j - 1]]; --j) std::swap(order[j], order[j - 1]);
  const unsigned char *lo[3], *hi[3];
  int span_of[3], spans = 0;
  for (int i = 0; i < m; ++i) {
    const int k = order[i];
    if (spans > 0 && b[k] <= hi[spans - 1]) {
      if (e[k] > hi[spans - 1]) hi[spans - 1] = e[k];
    } else {
      lo[spans] = b[k], hi[spans] = e[k];
      ++spans;
    }
    span_of[k] = spans - 1;
  }
  size_t off[3], total = 0;
  for (int j = 0; j < spans; ++j) {
    off[j] = total;
    total  = (total + (size_t) (hi[j] - lo[j]) + 63) / 64 * 64;
  }
  int rc;
  if ((rc = s->staging.reserve(total + 64))) return rc;
  const unsigned char* d[3];
  for (int j = 0; j < spans; ++j)
    if ((rc = stage(s, lo[j], (size_t) (hi[j] - lo[j]), off[j], &d[j]))) return rc;
  for (int i = 0; i < m; ++i) {
    const int k = order[i];
    b[k]        = d[span_of[k]] + (b[k] - lo[span_of[k]]);
  }
  return 0;
}

// srrg2_adapt_lidar_sweep (x == nullptr) and srrg2_adapt_lidar_sweep_ex; `who` opens every message
int adapt_lidar_sweep(const std::string& who, srrg2_scene_h dst, const float* points, int point_stride, const float* intensity,
                      int intensity_stride, int n, int mem, const srrg2_lidar_adaptor_params* p, const srrg2_lidar_sweep_extras* x,
                      srrg2_adapt_result* out) {
  if (!dst || !p) return fail(SRRG2_E_INVALID, who + "null scene or params");
  if (dst->dim != 3) return fail(SRRG2_E_INVALID, who + "the scene must have dim 3");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (n < 0) return fail(SRRG2_E_INVALID, who + "n >= 0");
  if (p->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  if (p->normal_col_gap < 0 || p->normal_row_gap < 0 || (p->normal_col_gap == 0) != (p->normal_row_gap == 0))
    return fail(SRRG2_E_INVALID, who + "normal gaps >= 0, and both or neither 0");
  const bool rings  = x && x->ring_elevations;
  const bool deskew = x && x->deskew != 0;
  const bool timed  = deskew && x->times != nullptr;
  if (const char* why = sph::invalid(p->model, rings)) return fail(SRRG2_E_INVALID, who + why);
  sph::Rings table;
  Deskew K;
  std::memset(&K, 0, sizeof(K));
  table.rows = table.descending = 0;
  if (x) {
    if (x->reserved[0] != 0 || x->reserved[1] != 0) return fail(SRRG2_E_INVALID, who + "extras: reserved must be 0");
    if (rings) {
      bool unsupported;
      if (const char* why = sph::rings_of(p->model, x->ring_elevations, table, &unsupported))
        return fail(unsupported ? SRRG2_E_UNSUPPORTED : SRRG2_E_INVALID, who + why);
    }
    if (deskew) {
      bool finite = std::isfinite(x->reference);
      for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(x->motion[i]);
      if (!finite) return fail(SRRG2_E_INVALID, who + "extras: motion and reference must be finite");
      if (timed) {
        if (!std::isfinite(x->time_begin) || !std::isfinite(x->time_end) || x->time_begin == x->time_end)
          return fail(SRRG2_E_INVALID, who + "extras: time_begin and time_end must be finite and differ");
        if (x->time_stride_bytes < 4 || !aligned_to(x->times, x->time_stride_bytes, 4))
          return fail(SRRG2_E_INVALID, who + "extras: time stride >= 4 and a multiple of 4, times 4-byte aligned");
      }
    }
  }
  if (n > 0) {
    if (!points) return fail(SRRG2_E_INVALID, who + "null points");
    if (point_stride < 12 || !aligned_to(points, point_stride, 4))
      return fail(SRRG2_E_INVALID, who + "point stride >= 12 and a multiple of 4, points 4-byte aligned");
    if (intensity && (intensity_stride < 4 || !aligned_to(intensity, intensity_stride, 4)))
      return fail(SRRG2_E_INVALID, who + "intensity stride >= 4 and a multiple of 4, intensity 4-byte aligned");
  }
  int rc;
  HIP_TRY(hipSetDevice(dst->device));
  const bool with_inten = intensity != nullptr;
  LidarSource src;
  std::memset(&src, 0, sizeof(src));
  src.rows = p->model.rows, src.cols = p->model.cols;
  src.gc = p->normal_col_gap, src.gr = p->normal_row_gap;
  src.wrap  = sph::columns_wrap(p->model);
  src.maxd2 = p->normal_max_distance_squared;
  src.drop  = p->drop_points_without_normal != 0;
  const bool normals = src.gc > 0;
  if (n == 0) return run_adapt(dst, src, 0, normals, with_inten, p->compact != 0, out);  // an empty scene, INITIALIZING
  src.pts        = reinterpret_cast<const unsigned char*>(points);
  src.inten      = reinterpret_cast<const unsigned char*>(intensity);
  src.pts_stride = point_stride, src.inten_stride = intensity_stride;
  if (timed) {
    K.times       = reinterpret_cast<const unsigned char*>(x->times);
    K.time_stride = x->time_stride_bytes;
    K.t0          = x->time_begin;
    K.dt          = x->time_end - x->time_begin;
  }
  hipStream_t st = dst->stream;
  if (mem == SRRG2_MEM_HOST) {  // the records as they lie; interleaved intensities and times travel with their points, once
    const unsigned char* b[3] = {src.pts, src.inten, K.times};
    const unsigned char* e[3] = {b[0] + (size_t) (n - 1) * (size_t) point_stride + 12,
                                 with_inten ? b[1] + (size_t) (n - 1) * (size_t) intensity_stride + 4 : nullptr,
                                 timed ? b[2] + (size_t) (n - 1) * (size_t) K.time_stride + 4 : nullptr};
    if ((rc = stage_ranges(dst, 3, b, e))) return rc;
    src.pts = b[0], src.inten = b[1], K.times = b[2];
    HIP_TRY(hipStreamSynchronize(st));  // the caller's cloud is consumed (pinned memory too) before anything is queued
  }
  const size_t npix = (size_t) src.rows * (size_t) src.cols;
  if ((rc = dst->winner.reserve(npix))) return rc;
  if (deskew && (rc = dst->deskewed.reserve((size_t) n))) return rc;
  HIP_TRY(hipMemsetAsync(dst->winner.p, 0xff, npix * sizeof(unsigned long long), st));
  const dim3 grid(adapt_blocks(n)), block(256);
  const sph::Geom geom = sph::geom_of(p->model);
  if (!rings && !deskew) {
    hipLaunchKernelGGL(k_lidar_bin, grid, block, 0, st, src.pts, src.pts_stride, n, geom, dst->winner.p);
  } else {
    if (deskew) deskew_of(*x, K);
    float4* const dsk = deskew ? dst->deskewed.p : nullptr;
    const auto bin    = rings ? (deskew ? k_lidar_bin_ex<true, true> : k_lidar_bin_ex<true, false>) : k_lidar_bin_ex<false, true>;
    hipLaunchKernelGGL(bin, grid, block, 0, st, src.pts, src.pts_stride, n, geom, table, K, dst->winner.p, dsk);
    if (deskew) {  // the image reads the de-skewed points from here on
      src.pts        = reinterpret_cast<const unsigned char*>(dsk);
      src.pts_stride = 16;
    }
  }
  HIP_TRY(hipGetLastError());
  src.winner = dst->winner.p;
  if ((rc = run_adapt(dst, src, (int) npix, normals, with_inten, p->compact != 0, out))) return rc;
  if (out) out->num_raw = n;  // (run_adapt counted the pixels it walked)
  return 0;
}

}  // namespace

extern "C" {

void srrg2_adapt_default_depth_params(srrg2_depth_adaptor_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->camera_matrix[0] = p->camera_matrix[4] = p->camera_matrix[8] = 1.f;
  p->depth_scale                 = 0.001f;
  p->depth_min                   = 0.4f;
  p->depth_max                   = 8.f;
  p->normal_col_gap              = 1;
  p->normal_row_gap              = 1;
  p->normal_max_distance_squared = 0.0625f;
  p->drop_points_without_normal  = 1;
  p->compact                     = 0;
}

void srrg2_adapt_default_scan_params(srrg2_scan_adaptor_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->range_min                   = 0.05f;
  p->range_max                   = 30.f;
  p->normal_half_window          = 1;
  p->normal_max_distance_squared = 0.01f;
  p->drop_points_without_normal  = 1;
  p->compact                     = 0;
}

int srrg2_adapt_depth_image(srrg2_scene_h dst, const void* depth, int depth_type, int depth_stride, const void* intensity,
                            int intensity_type, int intensity_stride, int mem, const srrg2_depth_adaptor_params* p,
                            srrg2_adapt_result* out) {
  if (!dst || !p) return fail(SRRG2_E_INVALID, "adapt_depth_image: null scene or params");
  if (dst->dim != 3) return fail(SRRG2_E_INVALID, "adapt_depth_image: the scene must have dim 3");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, "adapt_depth_image: bad mem");
  if (depth_type != SRRG2_IMAGE_U16 && depth_type != SRRG2_IMAGE_F32)
    return fail(SRRG2_E_INVALID, "adapt_depth_image: depth_type must be SRRG2_IMAGE_U16 or SRRG2_IMAGE_F32");
  if (intensity_type != SRRG2_IMAGE_NONE && intensity_type != SRRG2_IMAGE_U8 && intensity_type != SRRG2_IMAGE_F32)
    return fail(SRRG2_E_INVALID, "adapt_depth_image: intensity_type must be NONE, U8 or F32");
  if (p->rows < 0 || p->cols < 0 || (long long) p->rows * (long long) p->cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, "adapt_depth_image: rows, cols >= 0 and rows*cols within int32");
  if (p->normal_col_gap < 0 || p->normal_row_gap < 0 || (p->normal_col_gap == 0) != (p->normal_row_gap == 0))
    return fail(SRRG2_E_INVALID, "adapt_depth_image: normal gaps >= 0, and both or neither 0");
  const float fx = p->camera_matrix[0], fy = p->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, "adapt_depth_image: fx and fy must be finite and non-zero");
  if (p->camera_matrix[1] != 0.f) return fail(SRRG2_E_UNSUPPORTED, "adapt_depth_image: a camera matrix with skew (K[0][1] != 0)");
  const int n  = p->rows * p->cols;
  const int de = depth_type == SRRG2_IMAGE_U16 ? 2 : 4, ie = intensity_type == SRRG2_IMAGE_F32 ? 4 : 1;
  const bool with_inten = intensity_type != SRRG2_IMAGE_NONE;
  if (n > 0) {
    if (!depth || (with_inten && !intensity)) return fail(SRRG2_E_INVALID, "adapt_depth_image: null image");
    if ((long long) depth_stride < (long long) p->cols * de || !aligned_to(depth, depth_stride, de))
      return fail(SRRG2_E_INVALID, "adapt_depth_image: depth row stride smaller than a row, or image not aligned to its element");
    if (with_inten && ((long long) intensity_stride < (long long) p->cols * ie || !aligned_to(intensity, intensity_stride, ie)))
      return fail(SRRG2_E_INVALID, "adapt_depth_image: intensity row stride smaller than a row, or image not aligned to its element");
  }
  int rc;
  HIP_TRY(hipSetDevice(dst->device));
  DepthArgs a;
  std::memset(&a, 0, sizeof(a));
  a.depth        = static_cast<const unsigned char*>(depth);
  a.inten        = with_inten ? static_cast<const unsigned char*>(intensity) : nullptr;
  a.depth_stride = depth_stride;
  a.inten_stride = intensity_stride;
  a.inten_f32    = intensity_type == SRRG2_IMAGE_F32;
  a.rows = p->rows, a.cols = p->cols;
  a.gc = p->normal_col_gap, a.gr = p->normal_row_gap;
  a.ifx = 1.0f / fx, a.ify = 1.0f / fy;
  a.cx = p->camera_matrix[2], a.cy = p->camera_matrix[5];
  a.scale = p->depth_scale, a.zmin = p->depth_min, a.zmax = p->depth_max;
  a.maxd2 = p->normal_max_distance_squared;
  a.drop  = p->drop_points_without_normal != 0;
  if (n > 0 && mem == SRRG2_MEM_HOST) {  // rows up to the last pixel of the last row, as they lie
    const size_t bd    = (size_t) (p->rows - 1) * (size_t) depth_stride + (size_t) p->cols * de;
    const size_t bi    = with_inten ? (size_t) (p->rows - 1) * (size_t) intensity_stride + (size_t) p->cols * ie : 0;
    const size_t off_i = (bd + 63) / 64 * 64;
    if ((rc = dst->staging.reserve(off_i + bi + 64))) return rc;
    if ((rc = stage(dst, depth, bd, 0, &a.depth))) return rc;
    if (with_inten && (rc = stage(dst, intensity, bi, off_i, &a.inten))) return rc;
  }
  const bool normals = a.gc > 0;
  if (depth_type == SRRG2_IMAGE_U16) return run_adapt(dst, DepthSource<uint16_t>{a}, n, normals, with_inten, p->compact != 0, out);
  return run_adapt(dst, DepthSource<float>{a}, n, normals, with_inten, p->compact != 0, out);
}

int srrg2_adapt_laser_scan(srrg2_scene_h dst, const float* ranges, int num_beams, int mem, const srrg2_scan_adaptor_params* p,
                           srrg2_adapt_result* out) {
  if (!dst || !p) return fail(SRRG2_E_INVALID, "adapt_laser_scan: null scene or params");
  if (dst->dim != 2) return fail(SRRG2_E_INVALID, "adapt_laser_scan: the scene must have dim 2");
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, "adapt_laser_scan: bad mem");
  if (num_beams < 0 || p->normal_half_window < 0) return fail(SRRG2_E_INVALID, "adapt_laser_scan: num_beams, normal_half_window >= 0");
  if (num_beams > 0 && (!ranges || reinterpret_cast<uintptr_t>(ranges) % 4 != 0))
    return fail(SRRG2_E_INVALID, "adapt_laser_scan: null or misaligned ranges");
  // (the bearings go through a fixed argument reduction: keep them where it is exact enough and its integer part fits)
  if (!std::isfinite(p->angle_min) || !std::isfinite(p->angle_increment) ||
      std::fabs(p->angle_min) + (double) num_beams * std::fabs(p->angle_increment) > 1.0e6)
    return fail(SRRG2_E_INVALID, "adapt_laser_scan: bearings must be finite and within 1e6 rad");
  int rc;
  HIP_TRY(hipSetDevice(dst->device));
  ScanSource src;
  std::memset(&src, 0, sizeof(src));
  src.ranges = ranges;
  src.n      = num_beams;
  src.w      = p->normal_half_window;
  src.amin = p->angle_min, src.ainc = p->angle_increment;
  src.rmin = p->range_min, src.rmax = p->range_max;
  src.maxd2 = p->normal_max_distance_squared;
  src.drop  = p->drop_points_without_normal != 0;
  if (num_beams > 0 && mem == SRRG2_MEM_HOST) {
    const unsigned char* d = nullptr;
    if ((rc = dst->staging.reserve((size_t) num_beams * 4 + 64))) return rc;
    if ((rc = stage(dst, ranges, (size_t) num_beams * 4, 0, &d))) return rc;
    src.ranges = reinterpret_cast<const float*>(d);
  }
  return run_adapt(dst, src, num_beams, src.w > 0, false, p->compact != 0, out);
}

void srrg2_adapt_default_lidar_params(srrg2_lidar_adaptor_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->model.range_min             = 0.5f;
  p->model.range_max             = 120.f;
  p->normal_col_gap              = 1;
  p->normal_row_gap              = 1;
  p->normal_max_distance_squared = 1.0f;
  p->drop_points_without_normal  = 1;
  p->compact                     = 0;
}

int srrg2_spherical_model_full_turn(srrg2_spherical_model* m, int rows, int cols, double elevation_first, double elevation_last) {
  if (!m) return fail(SRRG2_E_INVALID, "spherical_model_full_turn: null model");
  if (rows < 2 || cols < 1 || !std::isfinite(elevation_first) || !std::isfinite(elevation_last) || elevation_first == elevation_last)
    return fail(SRRG2_E_INVALID, "spherical_model_full_turn: rows >= 2, cols >= 1, two finite and distinct elevations");
  const double PI = 3.141592653589793;
  std::memset(m, 0, sizeof(*m));
  m->azimuth_increment   = (2.0 * PI) / (double) cols;
  m->azimuth_min         = -PI + PI / (double) cols;
  m->elevation_min       = elevation_first;
  m->elevation_increment = (elevation_last - elevation_first) / (double) (rows - 1);
  m->rows                = rows;
  m->cols                = cols;
  m->range_min           = 0.5f;
  m->range_max           = 120.f;
  return 0;
}

void srrg2_adapt_default_lidar_sweep_extras(srrg2_lidar_sweep_extras* x) {
  if (!x) return;
  std::memset(x, 0, sizeof(*x));
  x->reference = 1.0;
  x->motion[0] = x->motion[5] = x->motion[10] = 1.f;
}

int srrg2_adapt_lidar_sweep(srrg2_scene_h dst, const float* points, int point_stride, const float* intensity, int intensity_stride,
                            int n, int mem, const srrg2_lidar_adaptor_params* p, srrg2_adapt_result* out) {
  return adapt_lidar_sweep("adapt_lidar_sweep: ", dst, points, point_stride, intensity, intensity_stride, n, mem, p, nullptr, out);
}

int srrg2_adapt_lidar_sweep_ex(srrg2_scene_h dst, const float* points, int point_stride, const float* intensity,
                               int intensity_stride, int n, int mem, const srrg2_lidar_adaptor_params* p,
                               const srrg2_lidar_sweep_extras* x, srrg2_adapt_result* out) {
  return adapt_lidar_sweep("adapt_lidar_sweep_ex: ", dst, points, point_stride, intensity, intensity_stride, n, mem, p, x, out);
}

}  // extern "C"
