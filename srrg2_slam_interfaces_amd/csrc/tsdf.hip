// tsdf.hip -- srrg2_tsdf_*: a truncated signed-distance volume from depth frames and poses, on the device.  No reference
// counterpart; DESIGN.md section 4 "TSDF volume" is the contract and tests/tsdf_restatement.py its executable form.  A frame's
// float work (centre -> camera -> pixel -> q) is float32 in the written order, no FMA; what reaches the planes are integers, so the
// planes are a function of the inputs alone, bit for bit, whatever the scheduling, the frame order or the split into calls.
//   k_tsdf_count      the depth pixels of all frames that pass the depth gate: grid-stride, one atomic per workgroup
//   k_tsdf_integrate  what the library runs.  A wave owns a run of 64 voxels along x (256-byte runs of each plane), a workgroup
//                     four consecutive runs.  The K frames of the call are the INNER loop: a voxel's three sums stay in
//                     registers, the planes are read and written once per call and only where something arrived.  A frame's
//                     matrix and frustum planes are wave-uniform (readfirstlane'd run index: scalar loads, a uniform branch); a
//                     run that the frame's frustum provably misses (frame_record below) is skipped for that frame.
//   k_tsdf_integrate_plain  -DSRRG2_TSDF_PLAIN=1: one lane per voxel, lanes along x, one launch and one pass over the planes per
//                     frame -- what the kept kernel is measured against (tools/bench_tsdf.py); the same bits.
//   k_tsdf_mask       per 8 x 8 x 8 block: does it hold a voxel with weight >= min_weight (raycast, skip_empty)
//   k_tsdf_raycast    one lane per pixel, adjacent lanes adjacent pixels of a row; the march of the contract
//   k_tsdf_flag / k_tsdf_scatter   the export: 3 flags per voxel, srrg2amd::scene_compact_into scans them, the scatter writes a
//                     kept edge's point, normal and index
// Every index into a plane or an image is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "det_math.h"
#include "device_util.h"
#include "host_util.h"
#include "scene_state.h"

using srrg2amd::fail;

#ifndef SRRG2_TSDF_PLAIN
#define SRRG2_TSDF_PLAIN 0
#endif

struct srrg2_tsdf_s {
  int device = 0;
  // the volume's stream is this scratch scene's: the export hands it to scene_compact_into as the source of the compaction
  // (its flags, scan sums and counters are the scratch of that path); it never holds points
  srrg2_scene* work = nullptr;
  hipEvent_t uploaded = nullptr;  // recorded behind the upload out of host_stage: the next call waits for it before it refills
  bool upload_pending = false;
  bool is_set         = false;
  srrg2_tsdf_params p;
  srrg2amd::DevBuf<int> planes;   // sum, weight, then (with_intensity) isum: nx*ny*nz words each
  srrg2amd::DevBuf<char> stage;   // a call's frame records, then a host call's depth images, then its intensity images
  srrg2amd::PinnedBuf<char> host_stage;
  srrg2amd::DevBuf<unsigned long long> ctr;
  srrg2amd::PinnedBuf<unsigned long long> ctr_host;
  srrg2amd::DevBuf<float> depth;            // a raycast's depth image, packed
  srrg2amd::DevBuf<unsigned char> inten;    // ... and its intensity image, packed
  srrg2amd::DevBuf<unsigned char> mask;     // ... and its block mask
  long long voxels() const { return (long long) p.nx * p.ny * p.nz; }
  hipStream_t stream() const { return work->stream; }
  ~srrg2_tsdf_s() {
    (void) hipSetDevice(device);
    if (work) (void) hipStreamSynchronize(work->stream);
    if (uploaded) (void) hipEventDestroy(uploaded);
    if (work) (void) srrg2_scene_destroy(work);
  }
};

namespace {

enum { MAX_SIDE = 2048, MASK_SIDE = 8, MAX_BLOCKS = 2048, MAX_MARCH = 1 << 20 };
enum { C_VALID = 0, C_UPDATES, C_SURFACE, C_WORDS };

struct Vol {
  int* sum;
  int* weight;
  int* isum;  // null: no intensity plane
  int nx, ny, nz;
  float ox, oy, oz, vs;
};

struct Cam {
  float fx, fy, cx, cy;
  int rows, cols;
  float scale, dmin, dmax;
};

struct Images {
  const unsigned char* depth;
  const unsigned char* inten;
  long long depth_frame, inten_frame;  // bytes from one frame's image to the next
  int depth_stride, inten_stride;
  int inten_f32;
};

// one frame as the kernels read it: world_in_camera, the six frustum planes over voxel INDICES (distance in metres, >= 0 inside)
// and the margin a run has to be beyond one of them with both ends to be skipped
struct FrameRec {
  float W[12];
  float P[6][4];
  float margin;
  float pad[3];
};
static_assert(sizeof(FrameRec) == 160, "frame records are laid out back to back in the upload");

struct Pose {
  float M[12];
};

__device__ __forceinline__ float centre(float o, int i, float vs) { return o + ((float) i + 0.5f) * vs; }

template <typename T>
__device__ __forceinline__ bool depth_of(const unsigned char* at, const Cam& C, float& d);
template <>
__device__ __forceinline__ bool depth_of<uint16_t>(const unsigned char* at, const Cam& C, float& d) {
  const uint16_t raw = *reinterpret_cast<const uint16_t*>(at);
  d = (float) raw * C.scale;
  return raw != 0 && isfinite(d) && d >= C.dmin && d <= C.dmax;  // (count 0: no reading, as the depth adaptor has it)
}
template <>
__device__ __forceinline__ bool depth_of<float>(const unsigned char* at, const Cam& C, float& d) {
  d = *reinterpret_cast<const float*>(at);
  return isfinite(d) && d >= C.dmin && d <= C.dmax;
}

// steps 2 .. 6 of the contract for the voxel centre (px, py, pz) and frame k: false = the frame adds nothing here
template <typename D, bool INTEN>
__device__ __forceinline__ bool voxel_frame(const Cam& C, const Images& I, const float* W, float mu, long long k, float px, float py,
                                            float pz, int& q, int& inten) {
  const float cx = ((W[0] * px + W[1] * py) + W[2] * pz) + W[3];
  const float cy = ((W[4] * px + W[5] * py) + W[6] * pz) + W[7];
  const float cz = ((W[8] * px + W[9] * py) + W[10] * pz) + W[11];
  if (!(cz > 0.f)) return false;
  const float uf = ((C.fx * cx) / cz + C.cx) + 0.5f, vf = ((C.fy * cy) / cz + C.cy) + 0.5f;
  if (!(uf >= 0.f && uf < (float) C.cols && vf >= 0.f && vf < (float) C.rows)) return false;  // (a NaN fails)
  const int pc = min((int) floorf(uf), C.cols - 1), pr = min((int) floorf(vf), C.rows - 1);   // (the min never acts: a guard)
  float d;
  if (!depth_of<D>(I.depth + k * I.depth_frame + (long long) pr * I.depth_stride + (long long) pc * (long long) sizeof(D), C, d))
    return false;
  const float s = d - cz;
  if (s < -mu) return false;
  const float t = fminf(s, mu);
  q = (int) floorf((t / mu) * 32767.0f + 0.5f);
  if (INTEN) {
    const unsigned char* at = I.inten + k * I.inten_frame + (long long) pr * I.inten_stride;
    if (I.inten_f32) {
      const float r = floorf(reinterpret_cast<const float*>(at)[pc] + 0.5f);
      inten = r >= 255.f ? 255 : (r > 0.f ? (int) r : 0);  // (a NaN: 0)
    } else {
      inten = at[pc];
    }
  }
  return true;
}

template <typename D>
__global__ __launch_bounds__(256) void k_tsdf_count(Cam C, Images I, long long total, unsigned long long* __restrict__ ctr) {
  unsigned long long valid = 0;
  const long long per = (long long) C.rows * C.cols;
  for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < total; i += (long long) gridDim.x * 256) {
    const long long k = i / per, at = i - k * per;
    const int r = (int) (at / C.cols), c = (int) (at - (long long) r * C.cols);
    float d;
    if (depth_of<D>(I.depth + k * I.depth_frame + (long long) r * I.depth_stride + (long long) c * (long long) sizeof(D), C, d)) ++valid;
  }
  block_add(valid, &ctr[C_VALID]);
}

// the planes take what the call's frames left in a voxel's registers (unsigned: a wrap is the int32 planes' own)
__device__ __forceinline__ void add_to_planes(const Vol& V, long long at, int weight, unsigned q, unsigned n, unsigned inten) {
  V.sum[at]    = (int) ((unsigned) V.sum[at] + (unsigned) weight * q);
  V.weight[at] = (int) ((unsigned) V.weight[at] + (unsigned) weight * n);
  if (V.isum) V.isum[at] = (int) ((unsigned) V.isum[at] + (unsigned) weight * inten);
}

// runs = nz * ny * runs_x runs of 64 voxels, run index (z ny + y) runs_x + xr; gridDim.x = ceil(runs / 4)
template <typename D, bool INTEN>
__global__ __launch_bounds__(256) void k_tsdf_integrate(Vol V, Cam C, Images I, const FrameRec* __restrict__ frames, int K, float mu,
                                                        int weight, int runs_x, long long runs, unsigned long long* __restrict__ ctr) {
  unsigned long long updates = 0;
  const long long run = (long long) blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  if (run < runs) {
    const int xr        = (int) (run % runs_x);
    const long long row = run / runs_x;
    const int y = (int) (row % V.ny), z = (int) (row / V.ny);
    const int x0 = xr * 64, x = x0 + (int) (threadIdx.x & 63);
    const bool live = x < V.nx;
    const float px = centre(V.ox, x, V.vs), py = centre(V.oy, y, V.vs), pz = centre(V.oz, z, V.vs);
    const float e0 = (float) x0, e1 = (float) min(x0 + 63, V.nx - 1), fy = (float) y, fz = (float) z;
    unsigned acc_q = 0, acc_n = 0, acc_i = 0;
    for (int k = 0; k < K; ++k) {
      const FrameRec& R = frames[k];
      // a plane's distance is affine in x along the run: below -margin at both ends, it is below -margin at every voxel between
      bool miss = false;
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        const float rest = R.P[s][1] * fy + R.P[s][2] * fz + R.P[s][3];
        miss = miss || (R.P[s][0] * e0 + rest < -R.margin && R.P[s][0] * e1 + rest < -R.margin);  // (a NaN: not skipped)
      }
      if (miss) continue;
      int q = 0, inten = 0;
      if (live && voxel_frame<D, INTEN>(C, I, R.W, mu, k, px, py, pz, q, inten)) {
        acc_q += (unsigned) q, acc_i += (unsigned) inten;
        ++acc_n;
      }
    }
    if (acc_n) {  // (a voxel that received nothing is neither read nor stored)
      add_to_planes(V, ((long long) z * V.ny + y) * V.nx + x, weight, acc_q, acc_n, acc_i);
      updates = acc_n;
    }
  }
  block_add(updates, &ctr[C_UPDATES]);
}

// frame k alone; gridDim.x = ceil(voxels / 256)
template <typename D, bool INTEN>
__global__ __launch_bounds__(256) void k_tsdf_integrate_plain(Vol V, Cam C, Images I, const FrameRec* __restrict__ frames, int k, float mu,
                                                              int weight, long long voxels, unsigned long long* __restrict__ ctr) {
  unsigned long long updates = 0;
  const long long at = (long long) blockIdx.x * 256 + threadIdx.x;
  if (at < voxels) {
    const int x         = (int) (at % V.nx);
    const long long row = at / V.nx;
    const int y = (int) (row % V.ny), z = (int) (row / V.ny);
    int q = 0, inten = 0;
    if (voxel_frame<D, INTEN>(C, I, frames[k].W, mu, k, centre(V.ox, x, V.vs), centre(V.oy, y, V.vs), centre(V.oz, z, V.vs), q, inten)) {
      add_to_planes(V, at, weight, (unsigned) q, 1u, (unsigned) inten);
      updates = 1;
    }
  }
  block_add(updates, &ctr[C_UPDATES]);
}

__global__ __launch_bounds__(256) void k_tsdf_mask(Vol V, int minw, long long voxels, int mx, int my, unsigned char* __restrict__ mask) {
  for (long long at = (long long) blockIdx.x * 256 + threadIdx.x; at < voxels; at += (long long) gridDim.x * 256) {
    if (V.weight[at] < minw) continue;
    const int x         = (int) (at % V.nx);
    const long long row = at / V.nx;
    const int y = (int) (row % V.ny), z = (int) (row / V.ny);
    mask[((long long) (z / MASK_SIDE) * my + y / MASK_SIDE) * mx + x / MASK_SIDE] = 1;  // (every writer writes 1)
  }
}

// the trilinear sample of the contract at the world point (wx, wy, wz); mask: null = the plain march
__device__ __forceinline__ bool tsdf_sample(const Vol& V, int minw, const unsigned char* __restrict__ mask, int mx, int my, float wx,
                                            float wy, float wz, float& F) {
  const float gx = (wx - V.ox) / V.vs - 0.5f, gy = (wy - V.oy) / V.vs - 0.5f, gz = (wz - V.oz) / V.vs - 0.5f;
  const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
  // all eight corners inside the volume (a NaN fails; nx = 1 has no such sample)
  if (!(bx >= 0.f && bx <= (float) (V.nx - 2) && by >= 0.f && by <= (float) (V.ny - 2) && bz >= 0.f && bz <= (float) (V.nz - 2)))
    return false;
  const int ix = (int) bx, iy = (int) by, iz = (int) bz;
  // the corner (ix, iy, iz) is one of the eight: a block without a valid voxel has no valid sample
  if (mask && !mask[((long long) (iz / MASK_SIDE) * my + iy / MASK_SIDE) * mx + ix / MASK_SIDE]) return false;
  const long long at = ((long long) iz * V.ny + iy) * V.nx + ix, sy = V.nx, sz = (long long) V.nx * V.ny;
  float f[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const long long a = at + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
    const int w       = V.weight[a];
    if (w < minw) return false;
    f[c] = (float) V.sum[a] / (float) w;
  }
  const float tx = gx - bx, ty = gy - by, tz = gz - bz;
  const float c00 = f[0] + tx * (f[1] - f[0]), c10 = f[2] + tx * (f[3] - f[2]);
  const float c01 = f[4] + tx * (f[5] - f[4]), c11 = f[6] + tx * (f[7] - f[6]);
  const float c0 = c00 + ty * (c10 - c00), c1 = c01 + ty * (c11 - c01);
  F = c0 + tz * (c1 - c0);
  return true;
}

__device__ __forceinline__ void to_world(const Pose& T, float x, float y, float z, float& wx, float& wy, float& wz) {
  wx = ((T.M[0] * x + T.M[1] * y) + T.M[2] * z) + T.M[3];
  wy = ((T.M[4] * x + T.M[5] * y) + T.M[6] * z) + T.M[7];
  wz = ((T.M[8] * x + T.M[9] * y) + T.M[10] * z) + T.M[11];
}

// last: the largest i of the march (-1: no sample); depth: rows*cols floats, inten: rows*cols bytes or null
__global__ __launch_bounds__(256) void k_tsdf_raycast(Vol V, Cam C, Pose T, float step, int last, int minw,
                                                      const unsigned char* __restrict__ mask, int mx, int my, float* __restrict__ depth,
                                                      unsigned char* __restrict__ inten, unsigned long long* __restrict__ ctr) {
  unsigned long long surface = 0;
  const long long t = (long long) blockIdx.x * 256 + threadIdx.x;
  if (t < (long long) C.rows * C.cols) {
    const int r = (int) (t / C.cols), c = (int) (t - (long long) r * C.cols);
    const float xn = ((float) c - C.cx) / C.fx, yn = ((float) r - C.cy) / C.fy;
    float Fp = 0.f, zp = 0.f, zs = 0.f;
    bool vp = false, found = false;
    for (int i = 0; i <= last; ++i) {
      const float z = C.dmin + (float) i * step;
      float wx, wy, wz, F = 0.f;
      to_world(T, xn * z, yn * z, z, wx, wy, wz);
      const bool v = tsdf_sample(V, minw, mask, mx, my, wx, wy, wz, F);
      if (vp && v && Fp > 0.f && F <= 0.f) {
        zs    = zp + (step * Fp) / (Fp - F);
        found = true;
        break;
      }
      vp = v, Fp = F, zp = z;
    }
    const bool hit = found && zs >= C.dmin && zs <= C.dmax;
    depth[t] = hit ? zs : 0.f;
    if (hit) ++surface;
    if (inten) {
      int value = 0;
      if (hit) {
        float wx, wy, wz;
        to_world(T, xn * zs, yn * zs, zs, wx, wy, wz);
        const float bx = floorf((wx - V.ox) / V.vs), by = floorf((wy - V.oy) / V.vs), bz = floorf((wz - V.oz) / V.vs);
        if (bx >= 0.f && bx <= (float) (V.nx - 1) && by >= 0.f && by <= (float) (V.ny - 1) && bz >= 0.f && bz <= (float) (V.nz - 1)) {
          const long long at = ((long long) (int) bz * V.ny + (int) by) * V.nx + (int) bx;
          const long long w = V.weight[at], s = V.isum[at];
          if (w >= 1) {
            const long long mean = (s + w / 2) / w;
            value                = mean > 255 ? 255 : (mean > 0 ? (int) mean : 0);
          }
        }
      }
      inten[t] = (unsigned char) value;
    }
  }
  block_add(surface, &ctr[C_SURFACE]);
}

// F of voxel `at` when it is valid
__device__ __forceinline__ bool voxel_value(const Vol& V, long long at, int minw, float& F) {
  const int w = V.weight[at];
  if (w < minw) return false;
  F = (float) V.sum[at] / (float) w;
  return true;
}

__device__ __forceinline__ bool crosses(float a, float b) {
  return (a < 0.f && b > 0.f) || (a > 0.f && b < 0.f) || ((a == 0.f) != (b == 0.f));
}

// flags[3 v + a]: does the edge from voxel v along +a carry a point
__global__ __launch_bounds__(256) void k_tsdf_flag(Vol V, int minw, long long voxels, int* __restrict__ flags) {
  const long long stride[3] = {1, V.nx, (long long) V.nx * V.ny};
  for (long long at = (long long) blockIdx.x * 256 + threadIdx.x; at < voxels; at += (long long) gridDim.x * 256) {
    const int x         = (int) (at % V.nx);
    const long long row = at / V.nx;
    const int idx[3] = {x, (int) (row % V.ny), (int) (row / V.ny)}, side[3] = {V.nx, V.ny, V.nz};
    float F0 = 0.f;
    const bool v0 = voxel_value(V, at, minw, F0);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float F1 = 0.f;
      flags[3 * at + a] = v0 && idx[a] + 1 < side[a] && voxel_value(V, at + stride[a], minw, F1) && crosses(F0, F1) ? 1 : 0;
    }
  }
}

// behind the scan of the flags: a kept edge e = 3 v + a goes to slot offset[e]; the k >= cap guard is the clippers'
__global__ __launch_bounds__(256) void k_tsdf_scatter(Vol V, int minw, long long entries, const int* __restrict__ offset,
                                                      float4* __restrict__ out_pts, float4* __restrict__ out_nrm, int* __restrict__ gidx,
                                                      int cap) {
  const long long stride[3] = {1, V.nx, (long long) V.nx * V.ny};
  for (long long e = (long long) blockIdx.x * 256 + threadIdx.x; e < entries; e += (long long) gridDim.x * 256) {
    const int k = offset[e];
    if (offset[e + 1] == k || k >= cap) continue;
    const long long at = e / 3;
    const int a        = (int) (e - 3 * at);
    const int x         = (int) (at % V.nx);
    const long long row = at / V.nx;
    const int idx[3] = {x, (int) (row % V.ny), (int) (row / V.ny)}, side[3] = {V.nx, V.ny, V.nz};
    float F0 = 0.f, F1 = 0.f;
    (void) voxel_value(V, at, minw, F0);
    (void) voxel_value(V, at + stride[a], minw, F1);
    const float o[3] = {V.ox, V.oy, V.oz};
    float p[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) p[b] = b == a ? o[b] + (((float) idx[b] + 0.5f) + F0 / (F0 - F1)) * V.vs : centre(o[b], idx[b], V.vs);
    float g[3];
    bool whole = true;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      float lo = 0.f, hi = 0.f;
      whole = whole && idx[b] >= 1 && idx[b] + 1 < side[b] && voxel_value(V, at - stride[b], minw, lo) &&
              voxel_value(V, at + stride[b], minw, hi);
      g[b] = hi - lo;
    }
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const float qn  = __int_as_float(0x7fc00000);
    const bool ok   = whole && len > 0.f;
    out_pts[k] = make_float4(p[0], p[1], p[2], 0.f);
    out_nrm[k] = ok ? make_float4(g[0] / len, g[1] / len, g[2] / len, 0.f) : make_float4(qn, qn, qn, 0.f);
    gidx[k]    = (int) e;
  }
}

int blocks_of(long long n) { return (int) std::min<long long>((n + 255) / 256, MAX_BLOCKS); }

Vol vol_of(const srrg2_tsdf_s* h) {
  const long long n = h->voxels();
  return Vol{h->planes.p, h->planes.p + n, h->p.with_intensity ? h->planes.p + 2 * n : nullptr, h->p.nx, h->p.ny, h->p.nz,
             h->p.origin[0], h->p.origin[1], h->p.origin[2], h->p.voxel_size};
}

bool aligned_to(const void* p, long long stride, int elem) {
  return reinterpret_cast<uintptr_t>(p) % (uintptr_t) elem == 0 && stride % elem == 0;
}

bool positive(float v) { return std::isfinite(v) && v > 0.f; }

int check_volume_params(const std::string& who, const srrg2_tsdf_params* p) {
  if (!p) return fail(SRRG2_E_INVALID, who + "null params");
  if (p->nx < 0 || p->ny < 0 || p->nz < 0 || p->nx > MAX_SIDE || p->ny > MAX_SIDE || p->nz > MAX_SIDE)
    return fail(SRRG2_E_INVALID, who + "nx, ny and nz must lie in 0 .. 2048");
  if (p->with_intensity != 0 && p->with_intensity != 1) return fail(SRRG2_E_INVALID, who + "with_intensity must be 0 or 1");
  if (!positive(p->voxel_size)) return fail(SRRG2_E_INVALID, who + "voxel_size must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(p->origin[i])) return fail(SRRG2_E_INVALID, who + "origin must be finite");
  if ((long long) p->nx * p->ny * p->nz > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "nx * ny * nz beyond int32");
  return 0;
}

// what srrg2_adapt_depth_image refuses of its params, with its codes (`gaps`: the raycast hands them on; a frame does not read them)
int check_camera(const std::string& who, const srrg2_depth_adaptor_params* p, bool gaps) {
  if (!p) return fail(SRRG2_E_INVALID, who + "null camera params");
  if (p->rows < 0 || p->cols < 0 || (long long) p->rows * (long long) p->cols > 0x7fffffffLL)
    return fail(SRRG2_E_INVALID, who + "rows, cols >= 0 and rows*cols within int32");
  if (gaps && (p->normal_col_gap < 0 || p->normal_row_gap < 0 || (p->normal_col_gap == 0) != (p->normal_row_gap == 0)))
    return fail(SRRG2_E_INVALID, who + "normal gaps >= 0, and both or neither 0");
  const float fx = p->camera_matrix[0], fy = p->camera_matrix[4];
  if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.f || fy == 0.f)
    return fail(SRRG2_E_INVALID, who + "fx and fy must be finite and non-zero");
  if (p->camera_matrix[1] != 0.f) return fail(SRRG2_E_UNSUPPORTED, who + "a camera matrix with skew (K[0][1] != 0)");
  return 0;
}

int check_pose(const std::string& who, const float* T) {
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T[i])) return fail(SRRG2_E_INVALID, who + "camera_in_world must be finite");
  return 0;
}

int tsdf_ready(const std::string& who, srrg2_tsdf_s* h) {
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  if (!h->is_set) return fail(SRRG2_E_INVALID, who + "no volume (srrg2_tsdf_reset)");
  return 0;
}

Cam cam_of(const srrg2_depth_adaptor_params* p) {
  return Cam{p->camera_matrix[0], p->camera_matrix[4], p->camera_matrix[2], p->camera_matrix[5], p->rows, p->cols, p->depth_scale,
             p->depth_min, p->depth_max};
}

// The frame record of one pose: world_in_camera and the frustum over voxel indices.  A voxel the per-voxel float32 arithmetic
// updates has c.z > 0, 0 <= u + 0.5 < cols, 0 <= v + 0.5 < rows and c.z <= depth_max + mu in float32.  The planes below are those
// conditions in exact arithmetic, the image widened by `widen` pixels on every side (more than the rounding of u and v: four
// operations on magnitudes <= |K2| + cols + 2), normalised to metres in the camera frame and written over (x, y, z, 1) of the voxel
// INDEX.  A float32 camera point differs from the exact affine image of the index by less than 2^-21 B per coordinate (B: the sum
// over the rows of sum |W_ra| max |p_a| + |W_r3|, plus depth_max + mu; 8 roundings of terms <= B), the kernel's float32 plane
// value by less than 2^-22 B more.  margin = 2^-18 B + one voxel's reach in the camera frame: a run whose two ends are both
// beyond a plane by more than that has no voxel the per-voxel arithmetic could update (DESIGN.md section 4 "TSDF volume").
// Anything not finite gives a NaN or infinite margin: the run is never skipped.
FrameRec frame_record(const srrg2_tsdf_params& v, const Cam& C, float mu, const float* camera_in_world) {
  FrameRec R;
  std::memset(&R, 0, sizeof(R));
  dm::se3_inverse(camera_in_world, R.W);
  double W[12], reach = 0.0, B = 0.0;
  for (int i = 0; i < 12; ++i) W[i] = R.W[i];
  const int side[3] = {v.nx, v.ny, v.nz};
  for (int r = 0; r < 3; ++r) {
    double row = std::fabs(W[4 * r + 3]), step = 0.0;
    for (int a = 0; a < 3; ++a) {
      row += std::fabs(W[4 * r + a]) * (std::fabs((double) v.origin[a]) + (side[a] + 1.0) * v.voxel_size);
      step += std::fabs(W[4 * r + a]) * v.voxel_size;
    }
    B += row, reach += step;
  }
  B += std::fabs((double) C.dmax) + mu;
  R.margin = (float) (std::ldexp(B, -18) + reach);
  const double wu = 1.0 + std::ldexp(std::fabs((double) C.cx) + C.cols + 2.0, -19);
  const double wv = 1.0 + std::ldexp(std::fabs((double) C.cy) + C.rows + 2.0, -19);
  const double N[6][4] = {{0, 0, 1, 0},
                          {0, 0, -1, (double) C.dmax + mu},
                          {(double) C.fx, 0, (double) C.cx + 0.5 + wu, 0},
                          {-(double) C.fx, 0, C.cols + wu - 0.5 - (double) C.cx, 0},
                          {0, (double) C.fy, (double) C.cy + 0.5 + wv, 0},
                          {0, -(double) C.fy, C.rows + wv - 0.5 - (double) C.cy, 0}};
  for (int s = 0; s < 6; ++s) {
    const double len = std::sqrt(N[s][0] * N[s][0] + N[s][1] * N[s][1] + N[s][2] * N[s][2]);
    double n[3] = {N[s][0] / len, N[s][1] / len, N[s][2] / len}, at_origin = N[s][3] / len;
    for (int a = 0; a < 3; ++a) {
      const double g = n[0] * W[a] + n[1] * W[4 + a] + n[2] * W[8 + a];  // per metre along world axis a
      R.P[s][a] = (float) (g * v.voxel_size);
      at_origin += g * ((double) v.origin[a] + 0.5 * v.voxel_size);
    }
    at_origin += n[0] * W[3] + n[1] * W[7] + n[2] * W[11];
    R.P[s][3] = (float) at_origin;
  }
  return R;
}

template <typename D>
void launch_integrate(srrg2_tsdf_s* h, const Cam& C, const Images& I, const FrameRec* frames, int K, float mu, int weight) {
  const Vol V      = vol_of(h);
  const bool inten = V.isum != nullptr;
  hipStream_t st   = h->stream();
#if SRRG2_TSDF_PLAIN
  const long long n = h->voxels();
  const dim3 grid((unsigned) ((n + 255) / 256));
  for (int k = 0; k < K; ++k) {
    if (inten)
      hipLaunchKernelGGL((k_tsdf_integrate_plain<D, true>), grid, dim3(256), 0, st, V, C, I, frames, k, mu, weight, n, h->ctr.p);
    else
      hipLaunchKernelGGL((k_tsdf_integrate_plain<D, false>), grid, dim3(256), 0, st, V, C, I, frames, k, mu, weight, n, h->ctr.p);
  }
#else
  const int runs_x     = (V.nx + 63) / 64;
  const long long runs = (long long) V.nz * V.ny * runs_x;  // (<= 2^31: the grid fits)
  const dim3 grid((unsigned) ((runs + 3) / 4));
  if (inten)
    hipLaunchKernelGGL((k_tsdf_integrate<D, true>), grid, dim3(256), 0, st, V, C, I, frames, K, mu, weight, runs_x, runs, h->ctr.p);
  else
    hipLaunchKernelGGL((k_tsdf_integrate<D, false>), grid, dim3(256), 0, st, V, C, I, frames, K, mu, weight, runs_x, runs, h->ctr.p);
#endif
}

}  // namespace

extern "C" int srrg2_tsdf_create(int device, srrg2_tsdf_h* out) {
  if (!out) return fail(SRRG2_E_INVALID, "tsdf_create: out is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SRRG2_E_NO_DEVICE, "tsdf_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(SRRG2_E_INVALID, "tsdf_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<srrg2_tsdf_s> h(new srrg2_tsdf_s());  // (a failure below deletes it)
  h->device = device;
  srrg2_tsdf_default_params(&h->p);
  int rc;
  if ((rc = srrg2_scene_create(3, device, &h->work))) return rc;
  h->work->has_normals = true;  // (what the export's destination takes over: its points come with normals)
  HIP_TRY(hipEventCreateWithFlags(&h->uploaded, hipEventDisableTiming));
  if ((rc = h->ctr.reserve(C_WORDS)) || (rc = h->ctr_host.reserve(C_WORDS))) return rc;
  *out = h.release();
  return 0;
}

extern "C" int srrg2_tsdf_destroy(srrg2_tsdf_h h) {
  delete h;  // (null: nothing to do)
  return 0;
}

extern "C" void srrg2_tsdf_default_params(srrg2_tsdf_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->voxel_size = 0.02f;
}

extern "C" void srrg2_tsdf_default_frame_params(srrg2_tsdf_frame_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->mu = 0.06f;
}

extern "C" void srrg2_tsdf_default_raycast_params(srrg2_tsdf_raycast_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->step       = 0.02f;
  p->min_weight = 1;
  p->skip_empty = 0;  // (the mask did not pay on a volume the camera stands in: DESIGN.md section 4 "TSDF volume")
}

extern "C" int srrg2_tsdf_reset(srrg2_tsdf_h h, const srrg2_tsdf_params* p) {
  const std::string who = "tsdf_reset: ";
  int rc;
  if ((rc = check_volume_params(who, p))) return rc;  // (the parameters first: what they are refused for needs no handle)
  if (!h) return fail(SRRG2_E_INVALID, who + "null handle");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = (size_t) p->nx * (size_t) p->ny * (size_t) p->nz, planes = p->with_intensity ? 3 : 2;
  HIP_TRY(hipStreamSynchronize(h->stream()));  // (queued work still adds into the old planes)
  h->upload_pending = false;
  h->is_set         = false;
  if ((rc = h->planes.reserve(planes * n + 4))) return rc;
  if (n > 0) HIP_TRY(hipMemsetAsync(h->planes.p, 0, planes * n * sizeof(int), h->stream()));
  h->p      = *p;
  h->is_set = true;
  return 0;
}

extern "C" int srrg2_tsdf_integrate_frames(srrg2_tsdf_h h, const void* depth, int depth_type, int depth_stride, const void* intensity,
                                           int intensity_type, int intensity_stride, int num_frames, const float* camera_in_world, int mem,
                                           const srrg2_depth_adaptor_params* cam, const srrg2_tsdf_frame_params* fp, int weight,
                                           srrg2_tsdf_result* out) {
  const std::string who = "tsdf_integrate_frames: ";
  int rc;
  if (!fp) return fail(SRRG2_E_INVALID, who + "null frame params");
  if ((rc = check_camera(who, cam, false))) return rc;
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (weight != 1 && weight != -1) return fail(SRRG2_E_INVALID, who + "weight must be +1 or -1");
  if (num_frames < 0) return fail(SRRG2_E_INVALID, who + "num_frames >= 0");
  if (depth_type != SRRG2_IMAGE_U16 && depth_type != SRRG2_IMAGE_F32)
    return fail(SRRG2_E_INVALID, who + "depth_type must be SRRG2_IMAGE_U16 or SRRG2_IMAGE_F32");
  if (intensity_type != SRRG2_IMAGE_NONE && intensity_type != SRRG2_IMAGE_U8 && intensity_type != SRRG2_IMAGE_F32)
    return fail(SRRG2_E_INVALID, who + "intensity_type must be NONE, U8 or F32");
  if (!positive(fp->mu)) return fail(SRRG2_E_INVALID, who + "mu must be finite and > 0");
  if (fp->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  const long long pixels = (long long) cam->rows * cam->cols;
  const int de = depth_type == SRRG2_IMAGE_U16 ? 2 : 4, ie = intensity_type == SRRG2_IMAGE_F32 ? 4 : 1;
  const bool with_inten = intensity_type != SRRG2_IMAGE_NONE;
  if (num_frames > 0) {
    if (!camera_in_world) return fail(SRRG2_E_INVALID, who + "null poses");
    for (int k = 0; k < num_frames; ++k)
      if ((rc = check_pose(who, camera_in_world + 12 * (size_t) k))) return rc;
  }
  if (num_frames > 0 && pixels > 0) {
    if (!depth || (with_inten && !intensity)) return fail(SRRG2_E_INVALID, who + "null image");
    if ((long long) depth_stride < (long long) cam->cols * de || !aligned_to(depth, depth_stride, de))
      return fail(SRRG2_E_INVALID, who + "depth row stride smaller than a row, or image not aligned to its element");
    if (with_inten && ((long long) intensity_stride < (long long) cam->cols * ie || !aligned_to(intensity, intensity_stride, ie)))
      return fail(SRRG2_E_INVALID, who + "intensity row stride smaller than a row, or image not aligned to its element");
  }
  if ((rc = tsdf_ready(who, h))) return rc;
  if (with_inten != (h->p.with_intensity != 0))
    return fail(SRRG2_E_INVALID, who + (with_inten ? "an intensity image for a volume without the intensity plane"
                                                   : "a volume with the intensity plane needs an intensity image"));
  srrg2_tsdf_result res;
  std::memset(&res, 0, sizeof(res));
  res.num_frames = num_frames;
  res.num_pixels = (long long) num_frames * pixels;
  if (num_frames == 0 || pixels == 0) {
    if (out) *out = res;
    return 0;
  }
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  const Cam C    = cam_of(cam);
  const int K    = num_frames;
  // ONE upload through the pinned block: the frame records, then -- a host call -- the depth images and the intensity images
  const size_t rows_all = (size_t) K * (size_t) cam->rows;
  const size_t bf       = (size_t) K * sizeof(FrameRec);
  const bool host       = mem == SRRG2_MEM_HOST;
  const size_t bd       = host ? (rows_all - 1) * (size_t) depth_stride + (size_t) cam->cols * de : 0;
  const size_t bi       = host && with_inten ? (rows_all - 1) * (size_t) intensity_stride + (size_t) cam->cols * ie : 0;
  const size_t off_d = (bf + 63) / 64 * 64, off_i = (off_d + bd + 63) / 64 * 64, bytes = off_i + bi;
  if (h->upload_pending) {
    HIP_TRY(hipEventSynchronize(h->uploaded));
    h->upload_pending = false;
  }
  if ((rc = h->host_stage.reserve(bytes, bytes / 8)) || (rc = h->stage.reserve(bytes))) return rc;
  FrameRec* const recs = reinterpret_cast<FrameRec*>(h->host_stage.p);
  for (int k = 0; k < K; ++k) recs[k] = frame_record(h->p, C, fp->mu, camera_in_world + 12 * (size_t) k);
  if (host) {
    std::memcpy(h->host_stage.p + off_d, depth, bd);
    if (with_inten) std::memcpy(h->host_stage.p + off_i, intensity, bi);
  }
  HIP_TRY(hipMemcpyAsync(h->stage.p, h->host_stage.p, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(h->uploaded, st));
  h->upload_pending = true;
  Images I;
  std::memset(&I, 0, sizeof(I));
  I.depth        = host ? reinterpret_cast<const unsigned char*>(h->stage.p + off_d) : static_cast<const unsigned char*>(depth);
  I.inten        = !with_inten ? nullptr
                               : (host ? reinterpret_cast<const unsigned char*>(h->stage.p + off_i) : static_cast<const unsigned char*>(intensity));
  I.depth_stride = depth_stride, I.inten_stride = intensity_stride;
  I.depth_frame  = (long long) cam->rows * depth_stride;
  I.inten_frame  = (long long) cam->rows * intensity_stride;
  I.inten_f32    = intensity_type == SRRG2_IMAGE_F32;
  const FrameRec* const frames = reinterpret_cast<const FrameRec*>(h->stage.p);
  HIP_TRY(hipMemsetAsync(h->ctr.p, 0, C_WORDS * sizeof(unsigned long long), st));
  const bool u16 = depth_type == SRRG2_IMAGE_U16;
  if (u16)
    hipLaunchKernelGGL(k_tsdf_count<uint16_t>, dim3(blocks_of(res.num_pixels)), dim3(256), 0, st, C, I, res.num_pixels, h->ctr.p);
  else
    hipLaunchKernelGGL(k_tsdf_count<float>, dim3(blocks_of(res.num_pixels)), dim3(256), 0, st, C, I, res.num_pixels, h->ctr.p);
  if (h->voxels() > 0) {
    if (u16)
      launch_integrate<uint16_t>(h, C, I, frames, K, fp->mu, weight);
    else
      launch_integrate<float>(h, C, I, frames, K, fp->mu, weight);
  }
  HIP_TRY(hipGetLastError());
  if (!out) return 0;
  HIP_TRY(hipMemcpyAsync(h->ctr_host.p, h->ctr.p, C_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait
  h->upload_pending     = false;
  res.num_valid_depth   = (int64_t) h->ctr_host.p[C_VALID];
  res.num_voxel_updates = (int64_t) h->ctr_host.p[C_UPDATES];
  *out = res;
  return 0;
}

extern "C" int srrg2_tsdf_raycast(srrg2_tsdf_h h, const float* camera_in_world, const srrg2_depth_adaptor_params* cam,
                                  const srrg2_tsdf_raycast_params* rp, srrg2_scene_h dst, float* depth_out, int depth_mem,
                                  srrg2_tsdf_raycast_result* out) {
  const std::string who = "tsdf_raycast: ";
  int rc;
  if (!rp) return fail(SRRG2_E_INVALID, who + "null raycast params");
  if ((rc = check_camera(who, cam, true))) return rc;
  if (!camera_in_world) return fail(SRRG2_E_INVALID, who + "null pose");
  if ((rc = check_pose(who, camera_in_world))) return rc;
  if (depth_mem != SRRG2_MEM_HOST && depth_mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (!positive(rp->step)) return fail(SRRG2_E_INVALID, who + "step must be finite and > 0");
  if (rp->min_weight < 1) return fail(SRRG2_E_INVALID, who + "min_weight >= 1");
  if (rp->skip_empty != 0 && rp->skip_empty != 1) return fail(SRRG2_E_INVALID, who + "skip_empty must be 0 or 1");
  if (rp->reserved != 0) return fail(SRRG2_E_INVALID, who + "reserved must be 0");
  const float span = floorf((cam->depth_max - cam->depth_min) / rp->step);  // (float32, as the contract counts the samples)
  if (!(span <= (float) MAX_MARCH)) return fail(SRRG2_E_INVALID, who + "(depth_max - depth_min) / step must be a number and <= 2^20");
  if (depth_out && reinterpret_cast<uintptr_t>(depth_out) % 4 != 0) return fail(SRRG2_E_INVALID, who + "misaligned depth_out");
  if ((rc = tsdf_ready(who, h))) return rc;
  if (dst && (dst->dim != 3 || dst->device != h->device)) return fail(SRRG2_E_INVALID, who + "dst must be a 3-D scene on the volume's device");
  const int last       = span >= 0.f ? (int) span : -1;
  const long long n    = (long long) cam->rows * cam->cols;
  const bool inten     = h->p.with_intensity != 0;
  srrg2_tsdf_raycast_result res;
  std::memset(&res, 0, sizeof(res));
  res.num_pixels = (int) n;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  if (n > 0) {
    if ((rc = h->depth.reserve((size_t) n)) || (inten && (rc = h->inten.reserve((size_t) n)))) return rc;
    const Vol V  = vol_of(h);
    const Cam C  = cam_of(cam);
    const int mx = (V.nx + MASK_SIDE - 1) / MASK_SIDE, my = (V.ny + MASK_SIDE - 1) / MASK_SIDE, mz = (V.nz + MASK_SIDE - 1) / MASK_SIDE;
    const unsigned char* mask = nullptr;
    if (rp->skip_empty && h->voxels() > 0) {
      const size_t blocks = (size_t) mx * my * mz;
      if ((rc = h->mask.reserve(blocks))) return rc;
      HIP_TRY(hipMemsetAsync(h->mask.p, 0, blocks, st));
      hipLaunchKernelGGL(k_tsdf_mask, dim3(blocks_of(h->voxels())), dim3(256), 0, st, V, rp->min_weight, h->voxels(), mx, my, h->mask.p);
      mask = h->mask.p;
    }
    Pose T;
    std::memcpy(T.M, camera_in_world, sizeof(T.M));
    HIP_TRY(hipMemsetAsync(h->ctr.p, 0, C_WORDS * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, V, C, T, rp->step, last, rp->min_weight, mask,
                       mx, my, h->depth.p, inten ? h->inten.p : nullptr, h->ctr.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->ctr_host.p, h->ctr.p, C_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));  // (the adaptor reads the images on the scene's stream: they are complete)
  h->upload_pending = false;
  if (n > 0) res.num_surface = (int) h->ctr_host.p[C_SURFACE];
  if (dst) {
    if ((rc = srrg2_adapt_depth_image(dst, n > 0 ? h->depth.p : nullptr, SRRG2_IMAGE_F32, 4 * cam->cols, n > 0 && inten ? h->inten.p : nullptr,
                                      inten ? SRRG2_IMAGE_U8 : SRRG2_IMAGE_NONE, cam->cols, SRRG2_MEM_DEVICE, cam, &res.adapt)))
      return rc;
  }
  if (depth_out && n > 0)
    HIP_TRY(hipMemcpy(depth_out, h->depth.p, (size_t) n * sizeof(float),
                      depth_mem == SRRG2_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
  if (out) *out = res;
  return 0;
}

extern "C" int srrg2_tsdf_to_scene(srrg2_tsdf_h h, int min_weight, srrg2_scene_h dst, srrg2_tsdf_export_result* out) {
  const std::string who = "tsdf_to_scene: ";
  if (min_weight < 1) return fail(SRRG2_E_INVALID, who + "min_weight >= 1");
  int rc;
  if ((rc = tsdf_ready(who, h))) return rc;
  if (!dst) return fail(SRRG2_E_INVALID, who + "null scene");
  if (!srrg2amd::scene_clip_pair(h->work, dst)) return fail(SRRG2_E_INVALID, who + "dst must be a 3-D scene on the volume's device");
  const long long voxels = h->voxels(), entries = 3 * voxels;
  if (entries > 0x7fffffffLL - 1) return fail(SRRG2_E_UNSUPPORTED, who + "3 * nx * ny * nz beyond int32");
  srrg2_scene* const s = h->work;
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = srrg2amd::scene_clip_begin(s, dst))) return rc;  // (dst: normals, no features, empty until the call has succeeded)
  // (arrays even for an empty result, as the clippers leave them)
  if ((rc = srrg2amd::scene_make_room(dst, 1, 0)) || (rc = dst->gidx.reserve(1))) return rc;
  if (out) out->num_points = 0, out->reserved = 0;
  if (voxels == 0) return 0;
  if ((rc = s->flags.reserve((size_t) entries + 1))) return rc;
  hipStream_t st = h->stream();
  const Vol V    = vol_of(h);
  hipLaunchKernelGGL(k_tsdf_flag, dim3(blocks_of(voxels)), dim3(256), 0, st, V, min_weight, voxels, s->flags.p);
  HIP_TRY(hipGetLastError());
  const auto scatter = [&](int cap) {
    hipLaunchKernelGGL(k_tsdf_scatter, dim3(blocks_of(entries)), dim3(256), 0, st, V, min_weight, entries, s->flags.p, dst->pts.p,
                       dst->nrm.p, dst->gidx.p, cap);
  };
  rc = srrg2amd::scene_compact_into(s, dst, (int) entries, scatter, nullptr);
  h->upload_pending = false;
  if (!rc && out) out->num_points = dst->n;
  return rc;
}

extern "C" int srrg2_tsdf_get_planes(srrg2_tsdf_h h, int32_t* sum, int32_t* weight, int32_t* isum, int mem) {
  const std::string who = "tsdf_get_planes: ";
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  int rc;
  if ((rc = tsdf_ready(who, h))) return rc;
  if (isum && !h->p.with_intensity) return fail(SRRG2_E_INVALID, who + "the volume has no intensity plane");
  const size_t n = (size_t) h->voxels();
  if (n == 0 || (!sum && !weight && !isum)) return 0;
  HIP_TRY(hipSetDevice(h->device));
  const hipMemcpyKind kind = mem == SRRG2_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  int32_t* const to[3]     = {sum, weight, isum};
  for (int i = 0; i < 3; ++i)
    if (to[i]) HIP_TRY(hipMemcpyAsync(to[i], h->planes.p + i * n, n * sizeof(int), kind, h->stream()));
  HIP_TRY(hipStreamSynchronize(h->stream()));
  h->upload_pending = false;
  return 0;
}

extern "C" int srrg2_tsdf_device_arrays(srrg2_tsdf_h h, const int32_t** sum, const int32_t** weight, const int32_t** isum) {
  const std::string who = "tsdf_device_arrays: ";
  if (!sum || !weight) return fail(SRRG2_E_INVALID, who + "null output");
  int rc;
  if ((rc = tsdf_ready(who, h))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream()));  // (the arrays go to another stream: queued work has to be done)
  h->upload_pending = false;
  *sum    = h->planes.p;
  *weight = h->planes.p + h->voxels();
  if (isum) *isum = h->p.with_intensity ? h->planes.p + 2 * h->voxels() : nullptr;
  return 0;
}
