// normals.hip -- srrg2_scene_estimate_normals: radius-neighbourhood PCA normals for scenes that arrive as a plain list of points
// (a 3-D lidar sweep, a map from disk, a merged map whose averaged normals have drifted).  No reference counterpart; DESIGN.md
// section 4 "Normals of unorganised scenes" is the arithmetic contract and tests/normals_restatement.py its executable form: the
// result is a function of the points, the radius and the scene size alone, bit for bit.
//   k_grid_bbox / k_grid_spec / k_grid_keys   (cell_grid.h) box of the finite points, the cells' layout in the 64-bit key, a
//                   cell key per point; non-finite points get the all-ones key and sort to the end
//   (radix sort of (key, index) pairs: hipcub)
//   k_nrm_gather    the points in cell order, .w = index in the scene
//   k_nrm_neigh     THE pass: one wave per 64 consecutive sorted queries -- membership, fixed-point moments, covariance,
//                   Jacobi, orientation; details at the kernel
//   k_nrm_flag / k_nrm_scatter   drop_points_without_normal: stable compaction by exclusive scan, features carried
// The search is exact whatever the cells are: membership is decided by the float32 distance alone, the cells only bound where
// members can lie (cell side radius * (1 + 2^-16) in float64: two members' cells differ by at most one per axis).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "cell_grid.h"
#include "device_types.h"
#include "host_util.h"
#include "kernels.h"
#include "scene_device.h"
#include "scene_state.h"

using srrg2amd::fail;

namespace {

// points per LDS tile of k_nrm_neigh: one candidate per lane and load, 1 KB per wave.  A cell (or a row of cells) with more
// points goes through the tile as many times as it takes.
#define SRRG2_NRM_TILE 64
// cyclic Jacobi sweeps over (0,1), (0,2), (1,2): DESIGN.md section 4
#define SRRG2_NRM_SWEEPS 6
// counters block (ints): the grid's words (cell_grid.h: [0] finite points, [5] beyond the key range, [8, 14) the box) and, in
// between, [1] with normal, [2] too few, [3] degenerate, [4] too curved, [6] scan total
enum { C_FINITE = GRID_FINITE, C_NORMAL = 1, C_FEW = 2, C_DEGEN = 3, C_CURVED = 4, C_UNSUP = GRID_UNSUP, C_TOTAL = 6, C_WORDS = GRID_WORDS };

typedef GridSpec NrmSpec;

struct NrmArgs {
  float r2;               // one float32 product
  double scale1, scale2;  // 2^e1, 2^e2
  double inv1, inv2;      // 2^-e1, 2^-e2
  int min_neighbours;
  float max_curvature;
  int has_viewpoint;
  double vp[3];
  int nan_if_unsupported;  // the call returns before the host knows: the normals become NaN instead of staying stale
};

__global__ __launch_bounds__(256) void k_nrm_gather(const NrmSpec* __restrict__ spec, const float4* __restrict__ pts,
                                                    const int* __restrict__ sidx, int n, float4* __restrict__ sorted) {
  if (spec->unsupported) return;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const int i    = sidx[s];
    const float4 p = pts[i];
    sorted[s]      = make_float4(p.x, p.y, p.z, __int_as_float(i));
  }
}

// one Jacobi rotation on the pair (p, q) of a symmetric 3x3 (r: the third index) and the eigenvector columns p, q.
// Only + - * / sqrt, in this order; skipped when a_pq is exactly 0.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                           double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double at    = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t     = (theta >= 0.0 ? 1.0 : -1.0) / at;
  const double c     = 1.0 / sqrt(t * t + 1.0);
  const double s     = t * c;
  const double tap   = t * apq;
  app                = app - tap;
  aqq                = aqq + tap;
  apq                = 0.0;
  double a = arp, b = arq;
  arp = c * a - s * b;
  arq = s * a + c * b;
  a = v0p, b = v0q;
  v0p = c * a - s * b;
  v0q = s * a + c * b;
  a = v1p, b = v1q;
  v1p = c * a - s * b;
  v1q = s * a + c * b;
  a = v2p, b = v2q;
  v2p = c * a - s * b;
  v2q = s * a + c * b;
}

__device__ __forceinline__ int lower_bound_key(const unsigned long long* __restrict__ keys, int n, unsigned long long target,
                                               bool upper) {
  int lo = 0, hi = n;  // first position with key >= target (upper: > target)
  while (lo < hi) {
    const int mid              = (int) (((unsigned) lo + (unsigned) hi) >> 1);
    const unsigned long long k = keys[mid];
    if (upper ? k <= target : k < target)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The neighbourhood pass.  A workgroup is ONE wave and owns 64 consecutive queries of the cell-sorted cloud.  Sorted by
// (z, y, x) cell, its queries fall into a few ROWS of cells (same y and z cell); the lanes of one row are served together:
//   - the candidates of a row of queries [cx_lo, cx_hi] are the 3 (2-D) or 9 (3-D) key ranges
//     [key(cx_lo - 1, y', z'), key(cx_hi + 1, y', z')], y' = y - 1 .. y + 1, z' alike: 2 binary searches each over the sorted keys,
//     one per lane, all at once;
//   - every range streams through an LDS tile of SRRG2_NRM_TILE points, loaded coalesced, read back by broadcast: each
//     candidate is fetched once per wave, not once per query;
//   - a lane tests every candidate (float32, the gated finder's order) and adds a member's ten terms as integers: the fused
//     multiply-add onto 1.5 * 2^52 of the ICP reduction rounds each term once, the bit patterns are summed
//     with wrapping 64-bit adds and count * bits(1.5 * 2^52) comes off at the end.
// Nine 64-bit sums, the count and the float64 solve live in registers: scalars with fixed names, no indexed arrays, no scratch.
template <int DIM>
__global__ __launch_bounds__(64) void k_nrm_neigh(const NrmSpec* __restrict__ spec, const unsigned long long* __restrict__ skeys,
                                                  const float4* __restrict__ sorted, int n, NrmArgs A,
                                                  float4* __restrict__ out_nrm, float* __restrict__ out_curv,
                                                  int* __restrict__ ctr) {
  __shared__ float4 tile[SRRG2_NRM_TILE];
  __shared__ int rng[18];
  const NrmSpec S = *spec;
  const int lane  = threadIdx.x;
  const int s     = blockIdx.x * 64 + lane;
  const float fnan = __uint_as_float(0x7fc00000u);
  if (S.unsupported) {
    if (A.nan_if_unsupported && s < n) out_nrm[s] = make_float4(fnan, fnan, DIM == 3 ? fnan : 0.f, 0.f);
    return;
  }
  const int nf = S.nfinite;
  const bool active            = s < nf;
  const float4 me              = s < n ? sorted[s] : make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned long long key = active ? skeys[s] : ~0ull;
  const int NROWS              = DIM == 3 ? 9 : 3;
  const unsigned long long row = key >> S.shift[1];  // (shifts <= 60: k_grid_spec)
  const int cx                 = (int) (key & ((1ull << S.shift[1]) - 1ull));

  unsigned long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
  int cnt = 0;
  const double MAGIC = 6755399441055744.0;  // 1.5 * 2^52

  unsigned long long pending = __ballot(active);
  while (pending) {
    const int leader             = __ffsll((long long) pending) - 1;
    const unsigned long long cur = __shfl(row, leader);
    const bool mine              = active && row == cur;
    const unsigned long long grp = __ballot(mine);
    pending &= ~grp;
    const int last  = 63 - __clzll((long long) grp);
    const int cx_lo = __shfl(cx, leader), cx_hi = __shfl(cx, last);  // (sorted: the first lane of a row has its smallest x cell)
    __syncthreads();  // (the ranges of the row before have been read)
    if (lane < 2 * NROWS) {
      const int r  = lane >> 1;
      const int ybits = S.shift[2] - S.shift[1];
      const int cy    = (int) (cur & ((1ull << ybits) - 1ull));
      const int cz    = DIM == 3 ? (int) (cur >> ybits) : 0;
      const int yy = cy + (r % 3) - 1, zz = DIM == 3 ? cz + (r / 3) - 1 : 0;
      int pos = 0;
      if (yy >= 0 && yy <= S.cmax[1] && zz >= 0 && zz <= S.cmax[2]) {
        const int xx = (lane & 1) ? min(cx_hi + 1, S.cmax[0]) : max(cx_lo - 1, 0);
        unsigned long long target = (unsigned long long) xx | ((unsigned long long) yy << S.shift[1]);
        if (DIM == 3) target |= (unsigned long long) zz << S.shift[2];
        pos = lower_bound_key(skeys, nf, target, (lane & 1) != 0);
      }
      rng[lane] = pos;
    }
    __syncthreads();
    for (int r = 0; r < NROWS; ++r) {
      const int lo = rng[2 * r], hi = rng[2 * r + 1];
      for (int base = lo; base < hi; base += SRRG2_NRM_TILE) {
        __syncthreads();  // (the tile before has been read)
        if (base + lane < hi) tile[lane] = sorted[base + lane];  // (base + lane < hi <= nf <= n)
        __syncthreads();
        const int m = min(SRRG2_NRM_TILE, hi - base);
        if (mine) {
          for (int j = 0; j < m; ++j) {
            const float4 c = tile[j];
            const float dx = c.x - me.x, dy = c.y - me.y, dz = DIM == 3 ? c.z - me.z : 0.f;
            const float d2 = DIM == 3 ? (dx * dx + dy * dy) + dz * dz : dx * dx + dy * dy;
            if (d2 <= A.r2) {
              const double x = (double) dx, y = (double) dy;
              const double xs = x * A.scale2, ys = y * A.scale2;
              ++cnt;
              sx += (unsigned long long) __double_as_longlong(fma(x, A.scale1, MAGIC));
              sy += (unsigned long long) __double_as_longlong(fma(y, A.scale1, MAGIC));
              sxx += (unsigned long long) __double_as_longlong(fma(x, xs, MAGIC));
              sxy += (unsigned long long) __double_as_longlong(fma(x, ys, MAGIC));
              syy += (unsigned long long) __double_as_longlong(fma(y, ys, MAGIC));
              if (DIM == 3) {
                const double z  = (double) dz;
                const double zs = z * A.scale2;
                sz += (unsigned long long) __double_as_longlong(fma(z, A.scale1, MAGIC));
                sxz += (unsigned long long) __double_as_longlong(fma(x, zs, MAGIC));
                syz += (unsigned long long) __double_as_longlong(fma(y, zs, MAGIC));
                szz += (unsigned long long) __double_as_longlong(fma(z, zs, MAGIC));
              }
            }
          }
        }
      }
    }
  }

  // ---- per query: covariance, Jacobi, selection, orientation -------------------------------------------------------------------
  int cls = 1;  // 0 normal, 1 not finite, 2 too few, 3 degenerate, 4 too curved
  float nx = fnan, ny = fnan, nz = DIM == 3 ? fnan : 0.f, curv = fnan;
  if (active) {
    cls = 2;
    if (cnt >= A.min_neighbours) {
      const unsigned long long off = (unsigned long long) cnt * (unsigned long long) __double_as_longlong(MAGIC);
      const double k   = (double) cnt;
      const double mx_ = ((double) (long long) (sx - off) * A.inv1) / k;
      const double my_ = ((double) (long long) (sy - off) * A.inv1) / k;
      const double mz_ = DIM == 3 ? ((double) (long long) (sz - off) * A.inv1) / k : 0.0;
      double a00 = ((double) (long long) (sxx - off) * A.inv2) / k - mx_ * mx_;
      double a01 = ((double) (long long) (sxy - off) * A.inv2) / k - mx_ * my_;
      double a11 = ((double) (long long) (syy - off) * A.inv2) / k - my_ * my_;
      double a02 = 0.0, a12 = 0.0, a22 = 0.0;
      if (DIM == 3) {
        a02 = ((double) (long long) (sxz - off) * A.inv2) / k - mx_ * mz_;
        a12 = ((double) (long long) (syz - off) * A.inv2) / k - my_ * mz_;
        a22 = ((double) (long long) (szz - off) * A.inv2) / k - mz_ * mz_;
      }
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
      if (DIM == 3) {
        for (int sweep = 0; sweep < SRRG2_NRM_SWEEPS; ++sweep) {
          jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
          jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
          jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
      } else {
        jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (one rotation diagonalises a 2x2)
      }
      // (the columns leave through an empty asm as fresh values: read straight from the variables the rotations update by
      // reference, the compiler answers the selection below with an indexed load from a copy of the matrix in scratch)
      double c00, c10, c20, c01, c11, c21, c02, c12, c22;
      asm volatile("" : "=v"(c00), "=v"(c10), "=v"(c20) : "0"(v00), "1"(v10), "2"(v20));
      asm volatile("" : "=v"(c01), "=v"(c11), "=v"(c21) : "0"(v01), "1"(v11), "2"(v21));
      asm volatile("" : "=v"(c02), "=v"(c12), "=v"(c22) : "0"(v02), "1"(v12), "2"(v22));
      double l0 = a00, e0 = c00, e1 = c10, e2 = c20;
      if (a11 < l0) l0 = a11, e0 = c01, e1 = c11, e2 = c21;
      if (DIM == 3 && a22 < l0) l0 = a22, e0 = c02, e1 = c12, e2 = c22;
      const double trace = DIM == 3 ? (a00 + a11) + a22 : a00 + a11;
      cls = 3;
      if (trace > 0.0 && isfinite(trace)) {
        curv = (float) (l0 / trace);
        cls  = 4;
        if (!(curv > A.max_curvature)) {
          cls              = 0;
          const double len = sqrt(DIM == 3 ? (e0 * e0 + e1 * e1) + e2 * e2 : e0 * e0 + e1 * e1);
          e0 = e0 / len, e1 = e1 / len;
          if (DIM == 3) e2 = e2 / len;
          bool flip;
          if (A.has_viewpoint) {
            const double dot = DIM == 3 ? (e0 * (A.vp[0] - (double) me.x) + e1 * (A.vp[1] - (double) me.y)) + e2 * (A.vp[2] - (double) me.z)
                                        : e0 * (A.vp[0] - (double) me.x) + e1 * (A.vp[1] - (double) me.y);
            flip = dot < 0.0;
          } else {
            double big = e0;
            if (fabs(e1) > fabs(big)) big = e1;
            if (DIM == 3 && fabs(e2) > fabs(big)) big = e2;
            flip = big < 0.0;
          }
          if (flip) e0 = -e0, e1 = -e1, e2 = -e2;
          nx = (float) e0, ny = (float) e1, nz = DIM == 3 ? (float) e2 : 0.f;
        }
      }
    }
  }
  if (s < n) {
    const int i = __float_as_int(me.w);  // (a permutation of [0, n): the sort's payload)
    out_nrm[i]  = make_float4(nx, ny, nz, 0.f);
    out_curv[i] = curv;
  }
  for (int c = 0; c < 5; ++c) {
    if (c == 1) continue;
    const int k = __popcll(__ballot(s < n && cls == c));
    if (lane == 0 && k) atomicAdd(&ctr[c == 0 ? C_NORMAL : c], k);  // (C_FEW = 2, C_DEGEN = 3, C_CURVED = 4)
  }
}

__global__ __launch_bounds__(256) void k_nrm_flag(const NrmSpec* __restrict__ spec, const float4* __restrict__ nrm, int n,
                                                  int* __restrict__ flags) {
  const bool off = spec->unsupported != 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) flags[i] = (!off && nrm[i].x == nrm[i].x) ? 1 : 0;
}

template <bool FEAT>
__global__ __launch_bounds__(256) void k_nrm_scatter(const NrmSpec* __restrict__ spec, const float4* __restrict__ pts,
                                                     const float4* __restrict__ nrm, int n, const int* __restrict__ offset,
                                                     float4* __restrict__ out_pts, float4* __restrict__ out_nrm,
                                                     int* __restrict__ gidx, Feat f) {
  if (spec->unsupported) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 q = nrm[i];
    if (!(q.x == q.x)) continue;
    const int k = offset[i];
    if (k < 0 || k >= n) continue;  // (cannot happen: an exclusive scan of n flags)
    out_pts[k] = pts[i];
    out_nrm[k] = q;
    gidx[k]    = i;
    if (FEAT) move_features(f, i, k);
  }
}

int ceil_log2(int n) {
  int l = 0;
  while (l < 31 && (1ll << l) < (long long) n) ++l;
  return l;
}

}  // namespace

// the two exponents of the fixed-point moments: radius < 2^E, n <= 2^L;
// e1 = min(61 - L - E, 50 - E), e2 = min(61 - L - 2E, 50 - 2E)
extern "C" void srrg2_normals_exponents(float radius, int n, int* e1, int* e2) {
  int E = 0;
  (void) std::frexp(radius, &E);
  const int L = ceil_log2(n);
  if (e1) *e1 = std::min(61 - L - E, 50 - E);
  if (e2) *e2 = std::min(61 - L - 2 * E, 50 - 2 * E);
}

extern "C" void srrg2_normals_default_params(srrg2_normals_params* p, int dim) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius                     = 0.1f;
  p->min_neighbours             = dim == 2 ? 3 : 5;
  p->max_curvature              = 1.f;
  p->drop_points_without_normal = 1;
}

extern "C" int srrg2_scene_estimate_normals(srrg2_scene_h s, const srrg2_normals_params* p, float* curvature_out,
                                            srrg2_normals_result* out) {
  if (!s || !p) return fail(SRRG2_E_INVALID, "scene_estimate_normals: null scene or params");
  if (!std::isfinite(p->radius) || !(p->radius > 0.f)) return fail(SRRG2_E_INVALID, "scene_estimate_normals: radius must be finite and > 0");
  // (membership compares against the float32 square: it has to be a number a distance can exceed or fall short of.  With an
  // infinite square every point of the neighbouring cells would be a member and a term could leave the range the exponents assume)
  if (!std::isfinite(p->radius * p->radius) || !(p->radius * p->radius > 0.f))
    return fail(SRRG2_E_INVALID, "scene_estimate_normals: radius*radius must be finite and > 0 in float32 (about 1e-22 .. 1.8e19)");
  if (p->min_neighbours < s->dim + 1) return fail(SRRG2_E_INVALID, "scene_estimate_normals: min_neighbours >= dim + 1 (the point itself counts)");
  if (std::isnan(p->max_curvature)) return fail(SRRG2_E_INVALID, "scene_estimate_normals: max_curvature is NaN");
  if (p->drop_points_without_normal != 0 && p->drop_points_without_normal != 1)
    return fail(SRRG2_E_INVALID, "scene_estimate_normals: drop_points_without_normal must be 0 or 1");
  HIP_TRY(hipSetDevice(s->device));
  if (s->pending) {  // an adaptor's queued write
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->pending = false;
  }
  int rc;
  const int n     = s->n;
  const int dim   = s->dim;
  const bool drop = p->drop_points_without_normal == 1;
  if (out) std::memset(out, 0, sizeof(*out));
  if (n == 0) {
    if ((rc = srrg2amd::scene_make_room(s, 1, 0))) return rc;
    s->has_normals = true;
    return 0;
  }
  NrmArgs A;
  std::memset(&A, 0, sizeof(A));
  int e1 = 0, e2 = 0;
  srrg2_normals_exponents(p->radius, n, &e1, &e2);
  A.r2     = p->radius * p->radius;
  A.scale1 = std::ldexp(1.0, e1), A.inv1 = std::ldexp(1.0, -e1);
  A.scale2 = std::ldexp(1.0, e2), A.inv2 = std::ldexp(1.0, -e2);
  A.min_neighbours = p->min_neighbours;
  A.max_curvature  = p->max_curvature;
  A.has_viewpoint  = 1;
  for (int d = 0; d < 3; ++d) {
    A.vp[d] = d < dim ? (double) p->viewpoint[d] : 0.0;
    if (std::isnan(p->viewpoint[d])) A.has_viewpoint = 0;  // (any of the three, also for dim 2)
  }
  const bool queued    = !drop && !out && !curvature_out;  // nothing the host has to know: no wait at all
  A.nan_if_unsupported = queued ? 1 : 0;

  // The arrays the call writes are sized by n, not by the live capacity: reserve() adds its slack once, and after the swap the
  // scene's former arrays -- which held n points -- are the spares of the next call.  A handle reused frame after frame reaches
  // a fixed point after two calls: no allocation, no growth.
  const size_t room = (size_t) n;
  if ((rc = s->alt_nrm.reserve(room))) return rc;
  if ((rc = s->nrm_sorted.reserve((size_t) n)) || (rc = s->nrm_curv.reserve((size_t) n))) return rc;
  if ((rc = s->nrm_keys.reserve(2 * (size_t) n)) || (rc = s->nrm_idx.reserve(2 * (size_t) n))) return rc;
  if ((rc = s->nrm_ctr.reserve(C_WORDS + (sizeof(NrmSpec) + 3) / 4 + 2))) return rc;
  if (drop) {
    if ((rc = s->alt_pts.reserve(room)) || (rc = s->nrm_tmp.reserve((size_t) n)) || (rc = s->alt_gidx.reserve((size_t) n))) return rc;
    if (s->has_desc && (rc = s->alt_desc.reserve(2 * s->alt_pts.cap))) return rc;
    if (s->has_inten && (rc = s->alt_inten.reserve(s->alt_pts.cap))) return rc;
    if ((rc = s->flags.reserve((size_t) n + 1))) return rc;
    if ((rc = s->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(n) + 2))) return rc;
  }
  hipStream_t st = s->stream;
  int* const ctr = s->nrm_ctr.p;
  NrmSpec* const spec = reinterpret_cast<NrmSpec*>(ctr + C_WORDS);  // (64 bytes in: aligned for its doubles)
  unsigned long long* const keys = s->nrm_keys.p;
  unsigned long long* const skeys = keys + n;
  int* const idx  = s->nrm_idx.p;
  int* const sidx = idx + n;
  float4* const computed = drop ? s->nrm_tmp.p : s->alt_nrm.p;

  HIP_TRY(hipMemsetAsync(ctr, 0, C_WORDS * sizeof(int), st));
  const dim3 grid(blocks_for(n)), block(256);
  GridAnchor anchor;  // cells from the box minimum
  std::memset(&anchor, 0, sizeof(anchor));
  anchor.h = (double) p->radius * (1.0 + 0x1p-16);
  if (dim == 3)
    hipLaunchKernelGGL(k_grid_bbox<3>, dim3(std::min<int>(grid.x, 64)), block, 0, st, s->pts.p, n, ctr);
  else
    hipLaunchKernelGGL(k_grid_bbox<2>, dim3(std::min<int>(grid.x, 64)), block, 0, st, s->pts.p, n, ctr);
  hipLaunchKernelGGL(k_grid_spec, dim3(1), dim3(64), 0, st, dim, anchor, ctr, spec);
  if (dim == 3)
    hipLaunchKernelGGL(k_grid_keys<3>, grid, block, 0, st, spec, s->pts.p, n, keys, idx);
  else
    hipLaunchKernelGGL(k_grid_keys<2>, grid, block, 0, st, spec, s->pts.p, n, keys, idx);
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, skeys, idx, sidx, n, 0, 64, st));
  if ((rc = s->sort_tmp.reserve(std::max<size_t>(tmp_bytes, 1)))) return rc;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(s->sort_tmp.p, tmp_bytes, keys, skeys, idx, sidx, n, 0, 64, st));
  hipLaunchKernelGGL(k_nrm_gather, grid, block, 0, st, spec, s->pts.p, sidx, n, s->nrm_sorted.p);
  const dim3 ngrid((n + 63) / 64);
  if (dim == 3)
    hipLaunchKernelGGL(k_nrm_neigh<3>, ngrid, dim3(64), 0, st, spec, skeys, s->nrm_sorted.p, n, A, computed, s->nrm_curv.p, ctr);
  else
    hipLaunchKernelGGL(k_nrm_neigh<2>, ngrid, dim3(64), 0, st, spec, skeys, s->nrm_sorted.p, n, A, computed, s->nrm_curv.p, ctr);
  HIP_TRY(hipGetLastError());
  if (queued) {  // (an extent beyond the key range cannot be reported from here: the kernel has written NaN normals instead)
    std::swap(s->nrm, s->alt_nrm);
    s->has_normals = true;
    s->pending     = true;
    return 0;
  }
  if (drop) {
    // the compaction goes behind the pass before the host knows how many survive: one wait per call
    hipLaunchKernelGGL(k_nrm_flag, grid, block, 0, st, spec, computed, n, s->flags.p);
    srrg2amd::launch_exclusive_scan(s->flags.p, n, s->scan_sums.p, ctr + C_TOTAL, st);
    const Feat f{s->has_desc ? s->desc.p : nullptr, s->has_inten ? s->inten.p : nullptr,
                 s->has_desc ? s->alt_desc.p : nullptr, s->has_inten ? s->alt_inten.p : nullptr};
    if (f.dst_desc || f.dst_inten)
      hipLaunchKernelGGL(k_nrm_scatter<true>, grid, block, 0, st, spec, s->pts.p, computed, n, s->flags.p, s->alt_pts.p,
                         s->alt_nrm.p, s->alt_gidx.p, f);
    else
      hipLaunchKernelGGL(k_nrm_scatter<false>, grid, block, 0, st, spec, s->pts.p, computed, n, s->flags.p, s->alt_pts.p,
                         s->alt_nrm.p, s->alt_gidx.p, f);
  }
  HIP_TRY(hipMemcpyAsync(s->scalars.p, ctr, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (curvature_out) HIP_TRY(hipMemcpyAsync(curvature_out, s->nrm_curv.p, sizeof(float) * (size_t) n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  if (s->scalars.p[C_UNSUP])
    return fail(SRRG2_E_UNSUPPORTED,
                "scene_estimate_normals: the cloud spans more cells of one radius than the 63-bit cell key holds (2^30 per axis, "
                "63 bits over the axes)");
  std::swap(s->nrm, s->alt_nrm);
  s->has_normals = true;
  if (drop) {
    const int total = s->scalars.p[C_TOTAL];
    if (total < 0 || total > n) return fail(SRRG2_E_HIP, "scene_estimate_normals: the compaction scan returned a total out of range");
    std::swap(s->pts, s->alt_pts);
    if (s->has_desc) std::swap(s->desc, s->alt_desc);
    if (s->has_inten) std::swap(s->inten, s->alt_inten);
    std::swap(s->gidx, s->alt_gidx);
    s->n = s->ng = total;
  }
  if (out) {
    out->num_points      = n;
    out->num_finite      = s->scalars.p[C_FINITE];
    out->num_with_normal = s->scalars.p[C_NORMAL];
    out->num_too_few     = s->scalars.p[C_FEW];
    out->num_degenerate  = s->scalars.p[C_DEGEN];
    out->num_too_curved  = s->scalars.p[C_CURVED];
    out->scene_size      = s->n;
  }
  return 0;
}
