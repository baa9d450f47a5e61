// voxel.hip -- srrg2_scene_voxelize: one point per occupied cell of a grid of leaf_size cubes, for scenes whose density has to be
// bounded before anything else looks at them (a lidar sweep, a map grown by merges).  No reference counterpart; DESIGN.md
// section 4 "Voxel-grid decimation" is the contract and tests/voxel_restatement.py its executable form: the result is a
// function of the points and the parameters alone, bit for bit.
//   k_grid_bbox / k_grid_spec / k_grid_keys   (cell_grid.h, shared with normals.hip) box, key layout, a cell key per point
//   (stable radix sort of (key, index) pairs: hipcub -- inside a cell the indices ascend, the head of a run is the representative)
//   k_vox_heads     head flag per sorted entry; their exclusive scan gives every entry its cell's rank
//   k_vox_reduce    THE pass: one wave per 64 consecutive sorted entries -- gather, quantise, segmented sum across the lanes
//   k_vox_finish    one thread per cell: mean, normal, the min_points gate; keep flag and result at the representative's index
//   (exclusive scan of the keep flags in scene order + k_vox_scatter: the clippers' tail, srrg2amd::scene_compact_into)
// All sums are 64-bit integers: whichever way a cell's points are split over waves, the sum is the same.
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

// counters block (ints): the grid's words (cell_grid.h: [0] finite points, [5] beyond the key range, [8, 14) the box) and, in
// between, [1] occupied cells (the scan's total), [2] emitted cells with a normal, [3] the most points in one cell
enum { V_FINITE = GRID_FINITE, V_OCCUPIED = 1, V_WITH_NORMAL = 2, V_MAX_POINTS = 3, V_UNSUP = GRID_UNSUP, V_WORDS = GRID_WORDS };
// words of a cell's accumulator (int64): the sums of the quantised offsets and normal components, the two counts
enum { A_PX = 0, A_NX = 3, A_COUNT = 6, A_NCOUNT = 7, A_WORDS = 8 };

struct VoxArgs {
  double org[3], leaf;
  double scale, inv;  // 2^e, 2^-e: offsets from the cell's corner
  double nscale;      // 2^en: normal components
  int min_points;
};

__global__ __launch_bounds__(256) void k_vox_heads(const GridSpec* __restrict__ spec, const unsigned long long* __restrict__ skeys,
                                                   int n, int* __restrict__ heads) {
  const bool off = spec->unsupported != 0;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    int h = 0;
    if (!off) {
      const unsigned long long k = skeys[s];
      h = (k != ~0ull && (s == 0 || skeys[s - 1] != k)) ? 1 : 0;
    }
    heads[s] = h;
  }
}

__device__ __forceinline__ long long vox_quantise(double v, double scale) { return (long long) rint(v * scale); }

// The reduction.  A workgroup is ONE wave and owns 64 consecutive entries of the cell-sorted order; rank_ex is the exclusive scan
// of the head flags (n + 1 words, the total behind them): entry s belongs to cell rank_ex[s + 1] - 1 and heads its run iff
// rank_ex[s + 1] != rank_ex[s].  Every lane gathers its point (and normal) by index and quantises; a segmented inclusive sum
// across the lanes leaves each run's total in its last lane.  A run that lies wholly inside the wave is written with plain
// stores; only the at most two runs that cross the wave's edges add into the zero-initialised accumulators with 64-bit integer
// atomics -- a cell is written either by one lane or by atomics alone, never both.  A cell that holds every point of the scene
// is summed by n / 64 waves.
// SUMS: centroid mode (FIRST needs the count only); NRM: centroid mode and the scene has normals.
template <int DIM, bool SUMS, bool NRM>
__global__ __launch_bounds__(64) void k_vox_reduce(const GridSpec* __restrict__ spec, const float4* __restrict__ pts,
                                                   const float4* __restrict__ nrm, const int* __restrict__ sidx,
                                                   const int* __restrict__ rank_ex, VoxArgs A, long long* __restrict__ acc,
                                                   int* __restrict__ rep) {
  if (spec->unsupported) return;
  const int nf   = spec->nfinite;  // (the finite points sort in front: entries [0, nf))
  const int lane = threadIdx.x;
  const int s    = blockIdx.x * 64 + lane;
  if (blockIdx.x * 64 >= nf) return;  // (the whole wave)
  const bool active = s < nf;
  int rank = -1;
  bool head = false;
  long long v0 = 0, v1 = 0, v2 = 0, w0 = 0, w1 = 0, w2 = 0;
  int cnt = 0, ncnt = 0;
  if (active) {
    const int ex0 = rank_ex[s], ex1 = rank_ex[s + 1];
    rank = ex1 - 1;
    head = ex1 != ex0;
    cnt  = 1;
    const int i = sidx[s];  // (a permutation of [0, n): the sort's payload)
    if (head) rep[rank] = i;
    if (SUMS) {
      const float4 p = pts[i];
      const double x = (double) p.x, y = (double) p.y;
      v0 = vox_quantise(x - (A.org[0] + grid_cell_abs(x, A.org[0], A.leaf) * A.leaf), A.scale);
      v1 = vox_quantise(y - (A.org[1] + grid_cell_abs(y, A.org[1], A.leaf) * A.leaf), A.scale);
      if (DIM == 3) {
        const double z = (double) p.z;
        v2 = vox_quantise(z - (A.org[2] + grid_cell_abs(z, A.org[2], A.leaf) * A.leaf), A.scale);
      }
    }
    if (NRM) {
      const float4 q = nrm[i];
      const bool ok = fabsf(q.x) < 2.f && fabsf(q.y) < 2.f && (DIM == 2 || fabsf(q.z) < 2.f);  // (false for NaN and inf)
      if (ok) {
        ncnt = 1;
        w0 = vox_quantise((double) q.x, A.nscale);
        w1 = vox_quantise((double) q.y, A.nscale);
        if (DIM == 3) w2 = vox_quantise((double) q.z, A.nscale);
      }
    }
  }
  // segmented inclusive sum: the entries are sorted, so an equal rank `off` lanes down means one run all the way
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int below = __shfl_up(rank, off);  // (by every lane, outside the condition: a shuffle reads nothing from a masked lane)
    const bool take = lane >= off && below == rank;
    const int c = __shfl_up(cnt, off);
    if (take) cnt += c;
    if (SUMS) {
      const long long t0 = __shfl_up(v0, off), t1 = __shfl_up(v1, off);
      if (take) v0 += t0, v1 += t1;
      if (DIM == 3) {
        const long long t2 = __shfl_up(v2, off);
        if (take) v2 += t2;
      }
    }
    if (NRM) {
      const int m = __shfl_up(ncnt, off);
      const long long t0 = __shfl_up(w0, off), t1 = __shfl_up(w1, off);
      if (take) ncnt += m, w0 += t0, w1 += t1;
      if (DIM == 3) {
        const long long t2 = __shfl_up(w2, off);
        if (take) w2 += t2;
      }
    }
  }
  const int next_rank = __shfl_down(rank, 1);
  const int rank0     = __shfl(rank, 0);
  const int head0     = __shfl(head ? 1 : 0, 0);
  if (!active || (lane < 63 && next_rank == rank)) return;  // not the last lane of its run in this wave
  const bool starts_here = rank != rank0 || head0 != 0;
  const bool ends_here   = lane < 63 || s + 1 >= nf || rank_ex[s + 2] != rank_ex[s + 1];  // (s + 2 <= nf <= n)
  long long* const a     = acc + (size_t) rank * A_WORDS;                                  // (rank < occupied cells <= nf <= n)
  if (starts_here && ends_here) {
    a[A_COUNT] = cnt;
    if (SUMS) {
      a[A_PX] = v0, a[A_PX + 1] = v1;
      if (DIM == 3) a[A_PX + 2] = v2;
    }
    if (NRM) {
      a[A_NCOUNT] = ncnt;
      a[A_NX] = w0, a[A_NX + 1] = w1;
      if (DIM == 3) a[A_NX + 2] = w2;
    }
  } else {
    unsigned long long* const u = reinterpret_cast<unsigned long long*>(a);
    atomicAdd(&u[A_COUNT], (unsigned long long) cnt);
    if (SUMS) {
      atomicAdd(&u[A_PX], (unsigned long long) v0);
      atomicAdd(&u[A_PX + 1], (unsigned long long) v1);
      if (DIM == 3) atomicAdd(&u[A_PX + 2], (unsigned long long) v2);
    }
    if (NRM) {
      atomicAdd(&u[A_NCOUNT], (unsigned long long) ncnt);
      atomicAdd(&u[A_NX], (unsigned long long) w0);
      atomicAdd(&u[A_NX + 1], (unsigned long long) w1);
      if (DIM == 3) atomicAdd(&u[A_NX + 2], (unsigned long long) w2);
    }
  }
}

// one thread per occupied cell: what the cell emits, at its representative's index, and the keep flag of the scan in scene order
// HAS_NRM: the scene has normals (FIRST copies the representative's; without them the output normals are zero, as a clipper's)
template <int DIM, bool SUMS, bool HAS_NRM>
__global__ __launch_bounds__(256) void k_vox_finish(const GridSpec* __restrict__ spec, const float4* __restrict__ pts,
                                                    const float4* __restrict__ nrm, const int* __restrict__ rank_ex, int n, VoxArgs A,
                                                    const long long* __restrict__ acc, const int* __restrict__ rep,
                                                    float4* __restrict__ out_pts, float4* __restrict__ out_nrm,
                                                    int* __restrict__ out_cnt, int* __restrict__ flags, int* __restrict__ ctr) {
  if (spec->unsupported) return;
  const int nocc   = rank_ex[n];  // (the scan's total: <= n)
  const float fnan = __uint_as_float(0x7fc00000u);
  int most = 0, with_normal = 0;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nocc; r += gridDim.x * blockDim.x) {
    const long long* const a = acc + (size_t) r * A_WORDS;
    const int i        = rep[r];
    const long long k  = a[A_COUNT];
    const bool emitted = k >= (long long) A.min_points;
    const float4 p     = pts[i];
    float4 o           = make_float4(p.x, p.y, DIM == 3 ? p.z : 0.f, 0.f);
    if (SUMS && k > 1) {
      const double kd = (double) k;
      const double x = (double) p.x, y = (double) p.y;
      o.x = (float) ((A.org[0] + grid_cell_abs(x, A.org[0], A.leaf) * A.leaf) + ((double) a[A_PX] * A.inv) / kd);
      o.y = (float) ((A.org[1] + grid_cell_abs(y, A.org[1], A.leaf) * A.leaf) + ((double) a[A_PX + 1] * A.inv) / kd);
      if (DIM == 3) {
        const double z = (double) p.z;
        o.z = (float) ((A.org[2] + grid_cell_abs(z, A.org[2], A.leaf) * A.leaf) + ((double) a[A_PX + 2] * A.inv) / kd);
      }
    }
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HAS_NRM) {
      if (SUMS) {
        const double x = (double) a[A_NX], y = (double) a[A_NX + 1], z = DIM == 3 ? (double) a[A_NX + 2] : 0.0;
        const double len = sqrt(DIM == 3 ? (x * x + y * y) + z * z : x * x + y * y);
        if (a[A_NCOUNT] > 0 && len > 0.0)
          q = make_float4((float) (x / len), (float) (y / len), DIM == 3 ? (float) (z / len) : 0.f, 0.f);
        else
          q = make_float4(fnan, fnan, DIM == 3 ? fnan : 0.f, 0.f);
      } else {
        const float4 m = nrm[i];
        q = make_float4(m.x, m.y, DIM == 3 ? m.z : 0.f, 0.f);
      }
      if (emitted && q.x == q.x && q.y == q.y && q.z == q.z) ++with_normal;
    }
    out_pts[i] = o;
    out_nrm[i] = q;
    out_cnt[i] = (int) k;
    flags[i]   = emitted ? 1 : 0;
    most       = max(most, (int) k);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    most = max(most, __shfl_xor(most, off));
    with_normal += __shfl_xor(with_normal, off);
  }
  if ((threadIdx.x & 63) == 0) {  // one atomic per wave and word
    if (most) atomicMax(&ctr[V_MAX_POINTS], most);
    if (with_normal) atomicAdd(&ctr[V_WITH_NORMAL], with_normal);
  }
}

// the scatter behind the scan in scene order: a kept index i is a representative, its cell's result lies at i.  The counts go
// to a buffer of the source's size, whatever room `dst` has (k < total <= n); the k >= cap guard is the clippers'.
template <bool FEAT>
__global__ void k_vox_scatter(int n, const int* __restrict__ offset, const float4* __restrict__ vpts, const float4* __restrict__ vnrm,
                              const int* __restrict__ vcnt, float4* __restrict__ out_pts, float4* __restrict__ out_nrm,
                              int* __restrict__ gidx, int* __restrict__ counts, int cap, Feat f) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int k = offset[i];
    if (offset[i + 1] == k) continue;
    counts[k] = vcnt[i];
    if (k >= cap) continue;  // (no room yet: scene_compact_into repeats the scatter with room for all)
    out_pts[k] = vpts[i];
    out_nrm[k] = vnrm[i];
    gidx[k]    = i;
    if (FEAT) move_features(f, i, k);
  }
}

template <int DIM>
void launch_reduce_finish(srrg2_scene* src, bool sums, int n, const GridSpec* spec, const int* sidx, const VoxArgs& A, int* ctr) {
  hipStream_t st      = src->stream;
  const bool has_nrm  = src->has_normals;
  const float4* nrm   = has_nrm ? src->nrm.p : nullptr;
  const dim3 rgrid((n + 63) / 64), fgrid(blocks_for(n));
#define VOX_LAUNCH(S, N)                                                                                                             \
  do {                                                                                                                               \
    hipLaunchKernelGGL((k_vox_reduce<DIM, S, S && N>), rgrid, dim3(64), 0, st, spec, src->pts.p, nrm, sidx, src->vox_rank.p, A,      \
                       src->vox_acc.p, src->vox_rep.p);                                                                              \
    hipLaunchKernelGGL((k_vox_finish<DIM, S, N>), fgrid, dim3(256), 0, st, spec, src->pts.p, nrm, src->vox_rank.p, n, A,             \
                       src->vox_acc.p, src->vox_rep.p, src->vox_pts.p, src->vox_nrm.p, src->vox_cnt.p, src->flags.p, ctr);           \
  } while (0)
  if (sums && has_nrm)
    VOX_LAUNCH(true, true);
  else if (sums)
    VOX_LAUNCH(true, false);
  else if (has_nrm)
    VOX_LAUNCH(false, true);
  else
    VOX_LAUNCH(false, false);
#undef VOX_LAUNCH
}

}  // namespace

extern "C" void srrg2_voxel_default_params(srrg2_voxel_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->leaf_size            = 0.05f;
  p->mode                 = SRRG2_VOXEL_CENTROID;
  p->min_points_per_voxel = 1;
}

extern "C" int srrg2_scene_voxelize(srrg2_scene_h src, const srrg2_voxel_params* p, srrg2_scene_h dst, int32_t* counts_out,
                                    srrg2_voxel_result* out) {
  if (!src || !dst || !p) return fail(SRRG2_E_INVALID, "scene_voxelize: null scene or params");
  if (!srrg2amd::scene_clip_pair(src, dst))
    return fail(SRRG2_E_INVALID, "scene_voxelize: src and dst must be two scenes of one dim on one device");
  if (!std::isfinite(p->leaf_size) || !(p->leaf_size > 0.f)) return fail(SRRG2_E_INVALID, "scene_voxelize: leaf_size must be finite and > 0");
  if (!std::isfinite(p->origin[0]) || !std::isfinite(p->origin[1]) || !std::isfinite(p->origin[2]))
    return fail(SRRG2_E_INVALID, "scene_voxelize: origin must be finite");
  if (p->mode != SRRG2_VOXEL_CENTROID && p->mode != SRRG2_VOXEL_FIRST) return fail(SRRG2_E_INVALID, "scene_voxelize: mode outside srrg2_voxel_mode");
  if (p->min_points_per_voxel < 1) return fail(SRRG2_E_INVALID, "scene_voxelize: min_points_per_voxel >= 1");
  if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(SRRG2_E_INVALID, "scene_voxelize: reserved must be 0");
  // what a refusal that is known only after the wait puts back
  const int dst_n = dst->n, dst_ng = dst->ng;
  const bool dst_normals = dst->has_normals, dst_desc = dst->has_desc, dst_inten = dst->has_inten;
  int rc;
  if ((rc = srrg2amd::scene_clip_begin(src, dst))) return rc;
  // (arrays even for an empty result, as the clippers leave them; with room for one point the scatter below always runs once
  // before the wait and the counts travel with it)
  if ((rc = srrg2amd::scene_make_room(dst, 1, 0)) || (rc = dst->gidx.reserve(1))) return rc;
  const int n   = src->n;
  const int dim = src->dim;
  if (out) std::memset(out, 0, sizeof(*out));
  if (n == 0) return 0;

  VoxArgs A;
  std::memset(&A, 0, sizeof(A));
  int e = 0, en = 0;
  srrg2_normals_exponents(p->leaf_size, n, &e, nullptr);
  srrg2_normals_exponents(1.f, n, &en, nullptr);
  A.leaf  = (double) p->leaf_size;
  A.scale = std::ldexp(1.0, e), A.inv = std::ldexp(1.0, -e);
  A.nscale     = std::ldexp(1.0, en);
  A.min_points = p->min_points_per_voxel;
  GridAnchor anchor;
  std::memset(&anchor, 0, sizeof(anchor));
  anchor.h = A.leaf, anchor.anchored = 1;
  for (int d = 0; d < dim; ++d) A.org[d] = anchor.origin[d] = (double) p->origin[d];

  srrg2_scene* const s = src;  // the scratch is the source's
  if ((rc = s->nrm_keys.reserve(2 * (size_t) n)) || (rc = s->nrm_idx.reserve(2 * (size_t) n))) return rc;
  if ((rc = s->nrm_ctr.reserve(V_WORDS + (sizeof(GridSpec) + 3) / 4 + 2))) return rc;
  if ((rc = s->vox_rank.reserve((size_t) n + 1)) || (rc = s->flags.reserve((size_t) n + 1))) return rc;
  if ((rc = s->scan_sums.reserve((size_t) srrg2amd::scan_num_blocks(n) + 2))) return rc;
  if ((rc = s->vox_acc.reserve((size_t) n * A_WORDS)) || (rc = s->vox_rep.reserve((size_t) n))) return rc;
  if ((rc = s->vox_pts.reserve((size_t) n)) || (rc = s->vox_nrm.reserve((size_t) n))) return rc;
  if ((rc = s->vox_cnt.reserve((size_t) n)) || (rc = s->vox_counts.reserve((size_t) n))) return rc;
  hipStream_t st = s->stream;
  int* const ctr = s->nrm_ctr.p;
  GridSpec* const spec = reinterpret_cast<GridSpec*>(ctr + V_WORDS);  // (64 bytes in: aligned for its doubles)
  unsigned long long* const keys  = s->nrm_keys.p;
  unsigned long long* const skeys = keys + n;
  int* const idx  = s->nrm_idx.p;
  int* const sidx = idx + n;

  HIP_TRY(hipMemsetAsync(ctr, 0, V_WORDS * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(s->vox_acc.p, 0, sizeof(long long) * A_WORDS * (size_t) n, st));
  HIP_TRY(hipMemsetAsync(s->flags.p, 0, sizeof(int) * ((size_t) n + 1), st));
  if (counts_out) HIP_TRY(hipMemsetAsync(s->vox_counts.p, 0, sizeof(int) * (size_t) n, st));
  const dim3 grid(blocks_for(n)), block(256);
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
  hipLaunchKernelGGL(k_vox_heads, grid, block, 0, st, spec, skeys, n, s->vox_rank.p);
  srrg2amd::launch_exclusive_scan(s->vox_rank.p, n, s->scan_sums.p, ctr + V_OCCUPIED, st);
  const bool sums = p->mode == SRRG2_VOXEL_CENTROID;
  if (dim == 3)
    launch_reduce_finish<3>(s, sums, n, spec, sidx, A, ctr);
  else
    launch_reduce_finish<2>(s, sums, n, spec, sidx, A, ctr);
  HIP_TRY(hipGetLastError());

  // the clippers' tail: scan of the keep flags in scene order, one scatter, one wait -- which carries the counters and the counts
  const Feat f{dst->has_desc ? s->desc.p : nullptr, dst->has_inten ? s->inten.p : nullptr, nullptr, nullptr};
  const auto scatter = [&](int cap) {
    Feat g      = f;  // (dst's feature arrays exist from scene_compact_into on, and may move when it makes room)
    g.dst_desc  = dst->has_desc ? dst->desc.p : nullptr;
    g.dst_inten = dst->has_inten ? dst->inten.p : nullptr;
    if (g.dst_desc || g.dst_inten)
      hipLaunchKernelGGL(k_vox_scatter<true>, grid, block, 0, st, n, s->flags.p, s->vox_pts.p, s->vox_nrm.p, s->vox_cnt.p, dst->pts.p,
                         dst->nrm.p, dst->gidx.p, s->vox_counts.p, cap, g);
    else
      hipLaunchKernelGGL(k_vox_scatter<false>, grid, block, 0, st, n, s->flags.p, s->vox_pts.p, s->vox_nrm.p, s->vox_cnt.p, dst->pts.p,
                         dst->nrm.p, dst->gidx.p, s->vox_counts.p, cap, g);
  };
  const auto before_wait = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(s->scalars.p + 8, ctr, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, s->vox_counts.p, sizeof(int) * (size_t) n, hipMemcpyDeviceToHost, st));
    return 0;
  };
  rc = srrg2amd::scene_compact_into(s, dst, n, scatter, before_wait);
  const int* const got = s->scalars.p + 8;
  if (rc || got[V_UNSUP]) {
    dst->n = dst_n, dst->ng = dst_ng;
    dst->has_normals = dst_normals, dst->has_desc = dst_desc, dst->has_inten = dst_inten;
    if (rc) return rc;
    return fail(SRRG2_E_UNSUPPORTED,
                "scene_voxelize: the cloud spans more cells of one leaf than the 63-bit cell key holds (2^30 per axis, 63 bits over "
                "the axes)");
  }
  if (out) {
    out->num_points           = n;
    out->num_finite           = got[V_FINITE];
    out->num_occupied         = got[V_OCCUPIED];
    out->num_voxels           = dst->n;
    out->num_with_normal      = got[V_WITH_NORMAL];
    out->max_points_per_voxel = got[V_MAX_POINTS];
  }
  return 0;
}
