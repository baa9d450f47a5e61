// cell_grid.h -- points binned into float64 cells behind a 64-bit key: what normals.hip (cells a little larger than the radius,
// anchored at the box minimum) and voxel.hip (cells of one leaf, anchored at a corner the caller names) share.  Internal to the
// library.
//   k_grid_bbox     box of the finite points (dim coordinates) + their number
//   k_grid_spec     one thread: cells per axis and the bits each axis gets in the key, or "beyond the key range"
//   k_grid_keys     cell key of every point (x fastest); non-finite points get the all-ones key and sort to the end
// A cell coordinate is floor((p - org) / h) in float64; the key holds it relative to the lowest occupied cell of its axis (c0,
// itself a floor: monotone in p, so the box of the points gives the box of the cells).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// a cell coordinate has at most 30 bits, the three of them 63 in all
#define SRRG2_GRID_AXIS_BITS 30
#define SRRG2_GRID_KEY_BITS 63

// words of the counters block (ints) the grid kernels use: [0] finite points, [5] beyond the key range, [8, 11) complemented keys
// of the box minimum, [11, 14) keys of the maximum (zero-initialised, atomicMax).  The words in between are the caller's.
enum { GRID_FINITE = 0, GRID_UNSUP = 5, GRID_MIN = 8, GRID_MAX = 11, GRID_WORDS = 16 };

struct GridSpec {  // written by k_grid_spec
  double org[3], h;
  double c0[3];  // the lowest occupied cell per axis
  int cmax[3], shift[3];
  int unsupported, nfinite;
};

struct GridAnchor {  // anchored = 0: the cells start at the box minimum; 1: at `origin`
  double h;
  double origin[3];
  int anchored;
};

__device__ __forceinline__ unsigned okey(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int DIM>
__device__ __forceinline__ bool grid_finite(const float4 p) {
  return isfinite(p.x) && isfinite(p.y) && (DIM == 2 || isfinite(p.z));
}

template <int DIM>
__global__ __launch_bounds__(256) void k_grid_bbox(const float4* __restrict__ pts, int n, int* __restrict__ ctr) {
  unsigned mn[3] = {0u, 0u, 0u}, mx[3] = {0u, 0u, 0u};  // (mn complemented: a maximum as well)
  int valid = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    if (!grid_finite<DIM>(p)) continue;
    ++valid;
    const float v[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const unsigned k = okey(v[d]);
      mn[d] = max(mn[d], ~k);
      mx[d] = max(mx[d], k);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      mn[d] = max(mn[d], (unsigned) __shfl_xor((int) mn[d], off));
      mx[d] = max(mx[d], (unsigned) __shfl_xor((int) mx[d], off));
    }
    valid += __shfl_xor(valid, off);
  }
  if ((threadIdx.x & 63) == 0 && valid) {  // one atomic per wave and word (a few grid-striding blocks)
    unsigned* u = reinterpret_cast<unsigned*>(ctr);
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      atomicMax(&u[GRID_MIN + d], mn[d]);
      atomicMax(&u[GRID_MAX + d], mx[d]);
    }
    atomicAdd(&ctr[GRID_FINITE], valid);
  }
}

// the cell coordinate of the contract, as a float64 whole number
__device__ __forceinline__ double grid_cell_abs(double p, double org, double h) { return floor((p - org) / h); }

__device__ __forceinline__ int grid_cell(double p, double org, double h, double c0, int cmax) {
  const double q = grid_cell_abs(p, org, h) - c0;
  return q < 0.0 ? 0 : (q > (double) cmax ? cmax : (int) q);  // (inside by monotonicity; the clamp keeps a key's fields apart)
}

__global__ void k_grid_spec(int dim, GridAnchor A, int* __restrict__ ctr, GridSpec* __restrict__ spec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned* u = reinterpret_cast<const unsigned*>(ctr);
  GridSpec S;
  S.h           = A.h;
  S.nfinite     = ctr[GRID_FINITE];
  S.unsupported = 0;
  int bits_total = 0;
  for (int d = 0; d < 3; ++d) {
    S.org[d] = 0.0, S.c0[d] = 0.0, S.cmax[d] = 0, S.shift[d] = bits_total;
    if (d >= dim || S.nfinite == 0) continue;
    const double lo = (double) okey_inv(~u[GRID_MIN + d]);
    S.org[d]        = A.anchored ? A.origin[d] : lo;
    S.c0[d]         = grid_cell_abs(lo, S.org[d], S.h);  // (at the box minimum: floor(0 / h) = 0)
    const double q  = grid_cell_abs((double) okey_inv(u[GRID_MAX + d]), S.org[d], S.h) - S.c0[d];
    if (!(q < (double) (1 << SRRG2_GRID_AXIS_BITS))) {  // (NaN included)
      S.unsupported = 1;
      continue;
    }
    S.cmax[d] = (int) q;
    bits_total += 32 - __clz(S.cmax[d]);
  }
  if (bits_total > SRRG2_GRID_KEY_BITS) S.unsupported = 1;
  ctr[GRID_UNSUP] = S.unsupported;
  *spec           = S;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_grid_keys(const GridSpec* __restrict__ spec, const float4* __restrict__ pts, int n,
                                                   unsigned long long* __restrict__ keys, int* __restrict__ idx) {
  const GridSpec S = *spec;
  if (S.unsupported) return;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p         = pts[i];
    unsigned long long key = ~0ull;
    if (grid_finite<DIM>(p)) {
      key = (unsigned long long) grid_cell((double) p.x, S.org[0], S.h, S.c0[0], S.cmax[0]) |
            ((unsigned long long) grid_cell((double) p.y, S.org[1], S.h, S.c0[1], S.cmax[1]) << S.shift[1]);
      if (DIM == 3) key |= (unsigned long long) grid_cell((double) p.z, S.org[2], S.h, S.c0[2], S.cmax[2]) << S.shift[2];
    }
    keys[i] = key;
    idx[i]  = i;
  }
}

}  // namespace
