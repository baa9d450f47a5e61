// desc_band.hip -- "the best 256-bit binary descriptor inside a band of image rows": the search the stereo matcher (stereo.hip,
// once per direction) and the feature tracker (tracking.hip) share, with its row table.  One compiled copy, launched through
// srrg2amd::launch_band_rows / launch_band_search (kernels.h).  Integer arithmetic and order-free minima throughout: the outputs
// are a function of the inputs alone, bit for bit (DESIGN.md section 4 "Banded descriptor search").
//   k_band_rows     row_begin[rows + 1] from the candidates' pixels, which ascend (raster order): thread i writes the rows that
//                   candidate i opens (boundary detection, no sort); with an error word the same pass checks the pixels
//   k_band_search   one wave per query: the lanes stride over the candidates of rows r - R .. r + R (one contiguous range), gate
//                   the column difference, take the Hamming distance (two 16-byte loads per side, four popcounts) and keep the
//                   smallest (distance << 32 | candidate index); a shuffle reduction gives the wave's.  SECOND: also the smallest
//                   distance of any other candidate.  REVERSE: every evaluated pair also sends ONE 64-bit atomicMin
//                   (distance << 32 | query index) to its candidate's word: a minimum does not depend on the order
// No launch is capped: one thread (or wave) per element and no loop behind a cap.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace {

using srrg2amd::NO_CANDIDATE;
using srrg2amd::NO_SECOND;

// pixel: n candidates' pixel indices, ascending.  row_begin[r] = the first candidate in row r or below it, row_begin[rows] = n.
// The rows are clamped into the image, so that every write stays inside row_begin whatever the pixels are.  error not null: a
// pixel outside [0, rows * cols) or not above its predecessor raises it (the search does nothing once it is set); null: the
// caller vouches for the pixels, and the clamp changes nothing.
__global__ __launch_bounds__(256) void k_band_rows(const int* __restrict__ pixel, int n, int rows, int cols, int* __restrict__ row_begin,
                                                   int* __restrict__ error) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  int cur = rows, prev = -1;
  if (i < n) {
    const int p = pixel[i];
    if (error && (p < 0 || p >= rows * cols || (i > 0 && pixel[i - 1] >= p))) *error = 1;
    cur = min(max(p / cols, 0), rows - 1);
  }
  if (i > 0) prev = min(max(pixel[i - 1] / cols, 0), rows - 1);
  for (int r = prev + 1; r <= cur; ++r) row_begin[r] = i;
}

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  const unsigned long long w0 = (unsigned long long) (a0.x ^ b0.x) | ((unsigned long long) (a0.y ^ b0.y) << 32);
  const unsigned long long w1 = (unsigned long long) (a0.z ^ b0.z) | ((unsigned long long) (a0.w ^ b0.w) << 32);
  const unsigned long long w2 = (unsigned long long) (a1.x ^ b1.x) | ((unsigned long long) (a1.y ^ b1.y) << 32);
  const unsigned long long w3 = (unsigned long long) (a1.z ^ b1.z) | ((unsigned long long) (a1.w ^ b1.w) << 32);
  return (__popcll(w0) + __popcll(w1)) + (__popcll(w2) + __popcll(w3));
}

// (best, second) of two disjoint candidate sets -> of their union: the smaller key wins; the loser's distance is a distance of
// "another candidate", as both seconds are.  NO_CANDIDATE's distance field is NO_SECOND: an empty side adds nothing.
template <bool SECOND>
__device__ __forceinline__ void merge_best(unsigned long long& key, unsigned& second, unsigned long long k, unsigned s) {
  if constexpr (SECOND) second = min(min(second, s), (unsigned) ((k < key ? key : k) >> 32));
  key = k < key ? k : key;
}

// One wave per query (4 per workgroup).  q_pixel[q] < 0: the query is skipped.  A candidate is inside the gate when
// lo <= its column - the query's column <= hi.  The candidates are in raster order, so the smaller candidate index is the
// smaller pixel index.  error null or *error == 0: search; else every query is left without a candidate.
template <bool SECOND, bool REVERSE>
__global__ __launch_bounds__(256) void k_band_search(int nq, const int* __restrict__ q_pixel, const uint4* __restrict__ q_desc,
                                                     const int* __restrict__ c_pixel, const uint4* __restrict__ c_desc,
                                                     const int* __restrict__ c_rows, int rows, int cols, int radius, int lo, int hi,
                                                     const int* __restrict__ error, unsigned long long* __restrict__ best,
                                                     unsigned* __restrict__ second, unsigned long long* __restrict__ reverse) {
  const int lane = threadIdx.x & 63;
  const int q    = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;  // (the whole wave)
  unsigned long long key = NO_CANDIDATE;
  unsigned sec           = NO_SECOND;
  const int pixel        = q_pixel[q];
  if (pixel >= 0 && !(error && *error)) {  // (the same for every lane)
    const int r = pixel / cols, c = pixel - r * cols;
    const int begin = c_rows[max(r - radius, 0)], end = c_rows[min(r + radius, rows - 1) + 1];
    const uint4 a0 = q_desc[2 * (size_t) q], a1 = q_desc[2 * (size_t) q + 1];
    const int* pj   = c_pixel + (begin + lane);  // (walked, not indexed: no address arithmetic in front of the loads)
    const uint4* dj = c_desc + 2 * (size_t) (begin + lane);
    for (int j = begin + lane; j < end; j += 64, pj += 64, dj += 128) {
      const int cp = *pj;
      const int dc = (cp - (cp / cols) * cols) - c;
      if (dc >= lo && dc <= hi) {
        const unsigned h = (unsigned) hamming(a0, a1, dj[0], dj[1]);
        merge_best<SECOND>(key, sec, ((unsigned long long) h << 32) | (unsigned) j, NO_SECOND);
        if constexpr (REVERSE) atomicMin(&reverse[j], ((unsigned long long) h << 32) | (unsigned) q);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long k = __shfl_xor(key, off);
      const unsigned s           = SECOND ? __shfl_xor(sec, off) : NO_SECOND;
      merge_best<SECOND>(key, sec, k, s);
    }
  }
  if (lane == 0) {
    best[q] = key;
    if constexpr (SECOND) second[q] = sec;
  }
}

}  // namespace

namespace srrg2amd {

void launch_band_rows(const int* pixel, int n, int rows, int cols, int* row_begin, int* error, hipStream_t s) {
  hipLaunchKernelGGL(k_band_rows, dim3((unsigned) (((long long) n + 256) / 256)), dim3(256), 0, s, pixel, n, rows, cols, row_begin, error);
}

void launch_band_search(int nq, const int* q_pixel, const uint4* q_desc, const int* c_pixel, const uint4* c_desc, const int* c_rows,
                        int rows, int cols, int radius, int lo, int hi, const int* error, unsigned long long* best, unsigned* second,
                        unsigned long long* reverse, hipStream_t s) {
  const dim3 grid((unsigned) ((nq + 3) / 4)), block(256);
#define BAND_SEARCH(SECOND, REVERSE)                                                                                               \
  hipLaunchKernelGGL((k_band_search<SECOND, REVERSE>), grid, block, 0, s, nq, q_pixel, q_desc, c_pixel, c_desc, c_rows, rows, cols, \
                     radius, lo, hi, error, best, second, reverse)
  if (reverse)  // (with the runner-up: the tracker is its only user)
    BAND_SEARCH(true, true);
  else if (second)
    BAND_SEARCH(true, false);
  else
    BAND_SEARCH(false, false);
#undef BAND_SEARCH
}

}  // namespace srrg2amd
