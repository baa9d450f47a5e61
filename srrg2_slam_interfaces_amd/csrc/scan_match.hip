// scan_match.hip -- srrg2_gridmap_build_likelihood / _get_likelihood / _match_scans: correlative scan matching against the
// occupancy grid, on the device.  No reference counterpart; DESIGN.md section 4 "Correlative scan matching" is the contract and
// tests/scan_match_restatement.py its executable form.  A beam's float work (the rotated guess composed with the mount, the end
// point, the float32 divide that makes a cell of it: gridmap.hip's expressions) happens once per (scan, rotation, beam); the
// scores behind it are integer sums of bytes, so results and volume are a function of the inputs alone, bit for bit.
//   k_field_build   the field is a dilation of the occupied cells: a workgroup owns 16 x 16 cells, the occupancy of the tile and
//                   its halo of R lies in LDS; a tile without an occupied cell in reach (most of a map) writes zeros and leaves
//   k_match_prep    one lane per (scan, rotation, beam): its end cell, or "dead" -- not a return, not traced, or out of the
//                   grid's reach for every shift of the window
//   k_match_score<LX, DY>  what the library runs: a workgroup owns one (scan, rotation) and a tile of shifts, LX along dx (a
//                   wave's lookups for one beam are LX consecutive bytes of 64 / LX field rows) by 256 / LX * DY along dy, a lane
//                   keeps DY shifts of dy in registers per beam cell.  The beam cells come through LDS in chunks, and only those
//                   that reach the grid under some shift of THIS tile are kept (integer adds commute: the order is free).  A
//                   lookup outside the grid reads the one zero byte behind the field: no branch.  The per-scan arg-max is ONE
//                   64-bit atomicMax per workgroup and tile on a key of score, guess flag and complemented flat index.
//                   LX is the one of 16 / 32 / 64 that pads a row of shifts least; a lane whose shifts all hang over the window
//                   looks nothing up, a wave of such lanes skips the beams.
//   k_match_score_plain  (make EXTRA=-DSRRG2_SCAN_MATCH_PLAIN=1 OUT=... and SRRG2_AMD_LIB): the obvious kernel the other is
//                   measured against -- one lane per candidate in flat order, the beam cells read from global memory; the tiled
//                   one is 3.6 times faster on 32 scans with a window of 81 x 81 cells x 81 rotations (DESIGN.md has both timings)
//   k_match_finish  one lane per scan: key -> result
// Everything runs on the grid's stream in order; one upload, one wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "det_math.h"
#include "device_util.h"
#include "gridmap_state.h"
#include "host_util.h"
#include "scan_beam.h"

using srrg2amd::fail;

#ifndef SRRG2_SCAN_MATCH_PLAIN
#define SRRG2_SCAN_MATCH_PLAIN 0
#endif

namespace {

enum { MAX_RADIUS = 16, LUT_BYTES = MAX_RADIUS * MAX_RADIUS + 1, FIELD_TILE = 16 };
enum { BEAM_CHUNK = 1024, MAX_SCORE_BLOCKS = 8192, MAX_PREP_BLOCKS = 8192, DEAD = INT_MIN };

struct Lut {
  unsigned char v[LUT_BYTES + 3];
};

__global__ __launch_bounds__(256) void k_field_build(const int* __restrict__ hits, const int* __restrict__ misses, int rows, int cols,
                                                     long long need, unsigned occupied, int R, Lut lut, int tiles_x,
                                                     unsigned char* __restrict__ field) {
  __shared__ unsigned char occ[(FIELD_TILE + 2 * MAX_RADIUS) * (FIELD_TILE + 2 * MAX_RADIUS)];
  __shared__ unsigned char sl[LUT_BYTES + 3];
  const int t = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int W = FIELD_TILE + 2 * R;
  int any = 0;
  for (int i = t; i < W * W; i += 256) {
    const int ly = i / W, lx = i - ly * W;
    const int gy = ty * FIELD_TILE + ly - R, gx = tx * FIELD_TILE + lx - R;
    unsigned char o = 0;
    if ((unsigned) gy < (unsigned) rows && (unsigned) gx < (unsigned) cols) {
      const long long at = (long long) gy * cols + gx;
      const unsigned v = cell_value(hits[at], misses[at], need);
      o = (v >= occupied && v <= 100u) ? 1 : 0;
    }
    occ[i] = o;
    any |= o;
  }
  for (int i = t; i <= R * R; i += 256) sl[i] = lut.v[i];
  any = __syncthreads_or(any);
  const int cy = t / FIELD_TILE, cx = t - cy * FIELD_TILE;
  const int gy = ty * FIELD_TILE + cy, gx = tx * FIELD_TILE + cx;
  if (gy >= rows || gx >= cols) return;
  unsigned best = 0;
  if (any) {
    for (int dy = -R; dy <= R; ++dy)
      for (int dx = -R; dx <= R; ++dx) {
        const int d2 = dx * dx + dy * dy;
        if (d2 <= R * R && occ[(cy + R + dy) * W + cx + R + dx]) best = max(best, (unsigned) sl[d2]);
      }
  }
  field[(long long) gy * cols + gx] = (unsigned char) best;
}

struct MatchArgs {
  const float* ranges;   // K * nb
  const float* guesses;  // 9 per scan
  int K, nb;
  double amin, ainc;
  float rmin, rmax;
  float S[9];
  int wx, wy, ht;  // half windows
  int nx, ny, nt;  // 2 w + 1
  int nc;          // candidates per scan
  double step;
  int rows, cols;
  float ox, oy, res;
};

// Pj of the contract: the guess of `scan` turned by j steps
__device__ __forceinline__ void rotated_guess(const MatchArgs& A, int scan, int j, float* P) {
  double s, c;
  dm::sincos(A.ht == 0 ? 0.0 : (double) j * A.step, s, c);
  const float cf = (float) c, sf = (float) s;
  const float R[9] = {cf, -sf, 0.f, sf, cf, 0.f, 0.f, 0.f, 1.f};
  dm::se2_compose(A.guesses + 9 * (long long) scan, R, P);
}

// aux: per scan the score at the guess, then the number of returns
__global__ __launch_bounds__(256) void k_match_prep(MatchArgs A, long long total, int2* __restrict__ cells, int* __restrict__ aux) {
  const long long per_scan = (long long) A.nt * A.nb;
  for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < total; i += (long long) gridDim.x * 256) {
    const int scan = (int) (i / per_scan);
    const int rem  = (int) (i - (long long) scan * per_scan);  // (total fits int32: the host's check)
    const int jj = rem / A.nb, k = rem - jj * A.nb;
    const float r  = A.ranges[(long long) scan * A.nb + k];
    int2 cell      = make_int2(DEAD, 0);
    if (isfinite(r) && A.rmin <= r && r <= A.rmax) {
      if (jj == 0) atomicAdd(&aux[2 * scan + 1], 1);
      float P[9], T[9];
      rotated_guess(A, scan, jj - A.ht, P);
      dm::se2_compose(P, A.S, T);
      const float2 b = scan_beam_point(A.amin, A.ainc, k, r);
      const float ex = (T[0] * b.x + T[1] * b.y) + T[2];
      const float ey = (T[3] * b.x + T[4] * b.y) + T[5];
      int x0, y0, x1, y1;
      if (cell_of(T[2], A.ox, A.res, x0) && cell_of(T[5], A.oy, A.res, y0) && cell_of(ex, A.ox, A.res, x1) &&
          cell_of(ey, A.oy, A.res, y1) && max(abs(x1 - x0), abs(y1 - y0)) <= GRIDMAP_MAX_RAY) {
        // in reach of the grid under some shift of the window (64-bit: a coordinate and a half window are below 2^30 each)
        if ((long long) x1 + A.wx >= 0 && (long long) x1 - A.wx < A.cols && (long long) y1 + A.wy >= 0 && (long long) y1 - A.wy < A.rows)
          cell = make_int2(x1, y1);
      }
    }
    cells[i] = cell;
  }
}

// score, then the guess flag, then the complemented flat index: the greatest key is the best candidate of the contract
// (0 is no candidate's key: a flat index stays below 2^31 - 1)
__device__ __forceinline__ unsigned long long key_of(int score, bool is_guess, int flat) {
  return ((unsigned long long) (unsigned) score << 32) | (is_guess ? 0x80000000ull : 0ull) | (unsigned long long) (0x7fffffffu - (unsigned) flat);
}

template <int LX, int DY>
__global__ __launch_bounds__(256) void k_match_score(MatchArgs A, const int2* __restrict__ cells, const unsigned char* __restrict__ field,
                                                     long long tiles, int tiles_x, int tiles_y, unsigned long long* __restrict__ words,
                                                     int* __restrict__ aux, int* __restrict__ volume) {
  constexpr int TY = (256 / LX) * DY;
  __shared__ int4 sb[BEAM_CHUNK];  // x1, y1, y1 * cols + x1 (mod 2^32)
  __shared__ int n_live;
  __shared__ unsigned long long red[4];
  const int t = threadIdx.x;
  const unsigned zero_at = (unsigned) A.rows * (unsigned) A.cols;  // the zero byte behind the field
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    long long rest = tile / tiles_x;
    const int tx   = (int) (tile - rest * tiles_x);
    const int ty   = (int) (rest % tiles_y);
    rest /= tiles_y;
    const int jj = (int) (rest % A.nt), scan = (int) (rest / A.nt);
    // (64-bit: a tile may hang over the window by up to LX - 1 and TY - 1 shifts)
    const long long dx0 = (long long) tx * LX - A.wx, dy0 = (long long) ty * TY - A.wy;
    const long long dxi = (long long) tx * LX + (t % LX), dyi0 = (long long) ty * TY + (t / LX) * DY;
    // the shifts of the tile that are candidates (the rest hangs over the window), and whether this lane holds one: a lane
    // without looks nothing up, and a wave of such lanes skips the beams
    const int wide = (int) min((long long) LX, A.nx - (long long) tx * LX), high = (int) min((long long) TY, A.ny - (long long) ty * TY);
    const bool holds = dxi < A.nx && dyi0 < A.ny;
    const unsigned dx = (unsigned) (dxi - A.wx);  // (mod 2^32 from here on: an index inside the grid comes out exact)
    unsigned dy[DY], off[DY];
    int acc[DY];
#pragma unroll
    for (int q = 0; q < DY; ++q) {
      dy[q]  = (unsigned) (dyi0 + q - A.wy);
      off[q] = dy[q] * (unsigned) A.cols + dx;
      acc[q] = 0;
    }
    const int2* const mine = cells + ((long long) scan * A.nt + jj) * A.nb;
    for (int b0 = 0; b0 < A.nb; b0 += BEAM_CHUNK) {
      __syncthreads();
      if (t == 0) n_live = 0;
      __syncthreads();
      const int end = min(A.nb, b0 + BEAM_CHUNK);
      for (int b = b0 + t; b < end; b += 256) {
        const int2 c = mine[b];
        if (c.x == DEAD) continue;
        const long long xl = (long long) c.x + dx0, yl = (long long) c.y + dy0;  // the first cell this tile looks up for the beam
        if (xl + wide <= 0 || xl >= A.cols || yl + high <= 0 || yl >= A.rows) continue;
        sb[atomicAdd(&n_live, 1)] = make_int4(c.x, c.y, (int) ((unsigned) c.y * (unsigned) A.cols + (unsigned) c.x), 0);
      }
      __syncthreads();
      const int n = n_live;
      for (int i = 0; holds && i < n; ++i) {
        const int4 c   = sb[i];
        const bool okx = (unsigned) c.x + dx < (unsigned) A.cols;
#pragma unroll
        for (int q = 0; q < DY; ++q) {
          const bool ok = okx && (unsigned) c.y + dy[q] < (unsigned) A.rows;
          acc[q] += (int) field[ok ? (unsigned) c.z + off[q] : zero_at];
        }
      }
    }
    unsigned long long best = 0;
    if (dxi < A.nx) {
#pragma unroll
      for (int q = 0; q < DY; ++q) {
        const long long dyi = dyi0 + q;
        if (dyi >= A.ny) continue;
        const int flat      = (int) (((long long) jj * A.ny + dyi) * A.nx + dxi);
        const bool is_guess = jj == A.ht && dyi == A.wy && dxi == A.wx;
        if (is_guess) aux[2 * scan] = acc[q];
        if (volume) volume[(long long) scan * A.nc + flat] = acc[q];
        best = max(best, key_of(acc[q], is_guess, flat));
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, (unsigned long long) __shfl_xor((long long) best, o));
    __syncthreads();  // (thread 0 has read red[] of the tile before)
    if ((t & 63) == 0) red[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
      const unsigned long long m = max(max(red[0], red[1]), max(red[2], red[3]));
      if (m) atomicMax(&words[scan], m);
    }
  }
}

// the floor: one lane per candidate in flat order
__global__ __launch_bounds__(256) void k_match_score_plain(MatchArgs A, const int2* __restrict__ cells, const unsigned char* __restrict__ field,
                                                           long long total, unsigned long long* __restrict__ words, int* __restrict__ aux,
                                                           int* __restrict__ volume) {
  for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < total; i += (long long) gridDim.x * 256) {
    const int scan = (int) (i / A.nc), flat = (int) (i - (long long) scan * A.nc);
    const int dxi = flat % A.nx, rest = flat / A.nx;
    const int dyi = rest % A.ny, jj = rest / A.ny;
    const int2* const mine = cells + ((long long) scan * A.nt + jj) * A.nb;
    int acc = 0;
    for (int b = 0; b < A.nb; ++b) {
      const int2 c = mine[b];
      if (c.x == DEAD) continue;
      const long long x = (long long) c.x + dxi - A.wx, y = (long long) c.y + dyi - A.wy;
      if (x >= 0 && x < A.cols && y >= 0 && y < A.rows) acc += (int) field[y * A.cols + x];
    }
    const bool is_guess = jj == A.ht && dyi == A.wy && dxi == A.wx;
    if (is_guess) aux[2 * scan] = acc;
    if (volume) volume[i] = acc;
    const unsigned long long key = key_of(acc, is_guess, flat);
    if (key > words[scan]) atomicMax(&words[scan], key);  // (the word only grows: a stale read costs an atomic, never a winner)
  }
}

__global__ __launch_bounds__(256) void k_match_finish(MatchArgs A, const unsigned long long* __restrict__ words, const int* __restrict__ aux,
                                                      srrg2_gridmap_match_result* __restrict__ out) {
  const int scan = blockIdx.x * 256 + threadIdx.x;
  if (scan >= A.K) return;
  const unsigned long long key = words[scan];
  const int flat = (int) (0x7fffffffu - ((unsigned) key & 0x7fffffffu));
  const int dxi = flat % A.nx, rest = flat / A.nx;
  const int dyi = rest % A.ny, jj = rest / A.ny;
  srrg2_gridmap_match_result r;
  rotated_guess(A, scan, jj - A.ht, r.robot_in_world);
  r.dx = dxi - A.wx, r.dy = dyi - A.wy, r.jtheta = jj - A.ht;
  r.robot_in_world[2] = r.robot_in_world[2] + (float) r.dx * A.res;
  r.robot_in_world[5] = r.robot_in_world[5] + (float) r.dy * A.res;
  r.score            = (int) (key >> 32);
  r.score_at_guess   = aux[2 * scan];
  r.num_scored_beams = aux[2 * scan + 1];
  out[scan]          = r;
}

int check_field_call(const std::string& who, int occupied_percent, int radius_cells, const uint8_t* lut) {
  if (radius_cells < 0 || radius_cells > MAX_RADIUS) return fail(SRRG2_E_INVALID, who + "radius_cells 0 .. 16");
  if (occupied_percent < 0 || occupied_percent > 100) return fail(SRRG2_E_INVALID, who + "occupied_percent 0 .. 100");
  if (!lut) return fail(SRRG2_E_INVALID, who + "null lut");
  return 0;
}

int fresh(const std::string& who, const srrg2_gridmap_s* h) {
  if (!h->field_fresh) return fail(SRRG2_E_INVALID, who + "the likelihood field is stale or was never built (srrg2_gridmap_build_likelihood)");
  return 0;
}

}  // namespace

extern "C" int srrg2_gridmap_default_likelihood_lut(int radius_cells, uint8_t* lut) {
  const std::string who = "gridmap_default_likelihood_lut: ";
  if (radius_cells < 0 || radius_cells > MAX_RADIUS) return fail(SRRG2_E_INVALID, who + "radius_cells 0 .. 16");
  if (!lut) return fail(SRRG2_E_INVALID, who + "null lut");
  const int n = radius_cells * radius_cells + 1;
  for (int d2 = 0; d2 < n; ++d2) lut[d2] = (uint8_t) ((255 * (n - d2)) / n);
  return 0;
}

extern "C" int srrg2_gridmap_build_likelihood(srrg2_gridmap_h h, int min_observations, int occupied_percent, int radius_cells,
                                              const uint8_t* lut) {
  const std::string who = "gridmap_build_likelihood: ";
  int rc;
  if ((rc = check_field_call(who, occupied_percent, radius_cells, lut))) return rc;
  if ((rc = srrg2amd::gridmap_ready(who, h))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st     = h->stream();
  const size_t cells = (size_t) h->cells();
  h->field_fresh     = false;
  if ((rc = h->field.reserve(cells + 1))) return rc;
  HIP_TRY(hipMemsetAsync(h->field.p + cells, 0, 1, st));  // what a lookup outside the grid reads
  if (cells > 0) {
    Lut L;
    std::memset(&L, 0, sizeof(L));
    std::memcpy(L.v, lut, (size_t) radius_cells * radius_cells + 1);
    const int tiles_x = (h->p.cols + FIELD_TILE - 1) / FIELD_TILE, tiles_y = (h->p.rows + FIELD_TILE - 1) / FIELD_TILE;  // (<= 2048 each)
    hipLaunchKernelGGL(k_field_build, dim3(tiles_x * tiles_y), dim3(256), 0, st, h->planes.p, h->planes.p + cells, h->p.rows, h->p.cols,
                       (long long) std::max(min_observations, 1), (unsigned) occupied_percent, radius_cells, L, tiles_x, h->field.p);
    HIP_TRY(hipGetLastError());
  }
  h->field_fresh = true;
  return 0;
}

extern "C" int srrg2_gridmap_get_likelihood(srrg2_gridmap_h h, uint8_t* dst, int row_stride_bytes, int mem) {
  const std::string who = "gridmap_get_likelihood: ";
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  int rc;
  if ((rc = srrg2amd::gridmap_ready(who, h)) || (rc = fresh(who, h))) return rc;
  const int rows = h->p.rows, cols = h->p.cols;
  if (h->cells() == 0) return 0;
  if (!dst) return fail(SRRG2_E_INVALID, who + "null image");
  if (row_stride_bytes < cols) return fail(SRRG2_E_INVALID, who + "row stride smaller than a row");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t) row_stride_bytes, h->field.p, (size_t) cols, (size_t) cols, (size_t) rows,
                           mem == SRRG2_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream()));
  HIP_TRY(hipStreamSynchronize(h->stream()));
  h->upload_pending = false;
  return 0;
}

extern "C" int srrg2_gridmap_match_scans(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* guess_robot_in_world, int mem,
                                         const srrg2_gridmap_scan_params* p, const srrg2_gridmap_match_params* mp,
                                         srrg2_gridmap_match_result* results, int32_t* scores_out, int scores_mem) {
  const std::string who = "gridmap_match_scans: ";
  int rc;
  if (!mp) return fail(SRRG2_E_INVALID, who + "null match params");
  if (mp->half_window_x < 0 || mp->half_window_y < 0 || mp->half_steps_theta < 0)
    return fail(SRRG2_E_INVALID, who + "half windows and half_steps_theta >= 0");
  if (mp->half_steps_theta > 0 && (!std::isfinite(mp->theta_step) || !(mp->theta_step > 0.0)))
    return fail(SRRG2_E_INVALID, who + "theta_step must be finite and > 0");
  if ((rc = srrg2amd::gridmap_check_scan_call(who, ranges, num_scans, guess_robot_in_world, mem, p, 1))) return rc;
  // (the guesses are read even when num_beams = 0: a scan without beams gets its guess back)
  if (num_scans > 0 && (!guess_robot_in_world || reinterpret_cast<uintptr_t>(guess_robot_in_world) % 4 != 0))
    return fail(SRRG2_E_INVALID, who + "null or misaligned guesses");
  if (num_scans > 0 && !results) return fail(SRRG2_E_INVALID, who + "null results");
  if (scores_out && scores_mem != SRRG2_MEM_HOST && scores_mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad scores_mem");
  if (reinterpret_cast<uintptr_t>(scores_out) % 4 != 0) return fail(SRRG2_E_INVALID, who + "misaligned scores_out");
  const long long nx = 2LL * mp->half_window_x + 1, ny = 2LL * mp->half_window_y + 1, nt = 2LL * mp->half_steps_theta + 1;
  // (three factors below 2^32: the product of two is tested before the third comes in)
  if (nx * ny > 0x7fffffffLL || nx * ny * nt > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "candidates per scan beyond int32");
  const long long nc = nx * ny * nt;
  if (scores_out && nc * num_scans > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "score volume beyond int32 elements");
  // (one end cell per scan, rotation and beam is kept: 8 bytes each)
  if ((long long) num_scans * p->num_beams * nt > 0x7fffffffLL)
    return fail(SRRG2_E_UNSUPPORTED, who + "num_scans * num_beams * rotations beyond int32");
  if ((rc = srrg2amd::gridmap_ready(who, h))) return rc;
  if (!(p->range_max / h->p.resolution <= GRIDMAP_MAX_STEPS)) return fail(SRRG2_E_INVALID, who + "range_max / resolution beyond 32000 cells");
  if ((rc = fresh(who, h))) return rc;
  if (num_scans == 0) return 0;
  const int K = num_scans, nb = p->num_beams;
  const long long beams = (long long) K * nb, prep_total = beams * nt;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  MatchArgs A;
  std::memset(&A, 0, sizeof(A));
  A.ranges = ranges, A.guesses = guess_robot_in_world;
  {  // ONE upload: the ranges, then the guesses, through the pinned block (the protocol of srrg2_gridmap_integrate_scans)
    const size_t br = (size_t) beams * 4, bp = (size_t) K * 36;
    if (mem == SRRG2_MEM_HOST) {
      if (h->upload_pending) {
        HIP_TRY(hipEventSynchronize(h->uploaded));
        h->upload_pending = false;
      }
      if ((rc = h->host_stage.reserve(br + bp, (br + bp) / 8)) || (rc = h->stage.reserve(br + bp))) return rc;
      if (br) std::memcpy(h->host_stage.p, ranges, br);
      std::memcpy(h->host_stage.p + br, guess_robot_in_world, bp);
      HIP_TRY(hipMemcpyAsync(h->stage.p, h->host_stage.p, br + bp, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(h->uploaded, st));
      h->upload_pending = true;
      A.ranges  = reinterpret_cast<const float*>(h->stage.p);
      A.guesses = reinterpret_cast<const float*>(h->stage.p + br);
    }
  }
  A.K = K, A.nb = nb;
  A.amin = p->angle_min, A.ainc = p->angle_increment;
  A.rmin = p->range_min, A.rmax = p->range_max;
  std::memcpy(A.S, p->sensor_in_robot, sizeof(A.S));
  A.wx = mp->half_window_x, A.wy = mp->half_window_y, A.ht = mp->half_steps_theta;
  A.nx = (int) nx, A.ny = (int) ny, A.nt = (int) nt, A.nc = (int) nc;
  A.step = mp->theta_step;
  A.rows = h->p.rows, A.cols = h->p.cols;
  A.ox = h->p.origin[0], A.oy = h->p.origin[1], A.res = h->p.resolution;
  const bool to_host = scores_out && scores_mem == SRRG2_MEM_HOST;
  if ((rc = h->match_cells.reserve((size_t) prep_total + 1)) || (rc = h->match_words.reserve(2 * (size_t) K)) ||
      (rc = h->match_results.reserve((size_t) K)) || (rc = h->match_results_host.reserve((size_t) K, (size_t) K / 8)) ||
      (to_host && (rc = h->match_volume.reserve((size_t) nc * K))))
    return rc;
  unsigned long long* const words = h->match_words.p;
  int* const aux                  = reinterpret_cast<int*>(words + K);
  int* const volume               = to_host ? h->match_volume.p : scores_out;
  HIP_TRY(hipMemsetAsync(words, 0, 2 * (size_t) K * sizeof(unsigned long long), st));
  if (prep_total > 0) {
    const int blocks = (int) std::min<long long>((prep_total + 255) / 256, MAX_PREP_BLOCKS);
    hipLaunchKernelGGL(k_match_prep, dim3(blocks), dim3(256), 0, st, A, prep_total, h->match_cells.p, aux);
    HIP_TRY(hipGetLastError());
  }
#if SRRG2_SCAN_MATCH_PLAIN
  {
    const long long total = nc * K;
    const int blocks      = (int) std::min<long long>((total + 255) / 256, MAX_SCORE_BLOCKS);
    hipLaunchKernelGGL(k_match_score_plain, dim3(blocks), dim3(256), 0, st, A, h->match_cells.p, h->field.p, total, words, aux, volume);
  }
#else
  {
    // lanes along dx: 16, 32 or 64, whichever pads the row of nx shifts least (the wider on a tie), the rest of the wave goes
    // to further rows of dy
    const auto launch = [&](auto kernel, int LX, int TY) {
      const long long tiles_x = (nx + LX - 1) / LX, tiles_y = (ny + TY - 1) / TY;
      const long long tiles   = tiles_x * tiles_y * nt * K;
      const int blocks        = (int) std::min<long long>(tiles, MAX_SCORE_BLOCKS);
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, A, h->match_cells.p, h->field.p, tiles, (int) tiles_x, (int) tiles_y, words,
                         aux, volume);
    };
    if (nx <= 16)
      launch(k_match_score<16, 4>, 16, 64);
    else if ((nx + 31) / 32 * 32 < (nx + 63) / 64 * 64)
      launch(k_match_score<32, 4>, 32, 32);
    else
      launch(k_match_score<64, 4>, 64, 16);
  }
#endif
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_match_finish, dim3((K + 255) / 256), dim3(256), 0, st, A, words, aux, h->match_results.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->match_results_host.p, h->match_results.p, (size_t) K * sizeof(srrg2_gridmap_match_result), hipMemcpyDeviceToHost, st));
  if (to_host) HIP_TRY(hipMemcpyAsync(scores_out, h->match_volume.p, (size_t) nc * K * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait
  h->upload_pending = false;
  std::memcpy(results, h->match_results_host.p, (size_t) K * sizeof(srrg2_gridmap_match_result));
  return 0;
}
