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
// srrg2_gridmap_build_bounds / _get_bounds / _match_scans_pruned, the same search through upper bounds, are the second half of the file.
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
  h->stale_field();  // (the bound planes are of the old field)
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

namespace {

// what srrg2_gridmap_match_scans and srrg2_gridmap_match_scans_pruned refuse without looking at their handle
int check_match_call(const std::string& who, const float* ranges, int num_scans, const float* guess_robot_in_world, int mem,
                     const srrg2_gridmap_scan_params* p, const srrg2_gridmap_match_params* mp, const void* results) {
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
  return 0;
}

// ... and of the window's size, still without the handle
int check_match_sizes(const std::string& who, const srrg2_gridmap_match_params* mp) {
  const long long nx = 2LL * mp->half_window_x + 1, ny = 2LL * mp->half_window_y + 1, nt = 2LL * mp->half_steps_theta + 1;
  // (three factors below 2^32: the product of two is tested before the third comes in)
  if (nx * ny > 0x7fffffffLL || nx * ny * nt > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "candidates per scan beyond int32");
  return 0;
}

// (one end cell per scan, rotation and beam is kept: 8 bytes each)
int check_match_cells(const std::string& who, int num_scans, const srrg2_gridmap_scan_params* p, const srrg2_gridmap_match_params* mp) {
  if ((long long) num_scans * p->num_beams * (2LL * mp->half_steps_theta + 1) > 0x7fffffffLL)
    return fail(SRRG2_E_UNSUPPORTED, who + "num_scans * num_beams * rotations beyond int32");
  return 0;
}

// ONE upload: the ranges, then the guesses, through the pinned block (the protocol of srrg2_gridmap_integrate_scans); then what
// the kernels need to know of the call
int stage_match(srrg2_gridmap_s* h, const float* ranges, int K, const float* guess_robot_in_world, int mem, const srrg2_gridmap_scan_params* p,
                const srrg2_gridmap_match_params* mp, MatchArgs& A) {
  int rc;
  hipStream_t st = h->stream();
  const int nb   = p->num_beams;
  std::memset(&A, 0, sizeof(A));
  A.ranges = ranges, A.guesses = guess_robot_in_world;
  const size_t br = (size_t) K * nb * 4, bp = (size_t) K * 36;
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
  A.K = K, A.nb = nb;
  A.amin = p->angle_min, A.ainc = p->angle_increment;
  A.rmin = p->range_min, A.rmax = p->range_max;
  std::memcpy(A.S, p->sensor_in_robot, sizeof(A.S));
  A.wx = mp->half_window_x, A.wy = mp->half_window_y, A.ht = mp->half_steps_theta;
  A.nx = 2 * A.wx + 1, A.ny = 2 * A.wy + 1, A.nt = 2 * A.ht + 1, A.nc = A.nx * A.ny * A.nt;
  A.step = mp->theta_step;
  A.rows = h->p.rows, A.cols = h->p.cols;
  A.ox = h->p.origin[0], A.oy = h->p.origin[1], A.res = h->p.resolution;
  return 0;
}

}  // namespace

extern "C" int srrg2_gridmap_match_scans(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* guess_robot_in_world, int mem,
                                         const srrg2_gridmap_scan_params* p, const srrg2_gridmap_match_params* mp,
                                         srrg2_gridmap_match_result* results, int32_t* scores_out, int scores_mem) {
  const std::string who = "gridmap_match_scans: ";
  int rc;
  if ((rc = check_match_call(who, ranges, num_scans, guess_robot_in_world, mem, p, mp, results))) return rc;
  if (scores_out && scores_mem != SRRG2_MEM_HOST && scores_mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad scores_mem");
  if (reinterpret_cast<uintptr_t>(scores_out) % 4 != 0) return fail(SRRG2_E_INVALID, who + "misaligned scores_out");
  if ((rc = check_match_sizes(who, mp))) return rc;
  const long long nx = 2LL * mp->half_window_x + 1, ny = 2LL * mp->half_window_y + 1, nt = 2LL * mp->half_steps_theta + 1;
  const long long nc = nx * ny * nt;
  if (scores_out && nc * num_scans > 0x7fffffffLL) return fail(SRRG2_E_UNSUPPORTED, who + "score volume beyond int32 elements");
  if ((rc = check_match_cells(who, num_scans, p, mp))) return rc;
  if ((rc = srrg2amd::gridmap_ready(who, h))) return rc;
  if (!(p->range_max / h->p.resolution <= GRIDMAP_MAX_STEPS)) return fail(SRRG2_E_INVALID, who + "range_max / resolution beyond 32000 cells");
  if ((rc = fresh(who, h))) return rc;
  if (num_scans == 0) return 0;
  const int K = num_scans;
  const long long prep_total = (long long) K * p->num_beams * nt;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  MatchArgs A;
  if ((rc = stage_match(h, ranges, K, guess_robot_in_world, mem, p, mp, A))) return rc;
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

// ---- pruned scan matching (DESIGN.md section 4 "Pruned scan matching", tests/scan_match_pruned_restatement.py) -------------------
// The window of srrg2_gridmap_match_scans searched through bound planes: P_l holds per cell the maximum of the field over the block
// of side 2^l that starts there, so the sum of P_l under a rotation's beam cells, moved to a block's first shift, bounds every
// candidate of the block.  Level-synchronous, one launch per step, sized from counts in device memory:
//   k_bounds_build     P_l from P_(l-1): one lane per byte, a 2 x 2 maximum at offset 2^(l-1)
//   k_prune_top        the dense top level, the shape of k_match_score: a workgroup owns one (scan, rotation) and 256 blocks, the
//                      live beam cells come through LDS; a wave's lookups for one beam are bytes 2^L apart.  Writes every bound
//                      and, with one atomicMax per workgroup, the scan's seed (highest bound, lowest flat block index)
//   k_prune_seed       the seed block's candidates and the guess, exactly: the floor is the score part of the scan's word
//   k_prune_expand_top the top blocks against the floor; the children of the survivors go to the scan's list
//   k_prune_level      one lane per listed block: its bound (beam cells from global memory), the survival test, its children
//   k_prune_exact      one lane per listed candidate: its score, one atomicMax per workgroup
//   k_prune_fallback   launched always: a scan whose list overflowed is scored exhaustively, one lane per candidate; without such
//                      a scan every workgroup leaves after reading K flags
//   k_prune_stats      one lane per scan
// A list belongs to one scan (its segment of `cap` entries): a workgroup reserves room for its children with ONE atomicAdd on the
// scan's counter, which goes on counting past the segment's end -- whether a scan falls back depends on its inputs alone.
namespace {

enum { MAX_LEVELS = 6, BOUNDS_BLOCKS = 2048, TOP_BLOCKS = 2048, SEED_BLOCKS = 1024, EXPAND_BLOCKS = 512, LIST_BLOCKS = 256, FALLBACK_BLOCKS = 2048 };
enum { DEFAULT_LIST_ENTRIES = 1 << 20 };
// per scan: the floor, whether the guess holds it, the seed block; per level the entries listed for it and its survivors
enum { ST_FLOOR = 0, ST_STRICT = 1, ST_SEED = 2, ST_COUNT = 4, ST_SURV = ST_COUNT + MAX_LEVELS + 1, STATE_INTS = ST_SURV + MAX_LEVELS + 1 };

// a bound plane (or the field: s = 1): P(x, y) = p[(y + s - 1) * W + x + s - 1] inside, p[zero] = 0 outside
struct Plane {
  const unsigned char* p;
  long long zero;
  int W, H, s;
};

__global__ __launch_bounds__(256) void k_bounds_build(const unsigned char* __restrict__ prev, int pw, int ph, unsigned char* __restrict__ out,
                                                      int ow, int oh, int half) {
  const long long total = (long long) ow * oh;
  for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < total; i += (long long) gridDim.x * 256) {
    const int Y = (int) (i / ow), X = (int) (i - (long long) Y * ow);
    unsigned best = 0;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int y = Y - b * half, x = X - a * half;
        if ((unsigned) y < (unsigned) ph && (unsigned) x < (unsigned) pw) best = max(best, (unsigned) prev[(long long) y * pw + x]);
      }
    out[i] = (unsigned char) best;
  }
}

// the sum of P under the beam cells of one (scan, rotation), read from global memory, moved by (ox, oy) plane cells
__device__ __forceinline__ int sum_under(const Plane& pl, const int2* __restrict__ mine, int nb, long long ox, long long oy) {
  int acc = 0;
  for (int b = 0; b < nb; ++b) {
    const int2 c = mine[b];
    if (c.x == DEAD) continue;
    const long long X = c.x + ox, Y = c.y + oy;
    const bool ok = X >= 0 && X < pl.W && Y >= 0 && Y < pl.H;
    acc += (int) pl.p[ok ? Y * pl.W + X : pl.zero];
  }
  return acc;
}

// the greatest key of the workgroup, in thread 0 (red: 4 words of LDS; every thread calls)
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, (unsigned long long) __shfl_xor((long long) v, o));
  __syncthreads();  // (thread 0 has read red[] of the round before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_prune_top(MatchArgs A, Plane pl, int nbx, int nby, long long tiles, int chunks,
                                                   const int2* __restrict__ cells, int* __restrict__ top, unsigned long long* __restrict__ seeds) {
  __shared__ int2 sb[BEAM_CHUNK];
  __shared__ int n_live;
  __shared__ unsigned long long red[4];
  const int t  = threadIdx.x;
  const int NB = nbx * nby;  // (<= Nx Ny)
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int chunk = (int) (tile % chunks);
    const long long rest = tile / chunks;
    const int jj = (int) (rest % A.nt), scan = (int) (rest / A.nt);
    const long long q = (long long) chunk * 256 + t;
    const bool holds  = q < NB;
    const int by = holds ? (int) (q / nbx) : 0, bx = holds ? (int) (q - (long long) by * nbx) : 0;
    const long long ox = (long long) bx * pl.s - A.wx + pl.s - 1, oy = (long long) by * pl.s - A.wy + pl.s - 1;
    const int2* const mine = cells + ((long long) scan * A.nt + jj) * A.nb;
    int acc = 0;
    for (int b0 = 0; b0 < A.nb; b0 += BEAM_CHUNK) {
      __syncthreads();
      if (t == 0) n_live = 0;
      __syncthreads();
      const int end = min(A.nb, b0 + BEAM_CHUNK);
      for (int b = b0 + t; b < end; b += 256) {
        const int2 c = mine[b];
        if (c.x != DEAD) sb[atomicAdd(&n_live, 1)] = c;  // (integer adds commute: the order is free)
      }
      __syncthreads();
      const int n = n_live;
      for (int i = 0; holds && i < n; ++i) {
        const int2 c = sb[i];
        const long long X = c.x + ox, Y = c.y + oy;
        const bool ok = X >= 0 && X < pl.W && Y >= 0 && Y < pl.H;
        acc += (int) pl.p[ok ? Y * pl.W + X : pl.zero];
      }
    }
    unsigned long long key = 0;
    if (holds) {
      top[((long long) scan * A.nt + jj) * NB + q] = acc;
      key = ((unsigned long long) (unsigned) acc << 32) | (unsigned long long) (0x7fffffffu - (unsigned) ((long long) jj * NB + q));
    }
    const unsigned long long m = block_max(key, red);
    if (t == 0 && m) atomicMax(&seeds[scan], m);
  }
}

__global__ __launch_bounds__(256) void k_prune_seed(MatchArgs A, Plane field, int L, int nbx, int nby, long long tiles, int parts,
                                                    const int2* __restrict__ cells, const unsigned long long* __restrict__ seeds,
                                                    unsigned long long* __restrict__ words, int* __restrict__ aux) {
  __shared__ unsigned long long red[4];
  const int t = threadIdx.x, s = 1 << L, NB = nbx * nby;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int scan = (int) (tile / parts), part = (int) (tile - (long long) scan * parts);
    const int block = (int) (0x7fffffffu - ((unsigned) seeds[scan] & 0x7fffffffu));
    const int jb = block / NB, q = block - jb * NB;
    const int by = q / nbx, bx = q - by * nbx;
    const int i = part * 256 + t;  // a candidate of the seed block; the one behind them is the guess
    long long dxi = (long long) bx * s + (i & (s - 1)), dyi = (long long) by * s + (i >> L);
    int jj = jb;
    if (i == s * s) dxi = A.wx, dyi = A.wy, jj = A.ht;
    unsigned long long key = 0;
    if (i <= s * s && dxi < A.nx && dyi < A.ny) {
      const int score     = sum_under(field, cells + ((long long) scan * A.nt + jj) * A.nb, A.nb, dxi - A.wx, dyi - A.wy);
      const bool is_guess = jj == A.ht && dyi == A.wy && dxi == A.wx;
      if (is_guess) aux[2 * scan] = score;
      key = key_of(score, is_guess, (int) (((long long) jj * A.ny + dyi) * A.nx + dxi));
    }
    const unsigned long long m = block_max(key, red);
    if (t == 0 && m) atomicMax(&words[scan], m);
  }
}

// the children inside the window of the workgroup's surviving blocks go to the scan's next list: ONE atomicAdd per workgroup
// reserves their room (and one counts the survivors); what lies past the segment's end is counted, not written.  Every thread of
// the workgroup calls; sh: 9 ints of LDS.
__device__ __forceinline__ void emit_children(bool alive, int jj, int by, int bx, int half, int cnbx, int cnby, const MatchArgs& A, int cap,
                                              int* __restrict__ count, int* __restrict__ survivors, int* __restrict__ out, int* sh) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int kx = alive ? 1 + ((2LL * bx + 1) * half < A.nx ? 1 : 0) : 0, ky = alive ? 1 + ((2LL * by + 1) * half < A.ny ? 1 : 0) : 0;
  const int c  = kx * ky;
  int inc      = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  const unsigned long long mask = __ballot(alive);
  if (lane == 63) sh[w] = inc;
  if (lane == 0) sh[4 + w] = __popcll(mask);
  __syncthreads();
  if (t == 0) {
    const int total = sh[0] + sh[1] + sh[2] + sh[3], ns = sh[4] + sh[5] + sh[6] + sh[7];
    sh[8] = total ? atomicAdd(count, total) : 0;
    if (ns) atomicAdd(survivors, ns);
  }
  __syncthreads();
  long long at = (long long) sh[8] + inc - c;
  for (int u = 0; u < w; ++u) at += sh[u];
  for (int b = 0; b < ky; ++b)
    for (int a = 0; a < kx; ++a, ++at)
      if (at < cap) out[at] = (int) (((long long) jj * cnby + 2 * by + b) * cnbx + 2 * bx + a);
  __syncthreads();  // (sh is the next round's too)
}

// the workgroup's first chunk of a scan's entries: turned by the scan, so that short lists of many scans spread over the launch
__device__ __forceinline__ long long first_chunk(int scan) {
  return (long long) ((blockIdx.x + gridDim.x - (unsigned) scan % gridDim.x) % gridDim.x) * 256;
}

__global__ __launch_bounds__(256) void k_prune_expand_top(MatchArgs A, int L, int nbx, int nby, int cnbx, int cnby, int cap,
                                                          const int* __restrict__ top, const unsigned long long* __restrict__ seeds,
                                                          const unsigned long long* __restrict__ words, const int* __restrict__ aux,
                                                          int* __restrict__ state, int* __restrict__ lists) {
  __shared__ int sh[9];
  const int t = threadIdx.x, NB = nbx * nby;
  const long long n = (long long) A.nt * NB;
  for (int scan = 0; scan < A.K; ++scan) {
    int* const st     = state + (long long) scan * STATE_INTS;
    const int floor   = (int) (words[scan] >> 32);
    const bool strict = floor == aux[2 * scan];
    const long long c1 = first_chunk(scan);
    if (c1 == 0 && t == 0)
      st[ST_FLOOR] = floor, st[ST_STRICT] = strict, st[ST_SEED] = (int) (0x7fffffffu - ((unsigned) seeds[scan] & 0x7fffffffu));
    for (long long c0 = c1; c0 < n; c0 += (long long) gridDim.x * 256) {
      const long long i = c0 + t;
      bool alive = false;
      int jj = 0, by = 0, bx = 0;
      if (i < n) {
        const int U = top[scan * n + i];
        jj = (int) (i / NB);
        const int q = (int) (i - (long long) jj * NB);
        by = q / nbx, bx = q - by * nbx;
        alive = strict ? U > floor : U >= floor;
      }
      emit_children(alive, jj, by, bx, 1 << (L - 1), cnbx, cnby, A, cap, st + ST_COUNT + L - 1, st + ST_SURV + L,
                    lists + ((long long) ((L - 1) & 1) * A.K + scan) * cap, sh);
    }
  }
}

__global__ __launch_bounds__(256) void k_prune_level(MatchArgs A, Plane pl, int l, int nbx, int nby, int cnbx, int cnby, int limit, int cap,
                                                     const int2* __restrict__ cells, int* __restrict__ state, int* __restrict__ lists) {
  __shared__ int sh[9];
  const int t = threadIdx.x;
  for (int scan = 0; scan < A.K; ++scan) {
    int* const st = state + (long long) scan * STATE_INTS;
    const int n   = st[ST_COUNT + l];
    if (n == 0 || n > limit) continue;  // (over the limit: the scan falls back)
    const int floor = st[ST_FLOOR];
    const bool strict = st[ST_STRICT] != 0;
    const int* const in = lists + ((long long) (l & 1) * A.K + scan) * cap;
    for (long long c0 = first_chunk(scan); c0 < n; c0 += (long long) gridDim.x * 256) {
      const long long i = c0 + t;
      bool alive = false;
      int jj = 0, by = 0, bx = 0;
      if (i < n) {
        const int flat = in[i];
        const int rest = flat / nbx;
        bx = flat - rest * nbx, jj = rest / nby, by = rest - jj * nby;
        const int U = sum_under(pl, cells + ((long long) scan * A.nt + jj) * A.nb, A.nb, (long long) bx * pl.s - A.wx + pl.s - 1,
                                (long long) by * pl.s - A.wy + pl.s - 1);
        alive = strict ? U > floor : U >= floor;
      }
      emit_children(alive, jj, by, bx, pl.s >> 1, cnbx, cnby, A, cap, st + ST_COUNT + l - 1, st + ST_SURV + l,
                    lists + ((long long) ((l - 1) & 1) * A.K + scan) * cap, sh);
    }
  }
}

__global__ __launch_bounds__(256) void k_prune_exact(MatchArgs A, Plane field, int limit, int cap, const int2* __restrict__ cells,
                                                     const int* __restrict__ state, const int* __restrict__ lists,
                                                     unsigned long long* __restrict__ words) {
  __shared__ unsigned long long red[4];
  const int t = threadIdx.x;
  for (int scan = 0; scan < A.K; ++scan) {
    const int n = state[(long long) scan * STATE_INTS + ST_COUNT];
    if (n == 0 || n > limit) continue;
    const int* const in = lists + (long long) scan * cap;
    unsigned long long key = 0;
    for (long long i = first_chunk(scan) + t; i < n; i += (long long) gridDim.x * 256) {
      const int flat = in[i];
      const int dxi = flat % A.nx, rest = flat / A.nx;
      const int dyi = rest % A.ny, jj = rest / A.ny;
      const int score = sum_under(field, cells + ((long long) scan * A.nt + jj) * A.nb, A.nb, (long long) dxi - A.wx, (long long) dyi - A.wy);
      key = max(key, key_of(score, jj == A.ht && dyi == A.wy && dxi == A.wx, flat));
    }
    const unsigned long long m = block_max(key, red);
    if (t == 0 && m) atomicMax(&words[scan], m);
  }
}

__device__ __forceinline__ bool fell_back(const int* st, int L, int limit) {
  bool fell = false;
  for (int l = 0; l < L; ++l) fell |= st[ST_COUNT + l] > limit;
  return fell;
}

__global__ __launch_bounds__(256) void k_prune_fallback(MatchArgs A, Plane field, int L, int limit, const int2* __restrict__ cells,
                                                        const int* __restrict__ state, unsigned long long* __restrict__ words) {
  __shared__ unsigned long long red[4];
  for (int scan = 0; scan < A.K; ++scan) {
    if (!fell_back(state + (long long) scan * STATE_INTS, L, limit)) continue;
    unsigned long long key = 0;
    for (long long i = (long long) blockIdx.x * 256 + threadIdx.x; i < A.nc; i += (long long) gridDim.x * 256) {
      const int flat = (int) i;
      const int dxi = flat % A.nx, rest = flat / A.nx;
      const int dyi = rest % A.ny, jj = rest / A.ny;
      const int score = sum_under(field, cells + ((long long) scan * A.nt + jj) * A.nb, A.nb, (long long) dxi - A.wx, (long long) dyi - A.wy);
      key = max(key, key_of(score, jj == A.ht && dyi == A.wy && dxi == A.wx, flat));
    }
    const unsigned long long m = block_max(key, red);
    if (threadIdx.x == 0 && m) atomicMax(&words[scan], m);
  }
}

__global__ __launch_bounds__(256) void k_prune_stats(MatchArgs A, int L, int limit, int top_blocks, const int* __restrict__ state,
                                                     srrg2_gridmap_prune_stats* __restrict__ out) {
  const int scan = blockIdx.x * 256 + threadIdx.x;
  if (scan >= A.K) return;
  const int* const st = state + (long long) scan * STATE_INTS;
  srrg2_gridmap_prune_stats* const o = out + scan;
  int over = -1;  // the highest level whose list overflowed
  for (int l = L - 1; l >= 0 && over < 0; --l)
    if (st[ST_COUNT + l] > limit) over = l;
  o->num_candidates = A.nc;
  for (int l = 0; l <= MAX_LEVELS; ++l) {
    o->num_evaluated[l] = l == L ? top_blocks : (l < L && l > over ? st[ST_COUNT + l] : 0);
    o->num_survivors[l] = l >= 1 && l <= L && l > over ? st[ST_SURV + l] : 0;
  }
  if (over >= 0) o->num_evaluated[0] = A.nc;
  o->floor_score = st[ST_FLOOR], o->seed_block = st[ST_SEED], o->fell_back = over >= 0;
}

int check_levels(const std::string& who, int num_levels) {
  if (num_levels < 1 || num_levels > MAX_LEVELS) return fail(SRRG2_E_INVALID, who + "num_levels 1 .. 6");
  return 0;
}

// level l of the planes as they are built (0: the field)
Plane plane_of(const srrg2_gridmap_s* h, int l) {
  Plane pl;
  pl.s = 1 << l, pl.W = h->p.cols + pl.s - 1, pl.H = h->p.rows + pl.s - 1;
  pl.p    = l == 0 ? h->field.p : h->bounds.p + h->bounds_at[l];
  pl.zero = l == 0 ? h->cells() : h->bounds_at[0] - h->bounds_at[l];
  return pl;
}

}  // namespace

extern "C" void srrg2_gridmap_default_prune_params(srrg2_gridmap_prune_params* p) {
  if (!p) return;
  p->num_levels = 4, p->max_list_entries = 0;
}

extern "C" int srrg2_gridmap_build_bounds(srrg2_gridmap_h h, int num_levels) {
  const std::string who = "gridmap_build_bounds: ";
  int rc;
  if ((rc = check_levels(who, num_levels)) || (rc = srrg2amd::gridmap_ready(who, h)) || (rc = fresh(who, h))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st   = h->stream();
  h->bounds_levels = 0;
  long long at = 0;
  for (int l = 1; l <= num_levels; ++l) {
    h->bounds_at[l] = at;
    at += (long long) (h->p.rows + (1 << l) - 1) * (h->p.cols + (1 << l) - 1);
  }
  h->bounds_at[0] = at;  // the zero byte
  if ((rc = h->bounds.reserve((size_t) at + 1))) return rc;
  HIP_TRY(hipMemsetAsync(h->bounds.p + at, 0, 1, st));
  for (int l = 1; l <= num_levels; ++l) {
    const int half = 1 << (l - 1);
    const int pw = h->p.cols + half - 1, ph = h->p.rows + half - 1, ow = h->p.cols + 2 * half - 1, oh = h->p.rows + 2 * half - 1;
    const int blocks = (int) std::min<long long>(((long long) ow * oh + 255) / 256, BOUNDS_BLOCKS);
    hipLaunchKernelGGL(k_bounds_build, dim3(blocks), dim3(256), 0, st, l == 1 ? h->field.p : h->bounds.p + h->bounds_at[l - 1], pw, ph,
                       h->bounds.p + h->bounds_at[l], ow, oh, half);
    HIP_TRY(hipGetLastError());
  }
  h->bounds_levels = num_levels;
  return 0;
}

extern "C" int srrg2_gridmap_get_bounds(srrg2_gridmap_h h, int level, uint8_t* dst, int row_stride_bytes, int mem) {
  const std::string who = "gridmap_get_bounds: ";
  if (mem != SRRG2_MEM_HOST && mem != SRRG2_MEM_DEVICE) return fail(SRRG2_E_INVALID, who + "bad mem");
  if (level < 1 || level > MAX_LEVELS) return fail(SRRG2_E_INVALID, who + "level 1 .. 6");
  int rc;
  if ((rc = srrg2amd::gridmap_ready(who, h)) || (rc = fresh(who, h))) return rc;
  if (h->bounds_levels == 0) return fail(SRRG2_E_INVALID, who + "the bound planes are stale or were never built (srrg2_gridmap_build_bounds)");
  if (level > h->bounds_levels) return fail(SRRG2_E_INVALID, who + "level above the number of levels built");
  const Plane pl = plane_of(h, level);
  if (!dst) return fail(SRRG2_E_INVALID, who + "null image");
  if (row_stride_bytes < pl.W) return fail(SRRG2_E_INVALID, who + "row stride smaller than a row");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t) row_stride_bytes, pl.p, (size_t) pl.W, (size_t) pl.W, (size_t) pl.H,
                           mem == SRRG2_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream()));
  HIP_TRY(hipStreamSynchronize(h->stream()));
  h->upload_pending = false;
  return 0;
}

extern "C" int srrg2_gridmap_match_scans_pruned(srrg2_gridmap_h h, const float* ranges, int num_scans, const float* guess_robot_in_world,
                                                int mem, const srrg2_gridmap_scan_params* p, const srrg2_gridmap_match_params* mp,
                                                const srrg2_gridmap_prune_params* pp, srrg2_gridmap_match_result* results,
                                                srrg2_gridmap_prune_stats* stats) {
  const std::string who = "gridmap_match_scans_pruned: ";
  int rc;
  if ((rc = check_match_call(who, ranges, num_scans, guess_robot_in_world, mem, p, mp, results))) return rc;
  if (!pp) return fail(SRRG2_E_INVALID, who + "null prune params");
  if ((rc = check_levels(who, pp->num_levels))) return rc;
  if (pp->max_list_entries < 0) return fail(SRRG2_E_INVALID, who + "max_list_entries >= 0");
  if ((rc = check_match_sizes(who, mp)) || (rc = check_match_cells(who, num_scans, p, mp))) return rc;
  if ((rc = srrg2amd::gridmap_ready(who, h))) return rc;
  if (!(p->range_max / h->p.resolution <= GRIDMAP_MAX_STEPS)) return fail(SRRG2_E_INVALID, who + "range_max / resolution beyond 32000 cells");
  if ((rc = fresh(who, h))) return rc;
  if (h->bounds_levels == 0) return fail(SRRG2_E_INVALID, who + "the bound planes are stale or were never built (srrg2_gridmap_build_bounds)");
  if (pp->num_levels > h->bounds_levels) return fail(SRRG2_E_INVALID, who + "num_levels above the number of levels built");
  if (num_scans == 0) return 0;
  const int K = num_scans, L = pp->num_levels;
  const int limit = pp->max_list_entries > 0 ? pp->max_list_entries : DEFAULT_LIST_ENTRIES;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream();
  MatchArgs A;
  if ((rc = stage_match(h, ranges, K, guess_robot_in_world, mem, p, mp, A))) return rc;
  int nbx[MAX_LEVELS + 1], nby[MAX_LEVELS + 1];
  for (int l = 0; l <= L; ++l) nbx[l] = (int) (((long long) A.nx + (1 << l) - 1) >> l), nby[l] = (int) (((long long) A.ny + (1 << l) - 1) >> l);
  const long long prep_total = (long long) K * A.nb * A.nt;
  const long long top_blocks = (long long) A.nt * nbx[L] * nby[L];  // per scan (<= the candidates)
  const int cap              = std::min(limit, A.nc);                // entries of a scan's list
  if ((rc = h->match_cells.reserve((size_t) prep_total + 1)) || (rc = h->match_words.reserve(3 * (size_t) K)) ||
      (rc = h->match_results.reserve((size_t) K)) || (rc = h->match_results_host.reserve((size_t) K, (size_t) K / 8)) ||
      (rc = h->prune_top.reserve((size_t) top_blocks * K)) || (rc = h->prune_lists.reserve(2 * (size_t) K * cap)) ||
      (rc = h->prune_state.reserve((size_t) K * STATE_INTS)) || (rc = h->prune_stats.reserve((size_t) K)) ||
      (rc = h->prune_stats_host.reserve((size_t) K, (size_t) K / 8)))
    return rc;
  unsigned long long* const words = h->match_words.p;
  int* const aux                  = reinterpret_cast<int*>(words + K);
  unsigned long long* const seeds = words + 2 * (size_t) K;
  HIP_TRY(hipMemsetAsync(words, 0, 3 * (size_t) K * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(h->prune_state.p, 0, (size_t) K * STATE_INTS * sizeof(int), st));
  if (prep_total > 0) {
    const int blocks = (int) std::min<long long>((prep_total + 255) / 256, MAX_PREP_BLOCKS);
    hipLaunchKernelGGL(k_match_prep, dim3(blocks), dim3(256), 0, st, A, prep_total, h->match_cells.p, aux);
    HIP_TRY(hipGetLastError());
  }
  const Plane field = plane_of(h, 0);
  {
    const int chunks      = (int) (((long long) nbx[L] * nby[L] + 255) / 256);
    const long long tiles = (long long) K * A.nt * chunks;
    hipLaunchKernelGGL(k_prune_top, dim3((int) std::min<long long>(tiles, TOP_BLOCKS)), dim3(256), 0, st, A, plane_of(h, L), nbx[L], nby[L], tiles,
                       chunks, h->match_cells.p, h->prune_top.p, seeds);
    HIP_TRY(hipGetLastError());
  }
  {
    const int parts       = ((1 << (2 * L)) + 1 + 255) / 256;
    const long long tiles = (long long) K * parts;
    hipLaunchKernelGGL(k_prune_seed, dim3((int) std::min<long long>(tiles, SEED_BLOCKS)), dim3(256), 0, st, A, field, L, nbx[L], nby[L], tiles,
                       parts, h->match_cells.p, seeds, words, aux);
    HIP_TRY(hipGetLastError());
  }
  {
    const long long chunks = (top_blocks + 255) / 256;
    hipLaunchKernelGGL(k_prune_expand_top, dim3((int) std::min<long long>(chunks, EXPAND_BLOCKS)), dim3(256), 0, st, A, L, nbx[L], nby[L],
                       nbx[L - 1], nby[L - 1], cap, h->prune_top.p, seeds, words, aux, h->prune_state.p, h->prune_lists.p);
    HIP_TRY(hipGetLastError());
  }
  // (a list holds at most `cap` entries: the launches below are sized for that and stride over what the counters say)
  const int list_blocks = std::min((cap + 255) / 256, (int) LIST_BLOCKS);
  for (int l = L - 1; l >= 1; --l) {
    hipLaunchKernelGGL(k_prune_level, dim3(list_blocks), dim3(256), 0, st, A, plane_of(h, l), l, nbx[l], nby[l], nbx[l - 1], nby[l - 1], limit, cap,
                       h->match_cells.p, h->prune_state.p, h->prune_lists.p);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_prune_exact, dim3(list_blocks), dim3(256), 0, st, A, field, limit, cap, h->match_cells.p, h->prune_state.p,
                     h->prune_lists.p, words);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_prune_fallback, dim3((int) std::min<long long>(((long long) A.nc + 255) / 256, FALLBACK_BLOCKS)), dim3(256), 0, st, A, field,
                     L, limit, h->match_cells.p, h->prune_state.p, words);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_match_finish, dim3((K + 255) / 256), dim3(256), 0, st, A, words, aux, h->match_results.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_prune_stats, dim3((K + 255) / 256), dim3(256), 0, st, A, L, limit, (int) top_blocks, h->prune_state.p, h->prune_stats.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->match_results_host.p, h->match_results.p, (size_t) K * sizeof(srrg2_gridmap_match_result), hipMemcpyDeviceToHost, st));
  if (stats) HIP_TRY(hipMemcpyAsync(h->prune_stats_host.p, h->prune_stats.p, (size_t) K * sizeof(srrg2_gridmap_prune_stats), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait
  h->upload_pending = false;
  std::memcpy(results, h->match_results_host.p, (size_t) K * sizeof(srrg2_gridmap_match_result));
  if (stats) std::memcpy(stats, h->prune_stats_host.p, (size_t) K * sizeof(srrg2_gridmap_prune_stats));
  return 0;
}
