// gridmap_state.h -- what the two translation units of the srrg2_gridmap_* family share: the handle (gridmap.hip draws the count
// planes, scan_match.hip builds the likelihood field and its bound planes from them and matches scans against both), the cell coordinate and the
// rendered value of the contract, and the checks both make of a batch of scans.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "host_util.h"
#include "scene_state.h"

struct srrg2_gridmap_s {
  int device = 0;
  // the grid's stream is this scratch scene's: the scene export hands it to scene_compact_into as the source of the compaction
  // (its flags, scan sums and counters are the scratch of that path); it never holds points
  srrg2_scene* work = nullptr;
  hipEvent_t uploaded = nullptr;  // recorded behind the upload out of host_stage: the next call waits for it before it refills
  bool upload_pending = false;
  bool is_set         = false;
  srrg2_gridmap_params p;
  srrg2amd::DevBuf<int> planes;  // hits, then misses: rows*cols words each
  srrg2amd::DevBuf<char> stage;  // a host call's ranges, then its poses
  srrg2amd::PinnedBuf<char> host_stage;
  srrg2amd::DevBuf<unsigned long long> ctr;
  srrg2amd::PinnedBuf<unsigned long long> ctr_host;
  srrg2amd::DevBuf<unsigned char> image;  // a host render's packed rows
  // scan_match.hip: the likelihood field (rows*cols bytes and ONE zero byte behind them, what a lookup outside the grid reads),
  // fresh = built from the planes as they are now; the end cells of a match, its per-scan words and results, its volume
  bool field_fresh = false;
  srrg2amd::DevBuf<unsigned char> field;
  srrg2amd::DevBuf<int2> match_cells;
  srrg2amd::DevBuf<unsigned long long> match_words;
  srrg2amd::DevBuf<srrg2_gridmap_match_result> match_results;
  srrg2amd::PinnedBuf<srrg2_gridmap_match_result> match_results_host;
  srrg2amd::DevBuf<int> match_volume;
  // pruned matching: the bound planes P_1 .. P_bounds_levels one behind the other (P_l: (rows + s - 1) * (cols + s - 1) bytes at
  // bounds_at[l], s = 2^l) and ONE zero byte behind them at bounds_at[0]; bounds_levels = 0: stale or never built -- whatever
  // clears field_fresh clears it too (stale_field()).  The top level's bounds, the two block lists a descent alternates
  // between, the per-scan search state and the statistics
  int bounds_levels = 0;
  long long bounds_at[7] = {0, 0, 0, 0, 0, 0, 0};
  srrg2amd::DevBuf<unsigned char> bounds;
  srrg2amd::DevBuf<int> prune_top;
  srrg2amd::DevBuf<int> prune_lists;
  srrg2amd::DevBuf<int> prune_state;
  srrg2amd::DevBuf<srrg2_gridmap_prune_stats> prune_stats;
  srrg2amd::PinnedBuf<srrg2_gridmap_prune_stats> prune_stats_host;
  void stale_field() { field_fresh = false, bounds_levels = 0; }
  long long cells() const { return (long long) p.rows * p.cols; }
  hipStream_t stream() const { return work->stream; }
  ~srrg2_gridmap_s() {
    (void) hipSetDevice(device);
    if (work) (void) hipStreamSynchronize(work->stream);
    if (uploaded) (void) hipEventDestroy(uploaded);
    if (work) (void) srrg2_scene_destroy(work);
  }
};

#define GRIDMAP_MAX_STEPS 32000.f          /* range_max / resolution beyond this is refused */
#define GRIDMAP_CELL_GUARD 1073741824.f    /* 2^30 */
#define GRIDMAP_MAX_RAY 32767

namespace srrg2amd {

// what srrg2_gridmap_integrate_scans refuses without looking at its handle (gridmap.hip); srrg2_gridmap_match_scans refuses the same
int gridmap_check_scan_call(const std::string& who, const float* ranges, int num_scans, const float* poses, int mem,
                            const srrg2_gridmap_scan_params* p, int weight);
// ... and what both refuse of their handle: null, or no grid yet
int gridmap_ready(const std::string& who, srrg2_gridmap_s* h);

}  // namespace srrg2amd

namespace {

// the cell coordinate of the contract; false: never converted
__device__ __forceinline__ bool cell_of(float x, float o, float res, int& c) {
  const float u = floorf((x - o) / res);
  if (!(u >= -GRIDMAP_CELL_GUARD && u < GRIDMAP_CELL_GUARD)) return false;  // (a NaN fails both)
  c = (int) u;
  return true;
}

// 0 .. 100, or 255 = unknown
__device__ __forceinline__ unsigned cell_value(int h, int m, long long need) {
  if (h < 0 || m < 0) return 255u;
  const unsigned long long n = (unsigned long long) h + (unsigned long long) m;
  if ((long long) n < need) return 255u;  // (need >= 1: n > 0 below)
  return (unsigned) ((100ull * (unsigned long long) h + n / 2) / n);
}

}  // namespace
