// search_plan.h -- how the list-search pass of a launch of up to four alignments is laid out on the chip (plain C++: no HIP).
//
// A single alignment's search pass is a chain of dependent round trips on a half-empty chip, so several lanes per moving point
// shorten it (kernels.hip: cnl_search's TEAM) -- but a workgroup of 256 threads then holds 64 or 128 points instead of 256, and
// a launch of more workgroups than the chip holds at once runs the whole chain a second time for the left-over ones: 1564
// workgroups against 1280 resident ones cost the first pass of a 100 k-point cloud a quarter of its time.  The plan deals the
// points over three classes of tiles so that the launch fits the workgroups that are resident together:
//   tiles [0, t4)             64 points at four lanes each,
//   tiles [t4, t4 + t2)      128 points at two lanes each,
//   tiles [t4 + t2, .. + t1) 256 points at one lane each,
// every tile full but the last one, and as many points as the capacity allows at the higher lane counts (four first).
#pragma once

namespace srrg2amd {

struct SearchTiles {
  int t4, t2, t1;
  int tiles() const { return t4 + t2 + t1; }
  // first moving point of a tile (the kernels compute the same from t4 and t2: TilePlan)
  long long first_point(int tile) const {
    if (tile < t4) return 64ll * tile;
    if (tile < t4 + t2) return 64ll * t4 + 128ll * (tile - t4);
    return 64ll * t4 + 128ll * t2 + 256ll * (tile - t4 - t2);
  }
};

// max_nm       : points of the largest cloud of the launch
// K            : alignments of the launch (every one gets the same tiles)
// capacity_wgs : workgroups that are resident together, less the ones of the launch that hold no tile (the prologue's)
// lanes_cap    : most lanes per point (4, 2 or 1)
// K * tiles() <= capacity_wgs whenever one lane per point fits; otherwise the one-lane layout, which then runs in rounds.
inline SearchTiles plan_search_tiles(int max_nm, int K, long long capacity_wgs, int lanes_cap) {
  const long long n  = max_nm > 0 ? max_nm : 0;
  const long long T1 = (n + 255) / 256;
  SearchTiles one{0, 0, (int) T1};
  if (n == 0 || K <= 0 || lanes_cap < 2) return one;
  const long long T = capacity_wgs / K;  // tiles per alignment
  if (T1 > T) return one;
  SearchTiles p{0, 0, 0};
  long long left = n, tiles = T;
  if (lanes_cap >= 4) {
    if ((n + 63) / 64 <= T) return SearchTiles{(int) ((n + 63) / 64), 0, 0};
    // the most four-lane tiles that leave the rest within 256 points per remaining tile: left - 64 t <= 256 (tiles - t)
    long long t = (256 * tiles - left) / 192;
    if (t > left / 64) t = left / 64;
    p.t4 = (int) t;
    left -= 64 * t;
    tiles -= t;
  }
  if ((left + 127) / 128 <= tiles) {
    p.t2 = (int) ((left + 127) / 128);
    return p;
  }
  long long t = (256 * tiles - left) / 128;  // left - 128 t <= 256 (tiles - t)
  if (t > left / 128) t = left / 128;
  p.t2 = (int) t;
  left -= 128 * t;
  p.t1 = (int) ((left + 255) / 256);
  return p;
}

}  // namespace srrg2amd
