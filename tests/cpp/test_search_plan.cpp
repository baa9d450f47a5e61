// The launch plan of the list-search pass (srrg2_slam_interfaces_amd/csrc/search_plan.h) on the host: plain C++, no device.
// Built and run by tests/test_search_plan_cpp.py (with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>

#include "../../srrg2_slam_interfaces_amd/csrc/search_plan.h"

using srrg2amd::SearchTiles;
using srrg2amd::plan_search_tiles;

static int failures = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      ++failures;                                        \
      std::printf("FAILED %s: ", #cond);                 \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
    }                                                    \
  } while (0)

// a4 + a2 + a1 tiles in class order cover n points, every tile holds a point and only the last one may be partly filled
static bool valid(long long n, long long a4, long long a2, long long a1) {
  if (a4 < 0 || a2 < 0 || a1 < 0) return false;
  const long long room = 64 * a4 + 128 * a2 + 256 * a1;
  if (a4 + a2 + a1 == 0) return n == 0;
  const long long last = a1 ? 256 : a2 ? 128 : 64;
  return room >= n && room - last < n;
}

int main() {
  const int nms[]        = {0, 1, 63, 64, 65, 1000, 81920, 81921, 100000, 4200000};
  const int Ks[]         = {1, 3, 4};
  const long long caps[] = {1, 6, 1280, 1536, 1000000};
  const int lanes[]      = {4, 2, 1};
  int cases = 0;
  for (int n : nms)
    for (int K : Ks)
      for (long long cap : caps)
        for (int lc : lanes) {
          ++cases;
          const SearchTiles p = plan_search_tiles(n, K, cap, lc);
          const long long T1  = (n + 255ll) / 256;
          const long long W   = p.tiles();
#define WFMT "n %d K %d capacity %lld lanes %d -> %d + %d + %d"
#define WARGS n, K, cap, lc, p.t4, p.t2, p.t1
#define WHERE WFMT, WARGS
          CHECK(p.t4 >= 0 && p.t2 >= 0 && p.t1 >= 0, WHERE);
          // the tiles cover the cloud exactly once, only the last one partly: walk them
          long long next = 0;
          for (int t = 0; t < W; ++t) {
            const long long size = t < p.t4 ? 64 : t < p.t4 + p.t2 ? 128 : 256;
            if (p.first_point(t) != next) {
              CHECK(false, "tile %d starts at %lld, not %lld; " WFMT, t, p.first_point(t), next, WARGS);
              break;
            }
            CHECK(next < n, "tile %d is empty; " WFMT, t, WARGS);
            if (t + 1 < W) CHECK(next + size <= n, "tile %d is not the last and not full; " WFMT, t, WARGS);
            next += size;
          }
          CHECK(next >= n, WHERE);
          CHECK(valid(n, p.t4, p.t2, p.t1), WHERE);
          // the ceiling on the lanes per point
          if (lc < 4) CHECK(p.t4 == 0, WHERE);
          if (lc < 2) CHECK(p.t2 == 0, WHERE);
          if (K * T1 > cap || lc == 1) {
            // the fallback is the one-lane layout (in rounds when it exceeds the capacity)
            CHECK(p.t4 == 0 && p.t2 == 0 && p.t1 == T1, WHERE);
            continue;
          }
          CHECK(K * W <= cap, WHERE);  // within the capacity whenever the one-lane layout is
          // no other split of the same number of workgroups gives more points the higher lane count: none with more four-lane
          // tiles, and none with as many four-lane tiles and more two-lane tiles
          if (lc >= 4)
            for (long long a2 = 0; a2 + p.t4 + 1 <= W; ++a2)
              CHECK(!valid(n, p.t4 + 1, a2, W - p.t4 - 1 - a2), "%lld two-lane tiles next to one more four-lane tile; " WFMT, a2, WARGS);
          for (long long a2 = p.t2 + 1; a2 + p.t4 <= W; ++a2)
            CHECK(!valid(n, p.t4, a2, W - p.t4 - a2), "%lld two-lane tiles; " WFMT, a2, WARGS);
          // ... and no more workgroups within the capacity would: either everything already has the most lanes, or one more
          // workgroup does not fit
          if (!(lc >= 4 ? p.t2 + p.t1 == 0 : p.t1 == 0)) CHECK(K * (W + 1) > cap, WHERE);
          if (W <= 48) {  // small plans: every split of W tiles
            for (long long a4 = 0; a4 <= (lc >= 4 ? W : 0); ++a4)
              for (long long a2 = 0; a4 + a2 <= W; ++a2)
                if (valid(n, a4, a2, W - a4 - a2))
                  CHECK(a4 < p.t4 || (a4 == p.t4 && a2 <= p.t2), "%lld + %lld + %lld is better; " WFMT, a4, a2, W - a4 - a2, WARGS);
          }
        }
  // the worked example of the knob's documentation: 1000 points on six workgroups
  {
    const SearchTiles p = plan_search_tiles(1000, 1, 6, 4);
    CHECK(p.t4 == 2 && p.t2 == 1 && p.t1 == 3, "%d + %d + %d", p.t4, p.t2, p.t1);
    const SearchTiles q = plan_search_tiles(100000, 1, 1279, 4);  // (a 100 k-point first pass on 256 x 5 workgroups, one for the prologue)
    CHECK(q.tiles() <= 1279 && q.t4 > 0, "%d + %d + %d", q.t4, q.t2, q.t1);
    std::printf("100000 points on 1279 workgroups: %d + %d + %d tiles\n", q.t4, q.t2, q.t1);
  }
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("%d plans PASSED\n", cases);
  return 0;
}
