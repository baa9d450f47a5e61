// spherical.h -- the spherical sensor model of a spinning 3-D lidar (srrg2_spherical_model): ONE projection of a sensor-frame
// point to a pixel of the rows x cols range image, shared by the sweep adaptor (adaptor.hip) and the spherical clipper
// (scene.hip), and the model's validation.  DESIGN.md section 4 "Lidar sweeps" is the arithmetic contract: float32 range in the
// written order, both angles by dm::atan2 in float64 (fixed reduction + polynomial: the same bits on host and device), the
// column binned exactly as the scan clipper bins a bearing (scene.hip: sclip_beam), the row without a wrap.
#pragma once
#include <cmath>

#include "../../include/srrg2_slam_amd.h"
#include "det_math.h"

namespace sph {

struct Geom {
  double az_min, az_inc, az_turn;  // az_turn = copysign(2 pi, az_inc)
  double el_min, el_inc;
  float range_min, range_max;
  int rows, cols;
};

// the rows of a sensor with a per-ring elevation table (srrg2_lidar_sweep_extras.ring_elevations, the table of
// srrg2_scene_clip_spherical_rings): the rows + 1 row boundaries, oriented -- B[k] = sigma * b[k] with sigma = -1 for a
// descending table -- so that they ascend either way.  At most 256 rows: the table travels by value in the kernel arguments
// (a host table is consumed by the launch) and every workgroup stages it into LDS once (stage_rings), where the row of a
// point is an 8-step binary search.
constexpr int MAX_RING_ROWS = 256;
struct Rings {
  int rows, descending;
  double B[MAX_RING_ROWS + 1];
};

// steps 1-7 of the contract for a point with finite coordinates: pixel = row * cols + col in [0, rows * cols), or -1 when the
// point is outside the range interval or the image.  rho is written whenever the range was computed, tf (the continuous column
// coordinate of step 3) whenever the pixel is >= 0.  RINGS: the row comes from the boundaries B[0 .. rows] (`descending`: of a
// descending table) instead of the model's uniform rows; G.el_min / G.el_inc are then not read.
template <bool RINGS>
DM_HD int project_t(const Geom& G, const double* B, int descending, float x, float y, float z, float& rho, double& tf) {
  rho = sqrtf((x * x + y * y) + z * z);
  if (!(rho >= G.range_min) || !(rho <= G.range_max)) return -1;
  const double xd = (double) x, yd = (double) y;
  const double alpha = dm::atan2(yd, xd);
  const double d     = alpha - G.az_min;
  double t           = d / G.az_inc;
  if (t < -0.5)
    t = (d + G.az_turn) / G.az_inc;
  else if (t >= (double) G.cols - 0.5)
    t = (d - G.az_turn) / G.az_inc;
  const double cf = t + 0.5;
  if (!(cf >= 0.0) || !(cf < (double) G.cols)) return -1;
  tf = cf;
  const double h   = sqrt(xd * xd + yd * yd);
  const double eps = dm::atan2((double) z, h);
  if (RINGS) {
    const double u = descending ? -eps : eps;
    if (!(u >= B[0]) || !(u < B[G.rows])) return -1;
    int lo = 0, hi = G.rows;  // B[lo] <= u < B[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (B[mid] <= u)
        lo = mid;
      else
        hi = mid;
    }
    return lo * G.cols + (int) floor(cf);
  }
  const double rf = (eps - G.el_min) / G.el_inc + 0.5;
  if (!(rf >= 0.0) || !(rf < (double) G.rows)) return -1;
  return (int) floor(rf) * G.cols + (int) floor(cf);
}

DM_HD int project(const Geom& G, float x, float y, float z, float& rho) {
  double tf;
  return project_t<false>(G, nullptr, 0, x, y, z, rho, tf);
}

#ifdef __HIPCC__
// every thread of the workgroup calls it once, before its first project_t<true>; sB holds MAX_RING_ROWS + 1 doubles
__device__ __forceinline__ void stage_rings(const Rings& T, double* sB) {
  for (int k = threadIdx.x; k <= T.rows; k += blockDim.x) sB[k] = T.B[k];
  __syncthreads();
}
#endif

constexpr double TWO_PI  = 6.283185307179586;
constexpr double HALF_PI = 1.5707963267948966;
constexpr double SLACK   = 0x1p-20;  // admits increments that went through float32 on their way here (as the scan clipper's)

// nullptr when the model is usable, else what is wrong with it
// (with_rings: a ring table replaces the model's rows -- elevation_min / elevation_increment are neither read nor validated)
inline const char* invalid(const srrg2_spherical_model& m, bool with_rings = false) {
  if (m.rows <= 0 || m.cols <= 0 || (long long) m.rows * (long long) m.cols > 0x7fffffffLL)
    return "rows, cols > 0 and rows*cols within int32";
  if (!std::isfinite(m.azimuth_increment) || m.azimuth_increment == 0.0 ||
      (!with_rings && (!std::isfinite(m.elevation_increment) || m.elevation_increment == 0.0)))
    return "azimuth_increment and elevation_increment must be finite and non-zero";
  if (!std::isfinite(m.azimuth_min) || std::fabs(m.azimuth_min) > TWO_PI) return "azimuth_min must be finite and within [-2 pi, 2 pi]";
  const double inc = std::fabs(m.azimuth_increment);
  if (inc * (double) m.cols > (TWO_PI + inc) * (1.0 + SLACK)) return "|azimuth_increment| * cols beyond 2 pi plus one increment";
  const double last = m.elevation_min + (double) (m.rows - 1) * m.elevation_increment;
  const double lim  = HALF_PI * (1.0 + SLACK);
  if (!with_rings && (!std::isfinite(m.elevation_min) || !(std::fabs(m.elevation_min) <= lim) || !(std::fabs(last) <= lim)))
    return "the first and the last row's elevation must lie within [-pi/2, pi/2]";
  if (!(m.range_min > 0.f) || !(m.range_max >= m.range_min)) return "0 < range_min <= range_max";
  return nullptr;
}

// the columns close the circle: column cols - 1 and column 0 are neighbours (the adaptor's normals)
inline bool columns_wrap(const srrg2_spherical_model& m) {
  return std::fabs(std::fabs(m.azimuth_increment) * (double) m.cols - TWO_PI) <= TWO_PI * SLACK;
}

inline Geom geom_of(const srrg2_spherical_model& m) {
  return Geom{m.azimuth_min, m.azimuth_increment, std::copysign(TWO_PI, m.azimuth_increment),
              m.elevation_min, m.elevation_increment, m.range_min, m.range_max, m.rows, m.cols};
}

// the boundaries of a ring table e[0 .. m.rows) (host memory), in float64 in the written order; nullptr when `T` was filled,
// else what is wrong with the table (*unsupported: more rows than travel by value)
inline const char* rings_of(const srrg2_spherical_model& m, const double* e, Rings& T, bool* unsupported) {
  *unsupported = false;
  const int rows = m.rows;
  if (rows < 2) return "a ring table needs rows >= 2";
  if (rows > MAX_RING_ROWS) {
    *unsupported = true;
    return "ring tables of more than 256 rows";
  }
  const double lim = HALF_PI * (1.0 + SLACK);
  for (int k = 0; k < rows; ++k)
    if (!std::isfinite(e[k]) || !(std::fabs(e[k]) <= lim)) return "ring elevations must be finite and within [-pi/2, pi/2]";
  const bool desc = e[1] < e[0];
  for (int k = 1; k < rows; ++k)
    if (desc ? !(e[k] < e[k - 1]) : !(e[k] > e[k - 1])) return "ring elevations must be strictly monotonic";
  T.rows       = rows;
  T.descending = desc ? 1 : 0;
  double b;
  b      = e[0] - (e[1] - e[0]) * 0.5;
  T.B[0] = desc ? -b : b;
  for (int k = 1; k < rows; ++k) {
    b      = (e[k - 1] + e[k]) * 0.5;
    T.B[k] = desc ? -b : b;
  }
  b         = e[rows - 1] + (e[rows - 1] - e[rows - 2]) * 0.5;
  T.B[rows] = desc ? -b : b;
  return nullptr;
}

}  // namespace sph
