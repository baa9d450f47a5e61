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

// steps 1-7 of the contract for a point with finite coordinates: pixel = row * cols + col in [0, rows * cols), or -1 when the
// point is outside the range interval or the image.  rho is written whenever the range was computed.
DM_HD int project(const Geom& G, float x, float y, float z, float& rho) {
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
  const double h   = sqrt(xd * xd + yd * yd);
  const double eps = dm::atan2((double) z, h);
  const double rf  = (eps - G.el_min) / G.el_inc + 0.5;
  if (!(rf >= 0.0) || !(rf < (double) G.rows)) return -1;
  return (int) floor(rf) * G.cols + (int) floor(cf);
}

constexpr double TWO_PI  = 6.283185307179586;
constexpr double HALF_PI = 1.5707963267948966;
constexpr double SLACK   = 0x1p-20;  // admits increments that went through float32 on their way here (as the scan clipper's)

// nullptr when the model is usable, else what is wrong with it
inline const char* invalid(const srrg2_spherical_model& m) {
  if (m.rows <= 0 || m.cols <= 0 || (long long) m.rows * (long long) m.cols > 0x7fffffffLL)
    return "rows, cols > 0 and rows*cols within int32";
  if (!std::isfinite(m.azimuth_increment) || m.azimuth_increment == 0.0 || !std::isfinite(m.elevation_increment) ||
      m.elevation_increment == 0.0)
    return "azimuth_increment and elevation_increment must be finite and non-zero";
  if (!std::isfinite(m.azimuth_min) || std::fabs(m.azimuth_min) > TWO_PI) return "azimuth_min must be finite and within [-2 pi, 2 pi]";
  const double inc = std::fabs(m.azimuth_increment);
  if (inc * (double) m.cols > (TWO_PI + inc) * (1.0 + SLACK)) return "|azimuth_increment| * cols beyond 2 pi plus one increment";
  const double last = m.elevation_min + (double) (m.rows - 1) * m.elevation_increment;
  const double lim  = HALF_PI * (1.0 + SLACK);
  if (!std::isfinite(m.elevation_min) || !(std::fabs(m.elevation_min) <= lim) || !(std::fabs(last) <= lim))
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

}  // namespace sph
