// scan_beam.h -- the sensor-frame point of one beam of a planar laser scan: what the scan adaptor (adaptor.hip) writes and the
// occupancy grid (gridmap.hip) traces towards.  ONE expression, so both give the same bits (DESIGN.md section 4 "Measurement
// adaptors", "Occupancy grid"; tests/adaptor_restatement.py restates it).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include "det_math.h"

namespace {

// bearing amin + k * ainc in float64, its sine / cosine by dm::sincos, rounded to float32, times the range
__device__ __forceinline__ float2 scan_beam_point(double amin, double ainc, int k, float r) {
  double s, c;
  dm::sincos(amin + (double) k * ainc, s, c);
  const float cf = (float) c, sf = (float) s;
  return make_float2(cf * r, sf * r);
}

}  // namespace
