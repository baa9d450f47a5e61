// consensus_math.h -- the sampler and the two minimal solvers of srrg2_consensus_compute (plain C++: no HIP).  DESIGN.md section 4
// "Consensus pose" is the contract and tests/consensus_restatement.py its executable form; every operation below is written in
// the contract's order and the library is compiled with -ffp-contract=off, so a host compiler, the device compiler and the
// restatement give the same bits (tests/test_consensus_cpp.py compiles this header with g++ and compares them).
// Only + - * / sqrt on IEEE doubles.  CM_HD: the one host/device macro; a host compiler that reads this header needs no HIP include.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef CM_HD
#ifdef __HIPCC__
#define CM_HD __host__ __device__ __forceinline__
#else
#define CM_HD inline
#endif
#endif

namespace cm {

enum { HYP_SCORED = 0, HYP_DEGENERATE = 1, HYP_REJECTED = 2 };

CM_HD uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// (finite: x - x is 0 for a finite x and NaN for an infinity or a NaN)
CM_HD bool fin(double x) { return (x - x) == 0.0; }
CM_HD double absd(double x) { return x < 0.0 ? -x : x; }

// The S pair indices of hypothesis h among N pairs; false: the hypothesis is degenerate (N < S, or four attempts at an index
// all met an earlier index of this hypothesis).  The candidate's index is deliberately not in the hash.
template <int S>
CM_HD bool sample(uint32_t seed, uint32_t h, int N, int* idx) {
  if (N < S) return false;
  const uint32_t base = mix32(mix32(seed) + h);
  for (int j = 0; j < S; ++j) {
    bool found = false;
    for (int a = 0; a < 4 && !found; ++a) {
      const uint32_t r = mix32(base + 4u * (uint32_t) j + (uint32_t) a);
      const int i      = (int) (((uint64_t) r * (uint64_t) (uint32_t) N) >> 32);
      bool fresh       = true;
      for (int e = 0; e < j; ++e) fresh = fresh && idx[e] != i;
      if (fresh) {
        idx[j] = i;
        found  = true;
      }
    }
    if (!found) return false;
  }
  return true;
}

struct Frame3 {
  double e1[3], e2[3], e3[3], c[3];
  double d01, d02, d12;  // squared distances of the sample points
};

CM_HD void cross3(const double* a, const double* b, double* n) {
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
}
CM_HD double sq3(const double* a) { return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; }

// the orthonormal frame of a point triple (three floats each); false: too close or collinear against msd2, or not finite
CM_HD bool frame3(const float* p0, const float* p1, const float* p2, double msd2, Frame3& F) {
  double a[3], b[3], c[3], n[3];
  for (int i = 0; i < 3; ++i) {
    a[i] = (double) p1[i] - (double) p0[i];
    b[i] = (double) p2[i] - (double) p0[i];
    c[i] = (double) p2[i] - (double) p1[i];
  }
  cross3(a, b, n);
  const double la = sq3(a), ln = sq3(n);
  F.d01 = la, F.d02 = sq3(b), F.d12 = sq3(c);
  if (!fin(la) || !fin(ln) || la < msd2 || ln < msd2 * la) return false;
  const double ra = sqrt(la), rn = sqrt(ln);
  for (int i = 0; i < 3; ++i) {
    F.e1[i] = a[i] / ra;
    F.e3[i] = n[i] / rn;
  }
  cross3(F.e3, F.e1, F.e2);
  for (int i = 0; i < 3; ++i) F.c[i] = (((double) p0[i] + (double) p1[i]) + (double) p2[i]) / 3.0;
  return true;
}

CM_HD bool length_differs(double d2m, double d2f, double tau) { return absd(sqrt(d2m) - sqrt(d2f)) > 2.0 * tau; }

// dim 3: moving triple m0 m1 m2 -> fixed triple f0 f1 f2.  X: row-major 3 x 4, float64.
CM_HD int solve3(const float* m0, const float* m1, const float* m2, const float* f0, const float* f1, const float* f2, double msd2,
                 double tau, int length_check, double* X) {
  Frame3 M, F;
  const bool okm = frame3(m0, m1, m2, msd2, M);
  const bool okf = frame3(f0, f1, f2, msd2, F);
  if (!okm || !okf) return HYP_DEGENERATE;
  if (length_check && (length_differs(M.d01, F.d01, tau) || length_differs(M.d02, F.d02, tau) || length_differs(M.d12, F.d12, tau)))
    return HYP_REJECTED;
  bool finite = true;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) X[i * 4 + j] = (F.e1[i] * M.e1[j] + F.e2[i] * M.e2[j]) + F.e3[i] * M.e3[j];
    X[i * 4 + 3] = F.c[i] - ((X[i * 4 + 0] * M.c[0] + X[i * 4 + 1] * M.c[1]) + X[i * 4 + 2] * M.c[2]);
    for (int j = 0; j < 4; ++j) finite = finite && fin(X[i * 4 + j]);
  }
  return finite ? HYP_SCORED : HYP_DEGENERATE;
}

// dim 2: moving pair m0 m1 -> fixed pair f0 f1 (two floats each).  X: row-major 3 x 3, float64.
CM_HD int solve2(const float* m0, const float* m1, const float* f0, const float* f1, double msd2, double tau, int length_check,
                 double* X) {
  const double a0 = (double) m1[0] - (double) m0[0], a1 = (double) m1[1] - (double) m0[1];
  const double A0 = (double) f1[0] - (double) f0[0], A1 = (double) f1[1] - (double) f0[1];
  const double la = a0 * a0 + a1 * a1, lA = A0 * A0 + A1 * A1;
  if (!fin(la) || !fin(lA) || la < msd2 || lA < msd2) return HYP_DEGENERATE;
  if (length_check && length_differs(la, lA, tau)) return HYP_REJECTED;
  const double den = sqrt(la) * sqrt(lA);
  const double c = (a0 * A0 + a1 * A1) / den, s = (a0 * A1 - a1 * A0) / den;
  const double cm0 = ((double) m0[0] + (double) m1[0]) * 0.5, cm1 = ((double) m0[1] + (double) m1[1]) * 0.5;
  const double cf0 = ((double) f0[0] + (double) f1[0]) * 0.5, cf1 = ((double) f0[1] + (double) f1[1]) * 0.5;
  X[0] = c, X[1] = -s, X[3] = s, X[4] = c;
  X[2] = cf0 - (X[0] * cm0 + X[1] * cm1);
  X[5] = cf1 - (X[3] * cm0 + X[4] * cm1);
  X[6] = 0.0, X[7] = 0.0, X[8] = 1.0;
  bool finite = true;
  for (int i = 0; i < 6; ++i) finite = finite && fin(X[i]);
  return finite ? HYP_SCORED : HYP_DEGENERATE;
}

}  // namespace cm
