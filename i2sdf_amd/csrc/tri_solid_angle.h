// The per-face term, the face moments and the far-field rule of the generalized winding number (include/i2sdf.h, "Winding number"),
// shared by the device kernels of winding.hip and by host code (tests/test_winding_host.py compiles this header with g++), like
// tri_closest.h.
//
// The per-face term is the solid angle of Van Oosterom and Strackee (IEEE Trans. Biomed. Eng. 1983); the far field is orders 0 and 1
// of Barill et al., Fast winding numbers for soups and clouds (SIGGRAPH 2018).  Every operation is ONE fp64 operation on the exact
// images of the fp32 inputs, rounded to nearest, in the order written, none contracted into an FMA; a dot product is
// (x x' + y y') + z z'.  tests/winding_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define I2SDF_WN_HD __host__ __device__ __forceinline__
#else
#define I2SDF_WN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace i2sdf {

constexpr double WN_FOUR_PI = 12.566370614359172;         // 4 * M_PI (the scaling by 4 is exact)
constexpr int WN_RECORD = 16;                             // fp64 values per internal node of the moments table

I2SDF_WN_HD double wn_dot(double x, double y, double z, double a, double b, double c) { return (x * a + y * b) + z * c; }

// The two arguments of atan2 for one face (A, B, C) seen from q: the solid angle is 2 atan2(det, den).
I2SDF_WN_HD void tri_solid_angle_terms(double q0, double q1, double q2, double A0, double A1, double A2, double B0, double B1, double B2,
                                       double C0, double C1, double C2, double& det, double& den) {
  const double a0 = A0 - q0, a1 = A1 - q1, a2 = A2 - q2;
  const double b0 = B0 - q0, b1 = B1 - q1, b2 = B2 - q2;
  const double c0 = C0 - q0, c1 = C1 - q1, c2 = C2 - q2;
  const double la = sqrt(wn_dot(a0, a1, a2, a0, a1, a2));
  const double lb = sqrt(wn_dot(b0, b1, b2, b0, b1, b2));
  const double lc = sqrt(wn_dot(c0, c1, c2, c0, c1, c2));
  const double x0 = b1 * c2 - b2 * c1, x1 = b2 * c0 - b0 * c2, x2 = b0 * c1 - b1 * c0;      // b x c
  det = wn_dot(a0, a1, a2, x0, x1, x2);
  const double ab = wn_dot(a0, a1, a2, b0, b1, b2), bc = wn_dot(b0, b1, b2, c0, c1, c2), ca = wn_dot(c0, c1, c2, a0, a1, a2);
  den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
}

// The solid angle of one face, in (-2 pi, 2 pi]: finite for every finite input, a query on the face included.
I2SDF_WN_HD double tri_solid_angle(double q0, double q1, double q2, double A0, double A1, double A2, double B0, double B1, double B2,
                                   double C0, double C1, double C2) {
  double det, den;
  tri_solid_angle_terms(q0, q1, q2, A0, A1, A2, B0, B1, B2, C0, C1, C2, det, den);
  return 2.0 * atan2(det, den);
}

// The composable moments of one face about the origin o: m[0] = area, m[1..3] = area * centroid, m[4..6] = the area vector
// 1/2 (B - A) x (C - A), m[7 + 3 i + j] = (centroid - o)_i * (area vector)_j.
I2SDF_WN_HD void tri_moments(double A0, double A1, double A2, double B0, double B1, double B2, double C0, double C1, double C2, double o0,
                             double o1, double o2, double m[WN_RECORD]) {
  const double e0 = B0 - A0, e1 = B1 - A1, e2 = B2 - A2;
  const double g0 = C0 - A0, g1 = C1 - A1, g2 = C2 - A2;
  const double n[3] = {(e1 * g2 - e2 * g1) * 0.5, (e2 * g0 - e0 * g2) * 0.5, (e0 * g1 - e1 * g0) * 0.5};
  const double area = sqrt(wn_dot(n[0], n[1], n[2], n[0], n[1], n[2]));
  const double c[3] = {((A0 + B0) + C0) / 3.0, ((A1 + B1) + C1) / 3.0, ((A2 + B2) + C2) / 3.0};
  const double o[3] = {o0, o1, o2};
  m[0] = area;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    m[1 + i] = area * c[i];
    m[4 + i] = n[i];
    const double r = c[i] - o[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) m[7 + 3 * i + j] = r * n[j];
  }
}

// Raw sums (area, S, N0, M about o) -> the record a query reads: t[0..2] = the area-weighted centroid, t[3] = the radius (the largest
// distance from the centroid to a corner of the box [lo, hi]), t[4..6] = N0, t[7 + 3 i + j] = N1_ij about the centroid.
// No area (nothing but degenerate or rejected faces below): radius +inf, so the node is always descended.
I2SDF_WN_HD void wn_finish(const double m[WN_RECORD], double o0, double o1, double o2, const float lo[3], const float hi[3],
                           double t[WN_RECORD]) {
  const double o[3] = {o0, o1, o2};
  const bool some = m[0] > 0.0;
  double e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double p = m[1 + i] / m[0];
    t[i] = p;
    t[4 + i] = m[4 + i];
    const double below = p - (double)lo[i], above = (double)hi[i] - p;
    e[i] = below > above ? below : above;
    const double s = p - o[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[7 + 3 * i + j] = m[7 + 3 * i + j] - s * m[4 + j];
  }
  t[3] = some ? sqrt(wn_dot(e[0], e[1], e[2], e[0], e[1], e[2])) : INFINITY;
}

// The far field of one node seen from q, in units of solid angle (as tri_solid_angle).  Returns false -- visit the children -- unless
// d^2 > beta^2 r^2 (a NaN on either side: false).
I2SDF_WN_HD bool wn_far_field(double q0, double q1, double q2, const double t[WN_RECORD], double beta2, double& omega) {
  const double r[3] = {t[0] - q0, t[1] - q1, t[2] - q2};
  const double d2 = wn_dot(r[0], r[1], r[2], r[0], r[1], r[2]);
  if (!(d2 > beta2 * (t[3] * t[3]))) return false;
  const double d = sqrt(d2);
  const double d3 = d2 * d, d5 = d3 * d2;
  const double order0 = wn_dot(r[0], r[1], r[2], t[4], t[5], t[6]) / d3;
  const double trace = (t[7] + t[11]) + t[15];
  double quad = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) quad = quad + (r[i] * r[j]) * t[7 + 3 * j + i];
  const double order1 = trace / d3 - (3.0 * quad) / d5;
  omega = order0 + order1;
  return true;
}

}  // namespace i2sdf
