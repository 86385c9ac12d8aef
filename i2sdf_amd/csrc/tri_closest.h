// The point / triangle rule, the point / box bound and the pseudonormal sign of the closest-point query (include/i2sdf.h, "Closest
// point"), shared by the device kernels of closest.hip and by host code (tests/test_closest_host.py compiles this header with g++),
// like tri_isect.h.
//
// The rule is Ericson, Real-Time Collision Detection, 5.1.5.  Every operation is ONE fp64 operation on the exact images of the fp32
// inputs, rounded to nearest, in the order written, none contracted into an FMA; a dot product is (x x' + y y') + z z'.
// tests/closest_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define I2SDF_CP_HD __host__ __device__ __forceinline__
#else
#define I2SDF_CP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace i2sdf {

constexpr int CP_FACE = 0, CP_EDGE_AB = 1, CP_EDGE_BC = 2, CP_EDGE_CA = 3, CP_VERT_A = 4, CP_VERT_B = 5, CP_VERT_C = 6;
constexpr double CP_BOX_REL = 1.0 / 1048576.0;            // 2^-20: the relative part of the box slack (i2sdf.h derives it)
constexpr double CP_BOX_ABS = 1.0 / 4294967296.0;         // 2^-32: its absolute part, in units of the largest coordinate magnitude

struct ClosestHit {
  double c0, c1, c2;           // the closest point, unrounded
  double d2;                   // |p - c|^2
  double u, v;                 // the weights of A and of B
  int feature;
};

I2SDF_CP_HD double cp_dot(double x, double y, double z, double a, double b, double c) { return (x * a + y * b) + z * c; }

// One face against one point.  (Whether the face may be closest at all -- valid indices, finite vertices, a non-zero ab x ac -- is
// the caller's business: tri_degenerate below.)
I2SDF_CP_HD void tri_closest(double p0, double p1, double p2, double a0, double a1, double a2, double b0, double b1, double b2, double c0,
                             double c1, double c2, ClosestHit& h) {
  const double ab0 = b0 - a0, ab1 = b1 - a1, ab2 = b2 - a2;
  const double ac0 = c0 - a0, ac1 = c1 - a1, ac2 = c2 - a2;
  const double ap0 = p0 - a0, ap1 = p1 - a1, ap2 = p2 - a2;
  const double d1 = cp_dot(ab0, ab1, ab2, ap0, ap1, ap2), d2 = cp_dot(ac0, ac1, ac2, ap0, ap1, ap2);
  const double bp0 = p0 - b0, bp1 = p1 - b1, bp2 = p2 - b2;
  const double d3 = cp_dot(ab0, ab1, ab2, bp0, bp1, bp2), d4 = cp_dot(ac0, ac1, ac2, bp0, bp1, bp2);
  const double cp0 = p0 - c0, cp1 = p1 - c1, cp2 = p2 - c2;
  const double d5 = cp_dot(ab0, ab1, ab2, cp0, cp1, cp2), d6 = cp_dot(ac0, ac1, ac2, cp0, cp1, cp2);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  double x0, x1, x2, u, v;
  int feature;
  if (d1 <= 0.0 && d2 <= 0.0) {
    feature = CP_VERT_A; x0 = a0; x1 = a1; x2 = a2; u = 1.0; v = 0.0;
  } else if (d3 >= 0.0 && d4 <= d3) {
    feature = CP_VERT_B; x0 = b0; x1 = b1; x2 = b2; u = 0.0; v = 1.0;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double s = d1 / (d1 - d3);
    feature = CP_EDGE_AB; x0 = a0 + s * ab0; x1 = a1 + s * ab1; x2 = a2 + s * ab2; u = 1.0 - s; v = s;
  } else if (d6 >= 0.0 && d5 <= d6) {
    feature = CP_VERT_C; x0 = c0; x1 = c1; x2 = c2; u = 0.0; v = 0.0;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    feature = CP_EDGE_CA; x0 = a0 + w * ac0; x1 = a1 + w * ac1; x2 = a2 + w * ac2; u = 1.0 - w; v = 0.0;
  } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
    const double w = e43 / (e43 + e56);
    feature = CP_EDGE_BC; x0 = b0 + w * (c0 - b0); x1 = b1 + w * (c1 - b1); x2 = b2 + w * (c2 - b2); u = 0.0; v = 1.0 - w;
  } else {
    const double den = 1.0 / ((va + vb) + vc);
    const double s = vb * den, w = vc * den;
    feature = CP_FACE; x0 = (a0 + s * ab0) + w * ac0; x1 = (a1 + s * ab1) + w * ac1; x2 = (a2 + s * ab2) + w * ac2; u = (1.0 - s) - w; v = s;
  }
  const double r0 = p0 - x0, r1 = p1 - x1, r2 = p2 - x2;
  h.c0 = x0; h.c1 = x1; h.c2 = x2;
  h.d2 = cp_dot(r0, r1, r2, r0, r1, r2);
  h.u = u; h.v = v;
  h.feature = feature;
}

// ab x ac (not normalised): the face normal of the sign test, and the zero test of the faces that are never closest
I2SDF_CP_HD void tri_cross(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1, double c2, double& n0,
                           double& n1, double& n2) {
  const double ab0 = b0 - a0, ab1 = b1 - a1, ab2 = b2 - a2;
  const double ac0 = c0 - a0, ac1 = c1 - a1, ac2 = c2 - a2;
  n0 = ab1 * ac2 - ab2 * ac1;
  n1 = ab2 * ac0 - ab0 * ac2;
  n2 = ab0 * ac1 - ab1 * ac0;
}
I2SDF_CP_HD bool tri_degenerate(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1, double c2) {
  double n0, n1, n2;
  tri_cross(a0, a1, a2, b0, b1, b2, c0, c1, c2, n0, n1, n2);
  return n0 == 0.0 && n1 == 0.0 && n2 == 0.0;
}

// does (d2, face) displace the best so far?  bound: max_dist^2.  (A NaN d2 never counts.)
I2SDF_CP_HD bool closest_takes(double d2, int32_t face, double bound, double best_d2, int32_t best_face) {
  if (!(d2 <= bound)) return false;
  return best_face < 0 || d2 < best_d2 || (d2 == best_d2 && face < best_face);
}

// The box bound.  q: the squared distance of p to the box [lo, hi] (the exact fp32 min / max of the vertices below it).
I2SDF_CP_HD double box_dist2(double p0, double p1, double p2, float lo0, float lo1, float lo2, float hi0, float hi1, float hi2) {
  const double l0 = (double)lo0 - p0, l1 = (double)lo1 - p1, l2 = (double)lo2 - p2;
  const double g0 = p0 - (double)hi0, g1 = p1 - (double)hi1, g2 = p2 - (double)hi2;
  double e0 = l0 > g0 ? l0 : g0, e1 = l1 > g1 ? l1 : g1, e2 = l2 > g2 ? l2 : g2;
  e0 = e0 > 0.0 ? e0 : 0.0; e1 = e1 > 0.0 ? e1 : 0.0; e2 = e2 > 0.0 ? e2 : 0.0;
  return (e0 * e0 + e1 * e1) + e2 * e2;
}
// A box is skipped iff q > box_skip_above(bound, M): bound the best d2 so far (max_dist^2 before there is one), M the largest
// coordinate magnitude of the query and of the mesh's bounds.  include/i2sdf.h, "Closest point", derives that no face below a skipped
// box has a computed d2 <= bound.  q == bound is entered (a tie may go to a smaller face index); a NaN on either side never skips;
// the empty box (+inf, -inf) has q = +inf and is skipped unless the threshold is +inf too (its leaves hold no face anyway).
I2SDF_CP_HD double box_skip_above(double bound, double M) {
  const double r = sqrt(bound) * (1.0 + CP_BOX_REL) + CP_BOX_ABS * M;
  return r * r;
}

// The sign of the pseudonormal test: +1 outside (and on the surface), -1 inside.
I2SDF_CP_HD double closest_sign(double p0, double p1, double p2, const ClosestHit& h, double n0, double n1, double n2) {
  return cp_dot(p0 - h.c0, p1 - h.c1, p2 - h.c2, n0, n1, n2) >= 0.0 ? 1.0 : -1.0;
}

}  // namespace i2sdf
