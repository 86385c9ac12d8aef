// The per-sample arithmetic of mesh simplification by vertex clustering (include/i2sdf.h, "Mesh simplification"): the quadric of one
// face about a cell centre, the regularised solve for the cell's representative and the clamp to the cell -- shared by the device
// kernel of simplify.hip and by host code (tests/test_simplify_host.py compiles this header with g++), like tri_closest.h.
//
// The quadric is Garland and Heckbert's with the unnormalised normal (so a face weighs in by its squared area), accumulated per cell
// as in Lindstrom, Out-of-core simplification of large polygonal models (SIGGRAPH 2000).  Every operation is ONE fp64 operation on the
// exact images of the fp32 inputs, rounded to nearest, in the order written, none contracted into an FMA; a dot product is
// (x x' + y y') + z z'.  tests/simplify_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define I2SDF_QD_HD __host__ __device__ __forceinline__
#else
#define I2SDF_QD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace i2sdf {

constexpr int QD_VALUES = 9;      // A as xx, xy, xz, yy, yz, zz, then bvec as x, y, z

I2SDF_QD_HD double qd_dot(double x, double y, double z, double a, double b, double c) { return (x * a + y * b) + z * c; }

// The quadric of face (a, b, c) about the centre cc:  n = (b - a) x (c - a),  d = -n . (a - cc);  q = (n n^T, d n).
I2SDF_QD_HD void quadric_face(const double a[3], const double b[3], const double c[3], const double cc[3], double q[QD_VALUES]) {
  const double e0 = b[0] - a[0], e1 = b[1] - a[1], e2 = b[2] - a[2];
  const double g0 = c[0] - a[0], g1 = c[1] - a[1], g2 = c[2] - a[2];
  const double n0 = e1 * g2 - e2 * g1, n1 = e2 * g0 - e0 * g2, n2 = e0 * g1 - e1 * g0;
  const double r0 = a[0] - cc[0], r1 = a[1] - cc[1], r2 = a[2] - cc[2];
  const double d = -qd_dot(n0, n1, n2, r0, r1, r2);
  q[0] = n0 * n0; q[1] = n0 * n1; q[2] = n0 * n2;
  q[3] = n1 * n1; q[4] = n1 * n2; q[5] = n2 * n2;
  q[6] = d * n0;  q[7] = d * n1;  q[8] = d * n2;
}

// The representative of a cell, relative to its centre:  (A + lambda I) x = -bvec + lambda m,  lambda = reg tr(A), by the adjugate of
// the symmetric matrix.  m: the cell's vertex mean minus the centre; half = h / 2.  Returns the fallback flag: tr(A) not finite and
// positive, or some |x_i| <= half not true (the minimiser left its cell, or is not a number) -> x = m.
I2SDF_QD_HD bool quadric_solve(const double q[QD_VALUES], double reg, const double m[3], double half, double x[3]) {
  const double tr = (q[0] + q[3]) + q[5];
  bool fallback = !(tr > 0.0) || !(tr < INFINITY);
  if (!fallback) {
    const double lam = reg * tr;
    const double m00 = q[0] + lam, m01 = q[1], m02 = q[2], m11 = q[3] + lam, m12 = q[4], m22 = q[5] + lam;
    const double r0 = lam * m[0] - q[6], r1 = lam * m[1] - q[7], r2 = lam * m[2] - q[8];
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = qd_dot(m00, m01, m02, c00, c01, c02);
    x[0] = qd_dot(c00, c01, c02, r0, r1, r2) / det;
    x[1] = qd_dot(c01, c11, c12, r0, r1, r2) / det;
    x[2] = qd_dot(c02, c12, c22, r0, r1, r2) / det;
    fallback = !(fabs(x[0]) <= half) || !(fabs(x[1]) <= half) || !(fabs(x[2]) <= half);
  }
  if (fallback) { x[0] = m[0]; x[1] = m[1]; x[2] = m[2]; }
  return fallback;
}

// The centre of cell index i along one axis: lo + (i + 1/2) h, lo = min - h / 2 (the grid of "Point sets": voxel_down_sample's).
I2SDF_QD_HD double quadric_cell_centre(double lo, int64_t i, double h) { return lo + ((double)i + 0.5) * h; }

// The normalised sum of normals, or zeros when the sum has no length.
I2SDF_QD_HD void quadric_normal(const double s[3], float out[3]) {
  const double len = sqrt(qd_dot(s[0], s[1], s[2], s[0], s[1], s[2]));
  const bool ok = len > 0.0 && len < INFINITY;
  out[0] = ok ? (float)(s[0] / len) : 0.0f;
  out[1] = ok ? (float)(s[1] / len) : 0.0f;
  out[2] = ok ? (float)(s[2] / len) : 0.0f;
}

}  // namespace i2sdf
