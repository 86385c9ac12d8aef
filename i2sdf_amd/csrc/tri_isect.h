// The ray / triangle rule and the ray / box test of the ray caster (include/i2sdf.h, "Ray casting"), shared by the device kernels of
// bvh.hip and by host code (tests/test_raycast_host.py compiles this header with g++), like brdf_dev.h.
//
// The rule is the watertight test of Woop, Benthin and Wald (JCGT 2013).  Every operation is ONE fp32 operation, rounded to nearest,
// in the order written, none contracted into an FMA: a*b - c*d is the exact negative of c*d - a*b only without one, and two faces that
// share an edge compute exactly negated edge functions there only then.  tests/raycast_ref.py restates it in numpy.
//
// Nothing in here indexes an array with a run-time value (pick3 selects), so that on the device everything stays in registers.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define I2SDF_TRI_HD __host__ __device__ __forceinline__
#else
#define I2SDF_TRI_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace i2sdf {

constexpr int RAY_CULL_NONE = 0, RAY_CULL_BACK = 1;
constexpr float BOX_T_SLACK = 1.0f / 1048576.0f;      // 2^-20: the relative widening of a box's depth interval (i2sdf.h derives 2^-21)

struct RayShear {
  int kx, ky, kz;
  float Sx, Sy, Sz;
  float ox, oy, oz;            // the origin, permuted to (kx, ky, kz)
};

I2SDF_TRI_HD float pick3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }
I2SDF_TRI_HD bool finite_f(float x) { return x - x == 0.0f; }

// false: a ray that hits nothing and sets I2SDF_RAYCAST_BAD_RAY (a non-finite component, the zero direction, 1 / d[kz] not finite)
I2SDF_TRI_HD bool ray_shear(float ox, float oy, float oz, float dx, float dy, float dz, RayShear& r) {
  if (!(finite_f(ox) && finite_f(oy) && finite_f(oz) && finite_f(dx) && finite_f(dy) && finite_f(dz))) return false;
  int kz = 0;
  float m = fabsf(dx);
  if (fabsf(dy) > m) { kz = 1; m = fabsf(dy); }
  if (fabsf(dz) > m) { kz = 2; m = fabsf(dz); }
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const float dkz = pick3(dx, dy, dz, kz);
  if (dkz < 0.0f) { const int s = kx; kx = ky; ky = s; }
  r.kx = kx; r.ky = ky; r.kz = kz;
  r.Sx = pick3(dx, dy, dz, kx) / dkz;
  r.Sy = pick3(dx, dy, dz, ky) / dkz;
  r.Sz = 1.0f / dkz;
  r.ox = pick3(ox, oy, oz, kx); r.oy = pick3(ox, oy, oz, ky); r.oz = pick3(ox, oy, oz, kz);
  return m > 0.0f && finite_f(r.Sz);
}

// One face.  true: the face is hit at t with t_min < t <= t_max; u, v are the barycentric weights of A and B.
I2SDF_TRI_HD bool tri_hit(const RayShear& r, float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1, float c2,
                          float t_min, float t_max, int cull, float& t, float& u, float& v) {
  const float Akz = pick3(a0, a1, a2, r.kz) - r.oz, Bkz = pick3(b0, b1, b2, r.kz) - r.oz, Ckz = pick3(c0, c1, c2, r.kz) - r.oz;
  const float Ax = (pick3(a0, a1, a2, r.kx) - r.ox) - r.Sx * Akz, Ay = (pick3(a0, a1, a2, r.ky) - r.oy) - r.Sy * Akz;
  const float Bx = (pick3(b0, b1, b2, r.kx) - r.ox) - r.Sx * Bkz, By = (pick3(b0, b1, b2, r.ky) - r.oy) - r.Sy * Bkz;
  const float Cx = (pick3(c0, c1, c2, r.kx) - r.ox) - r.Sx * Ckz, Cy = (pick3(c0, c1, c2, r.ky) - r.oy) - r.Sy * Ckz;
  float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  if (U == 0.0f || V == 0.0f || W == 0.0f) {      // on an edge (or a vertex) as far as fp32 can tell: all three again, exactly
    U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
    V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
    W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
  }
  if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
  const float det = (U + V) + W;
  if (det == 0.0f) return false;
  if (cull == RAY_CULL_BACK && det < 0.0f) return false;      // the right-hand normal points along the ray
  const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
  const float T = (U * Az + V * Bz) + W * Cz;
  t = T / det;
  if (!(t_min < t && t <= t_max)) return false;               // (a NaN t or bound fails it)
  u = U / det;
  v = V / det;
  return true;
}

// One box [lo, hi] (the exact fp32 min / max of the vertices below it).  false ONLY if tri_hit above accepts no face all of whose
// vertices lie in the box with t_min < t <= t_max (include/i2sdf.h, "Ray casting", derives that); a comparison with a NaN operand
// never skips.  t_near: the lower end of the widened depth interval, to order the two children of a node.
I2SDF_TRI_HD bool box_may_hit(const RayShear& r, float lo0, float lo1, float lo2, float hi0, float hi1, float hi2, float t_min, float t_max,
                              float& t_near) {
  if (!(lo0 <= hi0)) return false;                // the empty box (+inf, -inf) of a subtree without a valid face
  const float zl = pick3(lo0, lo1, lo2, r.kz) - r.oz, zh = pick3(hi0, hi1, hi2, r.kz) - r.oz;
  // sheared x and y of a vertex are monotone in its kx / ky coordinate and in its kz coordinate: their extremes lie at box corners
  const float sxl = r.Sx * zl, sxh = r.Sx * zh, syl = r.Sy * zl, syh = r.Sy * zh;
  const float x_min = (pick3(lo0, lo1, lo2, r.kx) - r.ox) - (r.Sx >= 0.0f ? sxh : sxl);
  const float x_max = (pick3(hi0, hi1, hi2, r.kx) - r.ox) - (r.Sx >= 0.0f ? sxl : sxh);
  if (x_min > 0.0f || x_max < 0.0f) return false;
  const float y_min = (pick3(lo0, lo1, lo2, r.ky) - r.oy) - (r.Sy >= 0.0f ? syh : syl);
  const float y_max = (pick3(hi0, hi1, hi2, r.ky) - r.oy) - (r.Sy >= 0.0f ? syl : syh);
  if (y_min > 0.0f || y_max < 0.0f) return false;
  const float za = r.Sz * zl, zb = r.Sz * zh;
  const float z_near = r.Sz >= 0.0f ? za : zb, z_far = r.Sz >= 0.0f ? zb : za;
  t_near = z_near - fabsf(z_near) * BOX_T_SLACK;
  const float t_far = z_far + fabsf(z_far) * BOX_T_SLACK;
  if (t_near > t_max || t_far < t_min) return false;          // t_near == t_max is entered: a tie may go to a smaller face index
  return true;
}

}  // namespace i2sdf
