// Surface shading, per point and per sample, for the host and the device (shade.hip; tests/shade_probe.cpp compiles it for the host).
//
// The reference's RenderingLayer (model/rendering/__init__.py) with its BRDF library (model/rendering/brdf.py), restated as a function
// of ONE surface point and ONE sample.  Every clamp, threshold and branch order below is the reference's: they are the behaviour.
//
//   frame     z = n / max(|n|, 1e-6);  s = z_z >= 0 ? 1 : -1;  a = -1 / (s + z_z);  b = z_x z_y a;
//             x = (1 + s z_x^2 a, s b, -s z_x);  y = (b, s + z_y^2 a, -z_y)                       [Duff et al. 2017]
//   wi        (x.v, y.v, z.v) of the view direction v;  wi_mask = wi_z >= 1e-5;  wi_z raised to 1e-5;  wi / max(|wi|, 1e-6)
//   lobe      pS = lS / (lD + lS), l = max(0.212671 r + 0.715160 g + 0.072169 b, 0.01) of Kd and Ks;  diffuse iff u0 >= pS
//   diffuse   wo = (cos(2 pi u1) sq(u2), sin(2 pi u1) sq(u2), sq(max(1 - u2, 0))),  sq(x) = sqrt(max(x, 1e-8))
//   specular  alpha = rough^2;  Vh = nrm(alpha wi_x, alpha wi_y, wi_z);  q = Vh_x^2 + Vh_y^2;
//             T1 = q > 0 ? (-Vh_y, Vh_x, 0) / sq(q) : (1, 0, 0);  T2 = Vh x T1;
//             t1 = sq(u1) cos(2 pi u2);  t2 = sq(u1) sin(2 pi u2);  s = (1 + Vh_z) / 2;  t2 <- lerp(sq(1 - t1^2), t2, s);
//             Nh = t1 T1 + t2 T2 + sq(max(1 - t1^2 - t2^2, 0)) Vh;  h = nrm(alpha Nh_x, alpha Nh_y, max(Nh_z, 0));
//             wo = 2 (wi.h) h - wi                                  [Heitz 2018, sampling the visible normals]
//             nrm(v) = v / max(|v|, 1e-8);  lerp(a, b, s) = s < 1/2 ? a + s (b - a) : b - (b - a)(1 - s)  (torch.lerp)
//   pdf       H = nrm(wi + wo);  A = max(alpha^2, 1e-5) (inside D only);  D = A / (pi ((A - 1) H_z^2 + 1)^2);
//             G1 = 2 / (sq((alpha^2 (1 - wi_z^2) + wi_z^2) / wi_z^2) + 1);
//             pdf = pS D G1 / (4 wi_z) + (1 - pS) wo_z / pi;  1e-4 where wi_z <= 1e-4 or wo_z <= 1e-4;  then max(pdf, 1e-5)
//   f         f_diff = Kd / pi;  f_spec = wo_z < 1e-4 ? 1e-4 : F G2 D with
//             G2 = 1/2 / (wi_z sq(alpha^2 + wo_z (wo_z - alpha^2 wo_z)) + wo_z sq(alpha^2 + wi_z (wi_z - alpha^2 wi_z)));
//             F = Ks + (F90 - Ks) (1 - wo.H)^5,  F90 = min(25 lum(Ks), 1)   (lum without the 0.01 clamp)
//   weight    w = max(wo_z, 0) / pdf;  a sample adds f_diff w L to colorDiffuse and f_spec w L to colorSpec (L: incident radiance)
//
// Derivatives.  Of the differentiable inputs only `rough` reaches wo (through alpha), and with wo the pdf, D, G2, F and w; Kd enters
// linearly; Ks enters through F alone, piecewise linearly (pS is a constant of the backward, as under the reference's no_grad).  So the
// per-sample function is written once for a scalar type S that is either a real or Dual<real> -- a value with ONE tangent, d/d rough --
// and the Kd and Ks derivatives are closed forms over its results.  A clamp passes the tangent where the reference's autograd does:
// max(x, m) for x >= m, min(x, m) for x <= m, a select for the side taken.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define I2SDF_HD __host__ __device__ __forceinline__
#else
#define I2SDF_HD inline
#endif

namespace i2sdf_brdf {

template <class T> struct Dual { T v, d; };
template <class S> struct Real { using type = S; };
template <class T> struct Real<Dual<T>> { using type = T; };

template <class T> I2SDF_HD Dual<T> operator+(Dual<T> a, Dual<T> b) { return {a.v + b.v, a.d + b.d}; }
template <class T> I2SDF_HD Dual<T> operator-(Dual<T> a, Dual<T> b) { return {a.v - b.v, a.d - b.d}; }
template <class T> I2SDF_HD Dual<T> operator*(Dual<T> a, Dual<T> b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
template <class T> I2SDF_HD Dual<T> operator/(Dual<T> a, Dual<T> b) { const T q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
template <class T> I2SDF_HD Dual<T> operator-(Dual<T> a) { return {-a.v, -a.d}; }
template <class T> I2SDF_HD Dual<T> operator+(Dual<T> a, T b) { return {a.v + b, a.d}; }
template <class T> I2SDF_HD Dual<T> operator+(T a, Dual<T> b) { return {a + b.v, b.d}; }
template <class T> I2SDF_HD Dual<T> operator-(Dual<T> a, T b) { return {a.v - b, a.d}; }
template <class T> I2SDF_HD Dual<T> operator-(T a, Dual<T> b) { return {a - b.v, -b.d}; }
template <class T> I2SDF_HD Dual<T> operator*(Dual<T> a, T b) { return {a.v * b, a.d * b}; }
template <class T> I2SDF_HD Dual<T> operator*(T a, Dual<T> b) { return {a * b.v, a * b.d}; }
template <class T> I2SDF_HD Dual<T> operator/(Dual<T> a, T b) { return {a.v / b, a.d / b}; }
template <class T> I2SDF_HD Dual<T> operator/(T a, Dual<T> b) { const T q = a / b.v; return {q, -q * b.d / b.v}; }

// value / tangent of either scalar type, and a constant of it
I2SDF_HD float val(float x) { return x; }
I2SDF_HD double val(double x) { return x; }
template <class T> I2SDF_HD T val(Dual<T> x) { return x.v; }
I2SDF_HD float tan_of(float) { return 0.f; }
I2SDF_HD double tan_of(double) { return 0.0; }
template <class T> I2SDF_HD T tan_of(Dual<T> x) { return x.d; }
template <class S> struct Make { static I2SDF_HD S constant(S c) { return c; } };
template <class T> struct Make<Dual<T>> { static I2SDF_HD Dual<T> constant(T c) { return {c, T(0)}; } };

I2SDF_HD float root(float x) { return sqrtf(x); }
I2SDF_HD double root(double x) { return sqrt(x); }
template <class T> I2SDF_HD Dual<T> root(Dual<T> x) { const T r = root(x.v); return {r, x.d / (r + r)}; }

// max(x, m) / min(x, m) with torch.clamp's derivative: the tangent passes where x itself is returned, bound included
template <class S> I2SDF_HD S at_least(S x, typename Real<S>::type m) { return val(x) >= m ? x : Make<S>::constant(m); }
template <class S> I2SDF_HD S at_most(S x, typename Real<S>::type m) { return val(x) <= m ? x : Make<S>::constant(m); }
// the reference's sqrt_: sqrt(max(x, 1e-8))
template <class S> I2SDF_HD S sq(S x) { return root(at_least(x, typename Real<S>::type(1e-8))); }

// sin / cos of u REVOLUTIONS (phi = 2 pi u, u a uniform of [0, 1)).  On the device sincospif(2 u): its range reduction is exact, no 2 pi u is
// ever rounded.  NOT v_sin_f32 / v_cos_f32, although they take revolutions directly: measured on gfx950 they put the sampled directions
// of the two golden fixtures 1.0e-5 and 1.8e-5 (max-norm) from the fp64 ones, against a forward bar of 2e-5; this form 7.5e-6 and 3.8e-6,
// which is what fp32 leaves of sq(1 - t1^2 - t2^2) for a sample with u1 near 1.
template <class T> I2SDF_HD void sincos_turns(T u, T& s, T& c) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (sizeof(T) == 4) {
    float sf, cf;
    sincospif(2.0f * (float)u, &sf, &cf);
    s = T(sf); c = T(cf);
    return;
  }
#endif
  const T phi = T(6.283185307179586476925286766559) * u;
  s = T(sin((double)phi)); c = T(cos((double)phi));
}

template <class T> I2SDF_HD T luminance(const T (&c)[3]) { return c[0] * T(0.212671) + c[1] * T(0.715160) + c[2] * T(0.072169); }

// ---------------------------------------------------------------------------------------------------------------------------------
// what is the same for every sample of a point
// ---------------------------------------------------------------------------------------------------------------------------------
template <class T> struct Point {
  T x[3], y[3], z[3];      // the frame, rows of the world -> local rotation
  T wi[3];                 // local view direction, wi_z >= ~1e-5
  bool wi_mask;            // the view is above the surface
  T pS;                    // probability of the specular lobe
  T Kd[3], Ks[3];
  T f90, df90;             // F90 and its derivative by lum(Ks): 25 where 25 lum <= 1, else 0
};

template <class T>
I2SDF_HD void point_setup(const T (&n)[3], const T (&v)[3], const T (&Kd)[3], const T (&Ks)[3], Point<T>& p) {
  T len = root(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  len = len > T(1e-6) ? len : T(1e-6);
  const T zx = n[0] / len, zy = n[1] / len, zz = n[2] / len;
  const T s = zz >= T(0) ? T(1) : T(-1);
  const T a = T(-1) / (s + zz);
  const T b = zx * zy * a;
  p.x[0] = T(1) + s * zx * zx * a; p.x[1] = s * b; p.x[2] = -s * zx;
  p.y[0] = b; p.y[1] = s + zy * zy * a; p.y[2] = -zy;
  p.z[0] = zx; p.z[1] = zy; p.z[2] = zz;
  T w0 = p.x[0] * v[0] + p.x[1] * v[1] + p.x[2] * v[2];
  T w1 = p.y[0] * v[0] + p.y[1] * v[1] + p.y[2] * v[2];
  T w2 = p.z[0] * v[0] + p.z[1] * v[1] + p.z[2] * v[2];
  p.wi_mask = w2 >= T(1e-5);
  w2 = w2 < T(1e-5) ? T(1e-5) : w2;
  T wl = root(w0 * w0 + w1 * w1 + w2 * w2);
  wl = wl > T(1e-6) ? wl : T(1e-6);
  p.wi[0] = w0 / wl; p.wi[1] = w1 / wl; p.wi[2] = w2 / wl;
  for (int c = 0; c < 3; ++c) { p.Kd[c] = Kd[c]; p.Ks[c] = Ks[c]; }
  T lD = luminance(Kd), lS = luminance(Ks);
  const T f = T(25) * lS;
  p.f90 = f <= T(1) ? f : T(1);
  p.df90 = f <= T(1) ? T(25) : T(0);
  lD = lD >= T(0.01) ? lD : T(0.01);
  lS = lS >= T(0.01) ? lS : T(0.01);
  p.pS = lS / (lD + lS);
}

// v / max(|v|, 1e-8)
template <class S> I2SDF_HD void normalize3(S (&v)[3]) {
  const S len = at_least(root(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), typename Real<S>::type(1e-8));
  v[0] = v[0] / len; v[1] = v[1] / len; v[2] = v[2] / len;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// one sample: S = T (values) or Dual<T> (values and d / d rough)
// ---------------------------------------------------------------------------------------------------------------------------------
template <class S> struct Sample {
  S wo[3];           // local outgoing direction
  S pdf;             // mixture pdf, after both 1e-4 substitutes and the 1e-5 floor
  S w;               // max(wo_z, 0) / pdf
  S gd;              // G2 D: f_spec = F gd
  S m5;              // (1 - wo.H)^5: F = Ks + (F90 - Ks) m5
  bool spec_const;   // wo_z < 1e-4: f_spec = 1e-4, a constant
};

// the sampled direction alone (shade_sample needs no more)
template <class S, class T>
I2SDF_HD void sample_direction(const Point<T>& p, S rough, T u0, T u1, T u2, S (&wo)[3]) {
  if (u0 >= p.pS) {      // cosine hemisphere from (u1, u2)
    T sn, cs;
    sincos_turns(u1, sn, cs);
    const T r = sq(u2), ct = sq(u2 <= T(1) ? T(1) - u2 : T(0));
    wo[0] = Make<S>::constant(cs * r); wo[1] = Make<S>::constant(sn * r); wo[2] = Make<S>::constant(ct);
    return;
  }
  const S alpha = rough * rough;
  S Vh[3] = {alpha * p.wi[0], alpha * p.wi[1], Make<S>::constant(p.wi[2])};
  normalize3(Vh);
  const S lensq = Vh[0] * Vh[0] + Vh[1] * Vh[1];
  S T1[3];
  if (val(lensq) > T(0)) {
    const S il = sq(lensq);
    T1[0] = -Vh[1] / il; T1[1] = Vh[0] / il; T1[2] = Make<S>::constant(T(0));
  } else {
    T1[0] = Make<S>::constant(T(1)); T1[1] = Make<S>::constant(T(0)); T1[2] = Make<S>::constant(T(0));
  }
  const S T2[3] = {Vh[1] * T1[2] - Vh[2] * T1[1], Vh[2] * T1[0] - Vh[0] * T1[2], Vh[0] * T1[1] - Vh[1] * T1[0]};
  T sn, cs;
  sincos_turns(u2, sn, cs);
  const T r = sq(u1);
  const T t1 = r * cs, t2u = r * sn;
  const S s = T(0.5) * (T(1) + Vh[2]);
  const T e0 = sq(T(1) - t1 * t1);
  const S t2 = val(s) < T(0.5) ? e0 + s * (t2u - e0) : t2u - (t2u - e0) * (T(1) - s);
  const S nz = sq(at_least(T(1) - t1 * t1 - t2 * t2, T(0)));
  S Nh[3];
  for (int k = 0; k < 3; ++k) Nh[k] = t1 * T1[k] + t2 * T2[k] + nz * Vh[k];
  S h[3] = {alpha * Nh[0], alpha * Nh[1], at_least(Nh[2], T(0))};
  normalize3(h);
  const S dot = T(2) * (p.wi[0] * h[0] + p.wi[1] * h[1] + p.wi[2] * h[2]);
  for (int k = 0; k < 3; ++k) wo[k] = dot * h[k] - p.wi[k];
}

template <class S, class T>
I2SDF_HD void sample_eval(const Point<T>& p, S rough, T u0, T u1, T u2, Sample<S>& o) {
  sample_direction(p, rough, u0, u1, u2, o.wo);
  const T nv = p.wi[2];
  const S nl = o.wo[2];
  const S alpha = rough * rough;
  const S a2 = alpha * alpha;
  S H[3] = {p.wi[0] + o.wo[0], p.wi[1] + o.wo[1], p.wi[2] + o.wo[2]};
  normalize3(H);
  const S A = at_least(a2, T(1e-5));
  const S b = (A - T(1)) * H[2] * H[2] + T(1);
  const S D = A / (T(3.14159265358979323846) * b * b);
  const T nv2 = nv * nv;
  const S G1 = T(2) / (sq((a2 * (T(1) - nv2) + nv2) / nv2) + T(1));
  const S pdf_spec = D * G1 / (T(4) * nv);
  const S pdf_diff = nl / T(3.14159265358979323846);
  S pdf = p.pS * pdf_spec + (T(1) - p.pS) * pdf_diff;
  if (nv <= T(1e-4)) pdf = Make<S>::constant(T(1e-4));
  if (val(nl) <= T(1e-4)) pdf = Make<S>::constant(T(1e-4));
  o.pdf = at_least(pdf, T(1e-5));
  const S ga = nv * sq(a2 + nl * (nl - a2 * nl));
  const S gb = nl * sq(a2 + nv * (nv - a2 * nv));
  o.gd = T(0.5) / (ga + gb) * D;
  const S m = T(1) - (o.wo[0] * H[0] + o.wo[1] * H[1] + o.wo[2] * H[2]);
  const S m2 = m * m;
  o.m5 = m2 * m2 * m;
  o.spec_const = val(nl) < T(1e-4);
  o.w = at_least(nl, T(0)) / o.pdf;
}

// f_spec of channel c
template <class S, class T> I2SDF_HD S spec_channel(const Point<T>& p, const Sample<S>& o, int c) {
  if (o.spec_const) return Make<S>::constant(T(1e-4));
  return (p.Ks[c] + (p.f90 - p.Ks[c]) * o.m5) * o.gd;
}

}  // namespace i2sdf_brdf
