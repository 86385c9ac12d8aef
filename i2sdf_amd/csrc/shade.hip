// Surface shading on the device: the reference's RenderingLayer (model/rendering/__init__.py) around the model call.
//
//   shade_sample    frame, wi, wi_mask, the uniforms, wo -> world direction and the offset origin of every secondary ray
//   (the caller asks the model for the radiance along those rays)
//   shade_reduce    colorDiffuse / colorSpec = mean over the samples of f cos / pdf L
//   shade_backward  the gradients of both by Kd, Ks, rough, radiance and radiance_scale, and the path rough -> direction / points
//   shade_draws     the uniforms a seed stands for
//
// The per-sample arithmetic is brdf_dev.h.  Nothing per-sample is kept between the kernels: each one recomputes wo, pdf and f from the
// same uniforms, which are either the caller's (bn, spp, 3) tensor or Philox4x32-10 words with counter (point spp + s, 0, 8, 0) --
// stream word 8; draws.hip uses 1..6, bubble.hip 7 -- and key = the 64-bit seed, words x, y, z as u0, u1, u2.
//
// Sums over the samples of a point: G = 2^k lanes of a wave share a point, lane j of them takes samples j, j + G, ..., and the G partial
// sums meet in a butterfly of log2 G exchanges: a fixed order, no atomics, bitwise reproducible.  G is the smallest power of two that is
// >= min(spp, 64), so 64 / G points share a wave when spp < 64.  These kernels are VALU work (about 300 fp32 operations a sample with the
// sine / cosine pair, against 24 bytes read); a wave is issued whole whatever its active lanes, and nothing but more waves hides the
// quarter-rate sqrt / rcp chains, so a wave of spp lanes with 64 - spp idle ones would waste exactly that share of the SIMD.  With
// G as chosen at least half of the lanes work for every spp; the cost is one redundant point set-up (60 operations) per lane, not per
// point, which is cheap beside a sample.  No kernel uses scratch; the forward kernels keep 7 or 8 waves per SIMD resident, the backward 3.
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/i2sdf.h"
#include "philox.h"
#include "brdf_dev.h"

int i2sdf_hip_check(hipError_t e, const char* what);
int i2sdf_refuse(const char* why);

namespace {

using i2sdf_philox::U4;
using i2sdf_philox::philox4x32_10;
using i2sdf_philox::u01;
using namespace i2sdf_brdf;
typedef Dual<float> DF;

constexpr unsigned SHADE_STREAM = 8u;
constexpr int THREADS = 256;
constexpr float INV_PI = 0.31830988618379067154f;

// The three sums of g_radiance_scale over the workgroup: lanes -> wave (butterfly) -> workgroup (LDS, wave order).  Every thread calls
// it; thread c < 3 gets component c.
__device__ __forceinline__ float workgroup_sum3(float p0, float p1, float p2) {
  __shared__ float ws[THREADS / 64][3];
  float part[3] = {p0, p1, p2};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) part[c] += __shfl_xor(part[c], off);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { ws[wv][0] = part[0]; ws[wv][1] = part[1]; ws[wv][2] = part[2]; }
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < 3) {
    t = ws[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) t += ws[w][threadIdx.x];
  }
  return t;
}

struct ShadeArgs {
  const float *x, *view, *normal, *Kd, *Ks, *rough;      // (bn, 3) each, rough (bn, 1)
  const float* samples;                                  // (bn, spp, 3), or NULL: Philox
  unsigned seed_lo, seed_hi;
  int bn, spp, lg;                                       // lg: log2 of the lanes that share a point (reduce / backward)
  const float *radiance, *scale;                         // (bn spp, 3), (3) or NULL
  const float *g_cd, *g_cs, *g_dir, *g_pts;              // upstream gradients; each pair may be NULL
  float *direction, *points;                             // (bn spp, 3)
  uint8_t* wi_mask;                                      // (bn)
  float *cd, *cs;                                        // (bn, 3)
  float *gKd, *gKs, *grough, *g_rad, *partial;           // (bn, 3), (bn, 3), (bn, 1), (bn spp, 3) or NULL, (blocks, 3) or NULL
};

__device__ __forceinline__ void uniforms(const ShadeArgs& a, int i, float& u0, float& u1, float& u2) {
  if (a.samples != nullptr) {
    const float* s = a.samples + 3 * (int64_t)i;
    u0 = s[0]; u1 = s[1]; u2 = s[2];
  } else {
    const U4 r = philox4x32_10(U4{(unsigned)i, 0u, SHADE_STREAM, 0u}, a.seed_lo, a.seed_hi);
    u0 = u01(r.x); u1 = u01(r.y); u2 = u01(r.z);
  }
}

__device__ __forceinline__ void load_point(const ShadeArgs& a, int p, Point<float>& pt) {
  const int64_t o = 3 * (int64_t)p;
  const float n[3] = {a.normal[o], a.normal[o + 1], a.normal[o + 2]};
  const float v[3] = {a.view[o], a.view[o + 1], a.view[o + 2]};
  const float kd[3] = {a.Kd[o], a.Kd[o + 1], a.Kd[o + 2]};
  const float ks[3] = {a.Ks[o], a.Ks[o + 1], a.Ks[o + 2]};
  point_setup(n, v, kd, ks, pt);
}

__global__ __launch_bounds__(THREADS) void shade_draws_kernel(ShadeArgs a, float* out) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (int64_t)a.bn * a.spp) return;
  float u0, u1, u2;
  uniforms(a, (int)i, u0, u1, u2);
  out[3 * i] = u0; out[3 * i + 1] = u1; out[3 * i + 2] = u2;
}

// one lane per (point, sample)
__global__ __launch_bounds__(THREADS) void shade_sample_kernel(ShadeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (int64_t)a.bn * a.spp) return;
  const int p = (int)(i / a.spp);
  Point<float> pt;
  load_point(a, p, pt);
  float u0, u1, u2, wo[3];
  uniforms(a, (int)i, u0, u1, u2);
  sample_direction(pt, a.rough[p], u0, u1, u2, wo);
  if (i == (int64_t)p * a.spp) a.wi_mask[p] = pt.wi_mask ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = wo[0] * pt.x[k] + wo[1] * pt.y[k] + wo[2] * pt.z[k];
    a.direction[3 * i + k] = d;
    a.points[3 * i + k] = a.x[3 * (int64_t)p + k] + d * 0.01f;
  }
}

// G = 1 << lg lanes per point; every lane of the wave takes part in the exchanges (lanes behind the last point add zeros)
__global__ __launch_bounds__(THREADS) void shade_reduce_kernel(ShadeArgs a) {
  const int G = 1 << a.lg;
  const int64_t slot = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> a.lg;
  const int sub = threadIdx.x & (G - 1);
  const bool valid = slot < a.bn;
  const int p = valid ? (int)slot : 0;
  Point<float> pt;
  load_point(a, p, pt);
  const float rough = a.rough[p];
  float sc[3] = {1.f, 1.f, 1.f};
  if (a.scale != nullptr) { sc[0] = a.scale[0]; sc[1] = a.scale[1]; sc[2] = a.scale[2]; }
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = sub; valid && s < a.spp; s += G) {
    const int i = p * a.spp + s;
    float u0, u1, u2;
    uniforms(a, i, u0, u1, u2);
    Sample<float> o;
    sample_eval(pt, rough, u0, u1, u2, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float L = a.radiance[3 * (int64_t)i + c] * sc[c];
      acc[c] += pt.Kd[c] * INV_PI * o.w * L;
      acc[3 + c] += spec_channel(pt, o, c) * o.w * L;
    }
  }
  for (int off = G >> 1; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += __shfl_xor(acc[c], off);
  if (valid && sub == 0) {
    const float n = (float)a.spp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.cd[3 * (int64_t)p + c] = acc[c] / n;
      a.cs[3 * (int64_t)p + c] = acc[3 + c] / n;
    }
  }
}

// (132 registers: 3 waves per SIMD.  Bounded to 128 for a fourth wave it spills 12 bytes a lane, and no kernel here may use scratch.)
__global__ __launch_bounds__(THREADS) void shade_backward_kernel(ShadeArgs a) {
  const int G = 1 << a.lg;
  const int64_t slot = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> a.lg;
  const int sub = threadIdx.x & (G - 1);
  const bool valid = slot < a.bn;
  const int p = valid ? (int)slot : 0;
  const bool colour = a.g_cd != nullptr;
  Point<float> pt;
  load_point(a, p, pt);
  const DF rough = {a.rough[p], 1.f};
  float sc[3] = {1.f, 1.f, 1.f};
  if (a.scale != nullptr) { sc[0] = a.scale[0]; sc[1] = a.scale[1]; sc[2] = a.scale[2]; }
  const float n = (float)a.spp;
  float gd[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f};
  if (colour) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { gd[c] = a.g_cd[3 * (int64_t)p + c] / n; gs[c] = a.g_cs[3 * (int64_t)p + c] / n; }
  }
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // gKd, gKs, grough
  float common = 0.f;                                       // what reaches every Ks channel through F90
  float part[3] = {0.f, 0.f, 0.f};                          // this lane's share of g_radiance_scale
  for (int s = sub; valid && s < a.spp; s += G) {
    const int i = p * a.spp + s;
    float u0, u1, u2;
    uniforms(a, i, u0, u1, u2);
    Sample<DF> o;
    sample_eval(pt, rough, u0, u1, u2, o);
    if (colour) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float rad = a.radiance[3 * (int64_t)i + c];
        const float L = rad * sc[c];
        const float kd_pi = pt.Kd[c] * INV_PI;
        const DF fs = spec_channel(pt, o, c);
        const DF fw = fs * o.w;
        const float aD = gd[c] * L, aS = gs[c] * L;
        acc[c] += aD * o.w.v * INV_PI;
        acc[6] += aD * kd_pi * o.w.d + aS * fw.d;
        if (!o.spec_const) {
          const float base = aS * o.w.v * o.gd.v;
          acc[3 + c] += base * (1.f - o.m5.v);
          common += base * o.m5.v;
        }
        const float coef = (gd[c] * kd_pi + gs[c] * fs.v) * o.w.v;
        if (a.g_rad != nullptr) a.g_rad[3 * (int64_t)i + c] = coef * sc[c];
        part[c] += coef * rad;
      }
    }
    if (a.g_dir != nullptr || a.g_pts != nullptr) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float t = 0.f;
        if (a.g_dir != nullptr) t = a.g_dir[3 * (int64_t)i + k];
        if (a.g_pts != nullptr) t += 0.01f * a.g_pts[3 * (int64_t)i + k];
        acc[6] += t * (o.wo[0].d * pt.x[k] + o.wo[1].d * pt.y[k] + o.wo[2].d * pt.z[k]);
      }
    }
  }
  const float lw[3] = {0.212671f, 0.715160f, 0.072169f};
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[3 + c] += common * pt.df90 * lw[c];
  for (int off = G >> 1; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < 7; ++c) acc[c] += __shfl_xor(acc[c], off);
  if (valid && sub == 0) {
    if (colour) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { a.gKd[3 * (int64_t)p + c] = acc[c]; a.gKs[3 * (int64_t)p + c] = acc[3 + c]; }
    }
    a.grough[p] = acc[6];
  }
  if (a.partial != nullptr) {      // (uniform) g_radiance_scale: this workgroup's slot
    const float t = workgroup_sum3(part[0], part[1], part[2]);
    if (threadIdx.x < 3) a.partial[3 * (int64_t)blockIdx.x + threadIdx.x] = t;
  }
}

// second pass of g_radiance_scale: one workgroup, lane t takes slots t, t + 256, ..., then the same wave / workgroup order
__global__ __launch_bounds__(THREADS) void shade_scale_sum_kernel(const float* partial, int64_t blocks, float* out) {
  float part[3] = {0.f, 0.f, 0.f};
  for (int64_t b = threadIdx.x; b < blocks; b += THREADS)
#pragma unroll
    for (int c = 0; c < 3; ++c) part[c] += partial[3 * b + c];
  const float t = workgroup_sum3(part[0], part[1], part[2]);
  if (threadIdx.x < 3) out[threadIdx.x] = t;
}

int refuse(const std::string& why) { return i2sdf_refuse(why.c_str()); }

// sizes and the uniforms' source, shared by every entry point; 0 or I2SDF_EINVAL
int check_common(const char* who, int64_t bn, int32_t spp, const float* samples, const uint64_t* seed) {
  const std::string w(who);
  if (bn < 0) return refuse(w + ": bn < 0");
  if (spp < 1) return refuse(w + ": spp < 1");
  if (bn > (((int64_t)1 << 31) - 1) / spp) return refuse(w + ": bn spp >= 2^31");
  if (samples != nullptr && seed != nullptr) return refuse(w + ": both samples and seed given, one of them chooses the uniforms");
  if (samples == nullptr && seed == nullptr) return refuse(w + ": neither samples nor seed given");
  return I2SDF_OK;
}

int lanes_log2(int32_t spp) {
  int lg = 0;
  while (lg < 6 && (1 << lg) < spp) ++lg;
  return lg;
}

int64_t group_blocks(int64_t bn, int lg) {
  const int64_t per_block = THREADS >> lg;
  return (bn + per_block - 1) / per_block;
}

void set_source(ShadeArgs& a, const float* samples, const uint64_t* seed) {
  a.samples = samples;
  if (seed != nullptr) { a.seed_lo = (unsigned)*seed; a.seed_hi = (unsigned)(*seed >> 32); }
}

}  // namespace

extern "C" int i2sdf_shade_draws(uint64_t seed, int64_t bn, int32_t spp, float* samples, void* stream) {
  if (int rc = check_common("i2sdf_shade_draws", bn, spp, nullptr, &seed)) return rc;
  if (samples == nullptr) return refuse("i2sdf_shade_draws: samples is NULL");
  if (bn == 0) return I2SDF_OK;
  ShadeArgs a{};
  set_source(a, nullptr, &seed);
  a.bn = (int)bn; a.spp = spp;
  const int64_t total = bn * spp;
  shade_draws_kernel<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, (hipStream_t)stream>>>(a, samples);
  return i2sdf_hip_check(hipGetLastError(), "shade_draws_kernel");
}

extern "C" int i2sdf_shade_sample(const float* surface_points, const float* view_direction, const float* normal, const float* Kd,
                                  const float* Ks, const float* rough, const float* samples, const uint64_t* seed, int64_t bn, int32_t spp,
                                  float* direction, float* points, uint8_t* wi_mask, void* stream) {
  if (int rc = check_common("i2sdf_shade_sample", bn, spp, samples, seed)) return rc;
  if (!surface_points || !view_direction || !normal || !Kd || !Ks || !rough) return refuse("i2sdf_shade_sample: an input pointer is NULL");
  if (!direction || !points || !wi_mask) return refuse("i2sdf_shade_sample: an output pointer is NULL");
  if (bn == 0) return I2SDF_OK;
  ShadeArgs a{};
  set_source(a, samples, seed);
  a.x = surface_points; a.view = view_direction; a.normal = normal; a.Kd = Kd; a.Ks = Ks; a.rough = rough;
  a.bn = (int)bn; a.spp = spp;
  a.direction = direction; a.points = points; a.wi_mask = wi_mask;
  const int64_t total = bn * spp;
  shade_sample_kernel<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, (hipStream_t)stream>>>(a);
  return i2sdf_hip_check(hipGetLastError(), "shade_sample_kernel");
}

extern "C" int i2sdf_shade_reduce(const float* view_direction, const float* normal, const float* Kd, const float* Ks, const float* rough,
                                  const float* samples, const uint64_t* seed, const float* radiance, const float* radiance_scale, int64_t bn,
                                  int32_t spp, float* colorDiffuse, float* colorSpec, void* stream) {
  if (int rc = check_common("i2sdf_shade_reduce", bn, spp, samples, seed)) return rc;
  if (!view_direction || !normal || !Kd || !Ks || !rough || !radiance) return refuse("i2sdf_shade_reduce: an input pointer is NULL");
  if (!colorDiffuse || !colorSpec) return refuse("i2sdf_shade_reduce: an output pointer is NULL");
  if (bn == 0) return I2SDF_OK;
  ShadeArgs a{};
  set_source(a, samples, seed);
  a.view = view_direction; a.normal = normal; a.Kd = Kd; a.Ks = Ks; a.rough = rough;
  a.bn = (int)bn; a.spp = spp; a.lg = lanes_log2(spp);
  a.radiance = radiance; a.scale = radiance_scale;
  a.cd = colorDiffuse; a.cs = colorSpec;
  shade_reduce_kernel<<<(unsigned)group_blocks(bn, a.lg), THREADS, 0, (hipStream_t)stream>>>(a);
  return i2sdf_hip_check(hipGetLastError(), "shade_reduce_kernel");
}

extern "C" int64_t i2sdf_shade_backward_workspace_bytes(int64_t bn, int32_t spp) {
  if (bn < 0 || spp < 1 || bn > (((int64_t)1 << 31) - 1) / spp) return 0;
  return (group_blocks(bn, lanes_log2(spp)) * 3 * (int64_t)sizeof(float) + 15) / 16 * 16 + 16;
}

extern "C" int i2sdf_shade_backward(const float* view_direction, const float* normal, const float* Kd, const float* Ks, const float* rough,
                                    const float* samples, const uint64_t* seed, const float* radiance, const float* radiance_scale,
                                    const float* g_colorDiffuse, const float* g_colorSpec, const float* g_direction, const float* g_points,
                                    int64_t bn, int32_t spp, void* workspace, float* gKd, float* gKs, float* grough, float* g_radiance,
                                    float* g_radiance_scale, void* stream) {
  const char* who = "i2sdf_shade_backward";
  if (int rc = check_common(who, bn, spp, samples, seed)) return rc;
  if (!view_direction || !normal || !Kd || !Ks || !rough) return refuse("i2sdf_shade_backward: an input pointer is NULL");
  if (!grough) return refuse("i2sdf_shade_backward: grough is NULL");
  const bool colour = g_colorDiffuse != nullptr || g_colorSpec != nullptr;
  if (colour && (!g_colorDiffuse || !g_colorSpec || !radiance || !gKd || !gKs))
    return refuse("i2sdf_shade_backward: g_colorDiffuse, g_colorSpec, radiance, gKd and gKs go together, one of them is NULL");
  if (!colour && !g_direction && !g_points) return refuse("i2sdf_shade_backward: no upstream gradient given");
  if (!colour && (g_radiance || g_radiance_scale)) return refuse("i2sdf_shade_backward: g_radiance / g_radiance_scale need g_colorDiffuse and g_colorSpec");
  if (g_radiance_scale && !workspace) return refuse("i2sdf_shade_backward: g_radiance_scale needs the workspace");
  hipStream_t st = (hipStream_t)stream;
  if (bn == 0) {
    if (g_radiance_scale) return i2sdf_hip_check(hipMemsetAsync(g_radiance_scale, 0, 3 * sizeof(float), st), "shade_backward clear");
    return I2SDF_OK;
  }
  ShadeArgs a{};
  set_source(a, samples, seed);
  a.view = view_direction; a.normal = normal; a.Kd = Kd; a.Ks = Ks; a.rough = rough;
  a.bn = (int)bn; a.spp = spp; a.lg = lanes_log2(spp);
  a.radiance = radiance; a.scale = radiance_scale;
  a.g_cd = g_colorDiffuse; a.g_cs = g_colorSpec; a.g_dir = g_direction; a.g_pts = g_points;
  a.gKd = gKd; a.gKs = gKs; a.grough = grough; a.g_rad = g_radiance;
  a.partial = g_radiance_scale ? (float*)workspace : nullptr;
  const int64_t blocks = group_blocks(bn, a.lg);
  shade_backward_kernel<<<(unsigned)blocks, THREADS, 0, st>>>(a);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "shade_backward_kernel")) return rc;
  if (g_radiance_scale) {
    shade_scale_sum_kernel<<<1, THREADS, 0, st>>>(a.partial, blocks, g_radiance_scale);
    return i2sdf_hip_check(hipGetLastError(), "shade_scale_sum_kernel");
  }
  return I2SDF_OK;
}
