// The marching rule of i2sdf_trace_rays (include/i2sdf.h, "Sphere tracing"): one step of one ray, shared by the rule kernel of the
// stepwise route and by the fused kernels.  Every operation is a single fp32 operation: contraction is switched off inside the rule, so
// that no two of them fuse into an FMA and tests/trace_ref.py can replay the march bit for bit from the f of every step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/i2sdf.h"

namespace i2sdf {

struct TraceRay {
  float t, lo, hi;
  int32_t status, steps, bracketed;
};

__device__ __forceinline__ void trace_init_ray(TraceRay& r, float t0, float t1) {
  r.status = (t1 > t0) ? I2SDF_TRACE_ACTIVE : I2SDF_TRACE_MISS;      // a NaN bound compares false: MISS
  r.t = r.lo = r.hi = t0;
  r.steps = 0;
  r.bracketed = 0;
}

// f = sdf(o + r.t d) of an ACTIVE ray
__device__ __forceinline__ void trace_step_ray(TraceRay& r, float f, float t0, float t1, float eps, float step_scale) {
  // hipcc's default contracts a * b + c into one rounding -- also across __fadd_rn(.., __fmul_rn(..)), which are plain operators compiled
  // with that default -- so the rule is written with operators under a pragma that switches contraction off for this block
#pragma clang fp contract(off)
  r.steps += 1;
  if (!(f - f == 0.0f)) { r.status = I2SDF_TRACE_UNRESOLVED; return; }                  // 1. inf or NaN
  if (fabsf(f) <= eps) { r.status = I2SDF_TRACE_HIT; return; }                          // 2.
  if (f < 0.0f && r.steps == 1) { r.status = I2SDF_TRACE_INSIDE; r.t = t0; return; }    // 3.
  if (f < 0.0f) { r.hi = r.t; r.bracketed = 1; } else r.lo = r.t;                       // 4.
  float tn;
  if (r.bracketed) {                                                                    // 5.
    tn = r.lo + 0.5f * (r.hi - r.lo);
    if (tn == r.lo || tn == r.hi) { r.status = I2SDF_TRACE_HIT; r.t = r.hi; return; }
  } else {                                                                              // 6.
    tn = r.t + step_scale * f;
    if (tn >= t1) { r.status = I2SDF_TRACE_MISS; r.t = t1; return; }
  }
  r.t = tn;                                                                             // 7.
}

// The point of depth t: the same expression as fetch_point (mlp_common.h), so that the compiler forms it the same way in every kernel --
// hipcc contracts it: x = fma(t, d, o), ONE rounding per component, which is what include/i2sdf.h states for the traced points.
__device__ __forceinline__ void trace_point(const float* __restrict__ cam, const float* __restrict__ dirs, int64_t ray, float t, float& x,
                                            float& y, float& z) {
  x = __fadd_rn(cam[ray * 3 + 0], __fmul_rn(t, dirs[ray * 3 + 0]));
  y = __fadd_rn(cam[ray * 3 + 1], __fmul_rn(t, dirs[ray * 3 + 1]));
  z = __fadd_rn(cam[ray * 3 + 2], __fmul_rn(t, dirs[ray * 3 + 2]));
}

}  // namespace i2sdf
