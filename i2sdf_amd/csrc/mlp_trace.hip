// Sphere tracing of the SDF's zero level (include/i2sdf.h: i2sdf_trace_rays; the rule itself: trace_rule.h).
// Stepwise route: trace_init once, then per step the sdf-only forward on the ray-form points x = cam + t * dirs (PointSpec with one point
// per ray and z = t_out, so the points are formed by fetch_point as everywhere else) and trace_step, which applies the rule to the f the
// forward wrote.  Everything is stream ordered; a finished ray keeps its t and is still evaluated (its f is ignored).
// Fused route (bf16x3 plans): ONE kernel whose workgroup keeps its 128 rays for the whole march -- sdf_trace3_kernel follows the body of
// sdf_fwd3_kernel (mlp_x3.hip, 64-wide nets, 32-point waves), sdf_trace3h_kernel that of sdf_fwd3h_kernel (mlp_x3h.hip, 256-wide nets,
// 16-point waves, three planes).  Every pass re-forms the points, rebuilds the encoding, RESTARTS the weight stream and runs the layer chain
// and the row vector, then applies the rule in registers; the workgroup leaves when a block-wide vote finds no ACTIVE ray.
// Built with the lifted unroll cap as the other bf16x3 units are (build.sh).
#define I2SDF_RELU_ASM 1      // common.h: relu0, as mlp_x3.hip / mlp_x3h.hip (the forward passes must give their bits)
#include <cmath>
#include <string>
#include "mlp_args.h"
#include "x3h.h"
#include "trace_rule.h"

using namespace i2sdf;

namespace {

constexpr int TRACE_THREADS = 256;

// workspace: f (N) | lo (N) | hi (N) | bracketed (N, int32)
struct TraceState {
  float* t; int32_t* status; int32_t* steps;
  float* f; float* lo; float* hi; int32_t* bracketed;
};

__global__ __launch_bounds__(TRACE_THREADS) void trace_init_kernel(TraceState s, const float* __restrict__ t_min, const float* __restrict__ t_max,
                                                                   int64_t N) {
  const int64_t r = (int64_t)blockIdx.x * TRACE_THREADS + threadIdx.x;
  if (r >= N) return;
  TraceRay ray;
  trace_init_ray(ray, t_min[r], t_max[r]);
  s.t[r] = ray.t; s.lo[r] = ray.lo; s.hi[r] = ray.hi;
  s.status[r] = ray.status; s.steps[r] = ray.steps; s.bracketed[r] = ray.bracketed;
}

// step `step` (0-based) of every ray that is still ACTIVE; LAST: what is ACTIVE after it ends UNRESOLVED
__global__ __launch_bounds__(TRACE_THREADS) void trace_step_kernel(TraceState s, const float* __restrict__ t_min, const float* __restrict__ t_max,
                                                                   int64_t N, float eps, float step_scale, int32_t step, int32_t last,
                                                                   float* __restrict__ f_trace) {
  const int64_t r = (int64_t)blockIdx.x * TRACE_THREADS + threadIdx.x;
  if (r >= N) return;
  TraceRay ray;
  ray.status = s.status[r];
  if (ray.status != I2SDF_TRACE_ACTIVE) return;
  ray.t = s.t[r]; ray.lo = s.lo[r]; ray.hi = s.hi[r]; ray.steps = s.steps[r]; ray.bracketed = s.bracketed[r];
  const float f = s.f[r];
  if (f_trace != nullptr) f_trace[(int64_t)step * N + r] = f;
  trace_step_ray(ray, f, t_min[r], t_max[r], eps, step_scale);
  if (last && ray.status == I2SDF_TRACE_ACTIVE) ray.status = I2SDF_TRACE_UNRESOLVED;
  s.t[r] = ray.t; s.lo[r] = ray.lo; s.hi[r] = ray.hi;
  s.status[r] = ray.status; s.steps[r] = ray.steps; s.bracketed[r] = ray.bracketed;
}

struct TraceArgs {
  const float *cam, *dirs, *t_min, *t_max;
  int64_t N;
  float* t; int32_t* status; int32_t* steps; float* f_trace;
  float eps, step_scale; int32_t max_steps;
};

// The restart of the weight stream is the hazard of the loop: begin() DMAs the first stage into buffer 0 at once, and the previous pass
// ends with LDS reads of its last stages (the row vector) and, in the K-outer ops, with a harmless re-fetch into the idle buffer.  Every
// wave must be past its last LDS read before any wave issues that DMA: the vote at the top of the loop is a workgroup barrier behind
// s_waitcnt lgkmcnt(0) (and the value voted on depends on those reads), and the explicit __syncthreads() in front of begin() states
// it where it matters.  DMAs of one wave into one LDS address land in issue order, and the first stage wait of a pass is a full drain
// (advance_barrier), so the stale re-fetch cannot outlive the new first stage.  The counted stage waits only ever see MORE outstanding
// vector-memory instructions than they count (the rule's loads and stores in front of begin()): they then wait longer, never shorter.
template <int H, int LF>
__global__ __launch_bounds__(256) void sdf_trace3_kernel(const float* __restrict__ stream, int n_stages, int L, int skip, TraceArgs a) {
  constexpr int NT = H / 32, KC = H / 8, KH16 = H / 16, PED = PE<LF>::DIM, PE16 = cdiv(PED, 16), NPE = PE16 * 8;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
  const int64_t m = ((int64_t)blockIdx.x * 4 + wave) * 32 + (lane & 31);
  const bool valid = m < a.N;
  const int64_t mc = valid ? m : a.N - 1;
  const float t0 = a.t_min[mc], t1 = a.t_max[mc];
  TraceRay ray;                                    // both halves of the wave hold the ray of their point and step it alike
  trace_init_ray(ray, t0, t1);
  if (!valid) ray.status = I2SDF_TRACE_MISS;       // a padding lane never votes
  for (int step = 0; step < a.max_steps; ++step) {
    if (!__syncthreads_or(ray.status == I2SDF_TRACE_ACTIVE)) break;
    float px, py, pz;
    trace_point(a.cam, a.dirs, mc, ray.t, px, py, pz);
    float pe[NPE];
    {
      float full[PE<LF>::PEC * 8], pad[PE16 * 16];
      pe_full<LF>(px, py, pz, full);
#pragma unroll
      for (int i = 0; i < PE16 * 16; ++i) pad[i] = (i < PED) ? full[i] : 0.f;
      x3_select_pe<PE16>(pad, pe, hi);
    }
    __syncthreads();                               // (see above: nobody reads the stage buffers any more)
    WStream ws;
    ws.begin(stream, lds, n_stages, tid);
    f32x16 accP[NT], accN[NT];
    {
      X3FwdSrc<NT, 0, NPE, false> src{accN, pe, nullptr, hi, valid};
      dense_x3g<NT, PE16, 1>(ws, src, accP, tid);
    }
    for (int l = 1; l < L - 1; ++l) {
      X3FwdSrc<NT, KH16, NPE, false> src{accP, pe, nullptr, hi, valid};
      if (l == skip) dense_x3g<NT, KH16 + PE16, 1>(ws, src, accN, tid);
      else dense_x3g<NT, KH16, 1>(ws, src, accN, tid);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) accP[nt] = accN[nt];
    }
    float h[NT * 16];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) h[nt * 16 + r] = softplus100(accP[nt][r]);
    float s[1];
    rowvec_op<1, KC>(ws, h, s, tid);
    if (ray.status == I2SDF_TRACE_ACTIVE) {
      if (a.f_trace != nullptr && hi == 0) a.f_trace[(int64_t)step * a.N + m] = s[0];
      trace_step_ray(ray, s[0], t0, t1, a.eps, a.step_scale);
    }
  }
  if (ray.status == I2SDF_TRACE_ACTIVE) ray.status = I2SDF_TRACE_UNRESOLVED;
  if (valid && hi == 0) { a.t[m] = ray.t; a.status[m] = ray.status; a.steps[m] = ray.steps; }
}

// The 256-wide kernel sits at the 256-register cap of its family (two waves per SIMD): a ray's state lives in LDS between the rule and
// the next pass, not in registers across the layer chain (kept there it cost 14 spilled registers).  A wave reads and writes only the
// rows of its own 16 rays, the four lanes of a ray the same values, and LDS operations of one wave execute in issue order.
struct TraceLds { float t[128], lo[128], hi[128]; int32_t status[128], steps[128], bracketed[128]; };
__device__ __forceinline__ void trace_lds_put(TraceLds& s, int i, const TraceRay& r) {
  s.t[i] = r.t; s.lo[i] = r.lo; s.hi[i] = r.hi; s.status[i] = r.status; s.steps[i] = r.steps; s.bracketed[i] = r.bracketed;
}
__device__ __forceinline__ void trace_lds_get(const TraceLds& s, int i, TraceRay& r) {
  r.t = s.t[i]; r.lo = s.lo[i]; r.hi = s.hi[i]; r.status = s.status[i]; r.steps = s.steps[i]; r.bracketed = s.bracketed[i];
}

template <int H, int LF, int NW>
__global__ __launch_bounds__(NW * 64, 2) void sdf_trace3h_kernel(const float* __restrict__ stream, int n_stages, int L, int skip, TraceArgs a) {
  constexpr int NT = H / 16, KH32 = H / 32, PED = PE<LF>::DIM, PE32 = cdiv(PED, 32), NPE = PE32 * 8;
  static_assert(NW * HP == 128, "TraceLds holds the 128 rays of a workgroup");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ TraceLds st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kg = lane >> 4;
  const int rl = wave * HP + (lane & 15);          // this lane's ray within the workgroup
  {
    const int64_t m = (int64_t)blockIdx.x * (NW * HP) + rl;
    const int64_t mc = m < a.N ? m : a.N - 1;
    TraceRay ray;
    trace_init_ray(ray, a.t_min[mc], a.t_max[mc]);
    if (m >= a.N) ray.status = I2SDF_TRACE_MISS;   // a padding lane never votes
    trace_lds_put(st, rl, ray);
  }
  for (int step = 0; step < a.max_steps; ++step) {
    if (!__syncthreads_or(st.status[rl] == I2SDF_TRACE_ACTIVE)) break;
    const int64_t m = (int64_t)blockIdx.x * (NW * HP) + rl;
    const bool valid = m < a.N;
    const int64_t mc = valid ? m : a.N - 1;
    float pe[NPE];
    {
      float px, py, pz;
      trace_point(a.cam, a.dirs, mc, st.t[rl], px, py, pz);
      float full[PE<LF>::PEC * 8], pad[PE32 * 32];
      pe_full<LF>(px, py, pz, full);
#pragma unroll
      for (int i = 0; i < PE32 * 32; ++i) pad[i] = (i < PED) ? full[i < PE<LF>::PEC * 8 ? i : 0] : 0.f;
      x3h_select<PE32>(pad, pe, kg);
    }
    __syncthreads();                               // (see sdf_trace3_kernel: nobody reads the stage buffers any more)
    WStreamH<NW> ws;
    ws.begin(stream, lds, n_stages, tid);
    f32x4 accP[NT], accN[NT];
    {
      XhFwdSrc<NT, 0, NPE, false> src{accN, pe, nullptr, kg, valid};
      dense_x3h<NT, PE32, 1, NW, XhFwdSrc<NT, 0, NPE, false>, 3>(ws, src, accP, tid);
    }
    for (int l = 1; l < L - 1; ++l) {
      XhFwdSrc<NT, KH32, NPE, false> src{accP, pe, nullptr, kg, valid};
      if (l == skip) dense_x3h<NT, KH32 + PE32, 1, NW, XhFwdSrc<NT, KH32, NPE, false>, 3>(ws, src, accN, tid);
      else dense_x3h<NT, KH32, 1, NW, XhFwdSrc<NT, KH32, NPE, false>, 3>(ws, src, accN, tid);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) accP[nt] = accN[nt];
    }
    float h[NT * 4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) h[nt * 4 + r] = softplus100(accP[nt][r]);
    float s[1];
    rowvec_h<1, NT, NW>(ws, h, s, tid);
    if (st.status[rl] == I2SDF_TRACE_ACTIVE) {
      TraceRay ray;
      trace_lds_get(st, rl, ray);
      if (a.f_trace != nullptr && kg == 0) a.f_trace[(int64_t)step * a.N + m] = s[0];
      trace_step_ray(ray, s[0], a.t_min[mc], a.t_max[mc], a.eps, a.step_scale);
      trace_lds_put(st, rl, ray);
    }
  }
  const int64_t m = (int64_t)blockIdx.x * (NW * HP) + rl;
  if (m < a.N && kg == 0) {
    TraceRay ray;
    trace_lds_get(st, rl, ray);
    if (ray.status == I2SDF_TRACE_ACTIVE) ray.status = I2SDF_TRACE_UNRESOLVED;
    a.t[m] = ray.t; a.status[m] = ray.status; a.steps[m] = ray.steps;
  }
}

// which fused kernel the plan has: 0 none, 64 / 256 the width it is built for -- they follow the bf16x3 sdf-only forwards
int fused_kind(const i2sdf_plan* p) {
  const SdfFwdKind kind = sdf_fwd_kind(p);
  return kind == SDF_FWD_X3H_256 ? 256 : kind == SDF_FWD_X3_64 ? 64 : 0;
}

int trace_fused(const i2sdf_plan* p, const float* packed, const TraceArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)((a.N + PTS_PER_WG - 1) / PTS_PER_WG);
  const i2sdf_mlp_desc& d = p->sdf.d;
  if (fused_kind(p) == 256) {
    const Span s3 = span(p, packed, p->sdf, SPAN_FWD3H_SDF);
    if (!s3.n_stages) return I2SDF_EINVAL;
    launch_lds_threads(512, sdf_trace3h_kernel<256, 6, 8>, grid, st, s3.w, s3.n_stages, d.n_lin, d.skip_layer, a);
  } else {
    const Span s3 = span(p, packed, p->sdf, SPAN_FWD3);
    if (!s3.n_stages) return I2SDF_EINVAL;
    launch_lds(sdf_trace3_kernel<64, 6>, grid, st, s3.w, s3.n_stages, d.n_lin, d.skip_layer, a);
  }
  return i2sdf_hip_check(hipGetLastError(), "trace_rays: fused launch");
}

int refuse(const std::string& why) { return i2sdf_refuse(("i2sdf_trace_rays: " + why).c_str()); }

}  // namespace

extern "C" int64_t i2sdf_trace_workspace_floats(int64_t N) { return N < 0 ? 0 : 4 * N; }

extern "C" int i2sdf_trace_rays(const i2sdf_plan* p, const float* packed, const i2sdf_trace_cfg* cfg, const float* cam, const float* dirs,
                                const float* t_min, const float* t_max, int64_t N, float* t_out, int32_t* status_out, int32_t* steps_out,
                                float* f_trace, float* workspace, void* stream) {
  if (!cfg) return refuse("cfg is NULL");
  if (!(cfg->eps > 0.0f) || !std::isfinite(cfg->eps)) return refuse("eps = " + std::to_string(cfg->eps) + " must be positive and finite");
  if (!(cfg->step_scale > 0.0f && cfg->step_scale <= 1.0f)) return refuse("step_scale = " + std::to_string(cfg->step_scale) + " is outside (0, 1]");
  if (cfg->max_steps < 1 || cfg->max_steps > I2SDF_TRACE_MAX_STEPS)
    return refuse("max_steps = " + std::to_string(cfg->max_steps) + " is outside 1.." + std::to_string(I2SDF_TRACE_MAX_STEPS));
  if (cfg->route != I2SDF_TRACE_AUTO && cfg->route != I2SDF_TRACE_STEPWISE && cfg->route != I2SDF_TRACE_FUSED)
    return refuse("route = " + std::to_string(cfg->route) + " is none of 0 (auto), 1 (stepwise), 2 (fused)");
  if (N < 0) return refuse("N = " + std::to_string(N) + " < 0");
  if (!p) return refuse("plan is NULL");
  if (cfg->route == I2SDF_TRACE_FUSED && fused_kind(p) == 0)
    return refuse("route 2 (fused): this plan has no fused trace kernel (they follow the bf16x3 sdf-only forwards: I2SDF_OPT_SDF_FWD_BF16X3)");
  if (N == 0) return I2SDF_OK;
  if (!packed || !cam || !dirs || !t_min || !t_max || !t_out || !status_out || !steps_out || !workspace)
    return refuse("a required pointer is NULL (packed, cam, dirs, t_min, t_max, t_out, status_out, steps_out, workspace)");
  if (N >= ((int64_t)1 << 31)) return refuse("N = " + std::to_string(N) + " >= 2^31");
  hipStream_t st = (hipStream_t)stream;
  // route 0 takes the fused kernel where the plan has one: 37.0 against 79.5 ms at 307 200 rays, no slower at 1024 (profiles/trace_timing.json)
  if (cfg->route == I2SDF_TRACE_FUSED || (cfg->route == I2SDF_TRACE_AUTO && fused_kind(p) != 0)) {
    const TraceArgs a{cam, dirs, t_min, t_max, N, t_out, status_out, steps_out, f_trace, cfg->eps, cfg->step_scale, cfg->max_steps};
    return trace_fused(p, packed, a, st);
  }
  TraceState s{t_out, status_out, steps_out, workspace, workspace + N, workspace + 2 * N, reinterpret_cast<int32_t*>(workspace + 3 * N)};
  const unsigned grid = (unsigned)((N + TRACE_THREADS - 1) / TRACE_THREADS);
  trace_init_kernel<<<grid, TRACE_THREADS, 0, st>>>(s, t_min, t_max, N);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "trace_rays: init launch")) return rc;
  for (int32_t step = 0; step < cfg->max_steps; ++step) {
    // the sdf-only forward of i2sdf_sdf_forward on the points cam + t * dirs: three planes, never the sampler's two
    if (int rc = i2sdf_sdf_forward_rays_flagged(p, packed, cam, dirs, t_out, 1, 1, N, s.f, nullptr, false, (void*)st))
      return rc == I2SDF_EINVAL ? i2sdf_refuse("i2sdf_trace_rays: the plan's SDF net has no sdf-only forward kernel") : rc;
    trace_step_kernel<<<grid, TRACE_THREADS, 0, st>>>(s, t_min, t_max, N, cfg->eps, cfg->step_scale, step, step == cfg->max_steps - 1, f_trace);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "trace_rays: step launch")) return rc;
  }
  return I2SDF_OK;
}
