// SDF network forward without gradient: ImplicitNetwork.forward / get_sdf_vals
// (model/network/mlp.py:84-105,145-151).  MFMA-bound: 2*524544 FLOP per point at synthetic.yml shapes.
#include "epi.h"
#include "mlp_args.h"

using namespace i2sdf;

namespace {

template <int H, int F, int LF, bool FULL>
__global__ __launch_bounds__(256) void sdf_fwd_kernel(const float* __restrict__ stream, int n_stages, int L, int skip, PointSpec ps,
                                                       const int* __restrict__ skip_flag, int64_t M, float* __restrict__ sdf_out,
                                                       float* __restrict__ feat_out, int64_t ld_feat) {
  constexpr int NT = H / 32, KC = H / 8, PEC = PE<LF>::PEC;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (skip_flag != nullptr && skip_flag[0] != 0) return;      // batch already converged (sampler)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5;
  const int64_t m = ((int64_t)blockIdx.x * 4 + wave) * 32 + (lane & 31);
  const bool valid = m < M;
  const int64_t mc = valid ? m : M - 1;
  float px, py, pz;
  fetch_point(ps, mc, px, py, pz);
  float pe[PEC * 4];
  {
    float full[PEC * 8];
    pe_full<LF>(px, py, pz, full);
    to_b_layout<PEC>(full, pe, hi);
  }
  WStream ws;
  ws.begin(stream, lds, n_stages, tid);
  f32x16 acc[NT];
  float h[NT * 16];
  SoftplusEpi sp{nullptr, hi, valid};
  dense_op_epi<NT, PEC, NT * 4, 0, 0, SoftplusEpi>(ws, pe, acc, sp, tid);
  commit_tiles<NT>(acc, h);
  for (int l = 1; l < L - 1; ++l) {
    if (l == skip) {
      constexpr float rs2 = RS2;
      float u[(KC + PEC) * 4];
#pragma unroll
      for (int i = 0; i < KC * 4; ++i) u[i] = h[i] * rs2;
#pragma unroll
      for (int i = 0; i < PEC * 4; ++i) u[KC * 4 + i] = pe[i] * rs2;
      dense_op_epi<NT, KC + PEC, NT * 4, 0, 0, SoftplusEpi>(ws, u, acc, sp, tid);
    } else {
      dense_op_epi<NT, KC, NT * 4, 0, 0, SoftplusEpi>(ws, h, acc, sp, tid);
    }
    commit_tiles<NT>(acc, h);
  }
  float s[1];
  rowvec_op<1, KC>(ws, h, s, tid);
  if (sdf_out != nullptr && valid && hi == 0) sdf_out[m] = s[0];
  if (FULL) {
    constexpr int FT = F / 32;
    f32x16 fa[FT];
    dense_op<FT, KC, 0>(ws, h, fa, tid);
    store_tile<FT>(feat_out + mc * ld_feat, hi, valid, fa);
  }
}

template <int H, int F, int LF>
int launch_sdf_fwd(const i2sdf_plan* p, const float* packed, PointSpec points, const int* skip_flag, int64_t M, float* sdf_out,
                   float* feat_out, int64_t ld_feat, hipStream_t st, bool sampler_pass = false) {
  const i2sdf_mlp_desc& d = p->sdf.d;
  const bool full = feat_out != nullptr;
  const unsigned grid = (unsigned)((M + PTS_PER_WG - 1) / PTS_PER_WG);
  const SdfFwdKind kind = sdf_fwd_kind(p);
  if (!full && sdf_out != nullptr && kind == SDF_FWD_X3H_256) {
    // the sampler's passes with two split planes under I2SDF_OPT_SAMPLER_BF16X2
    const int PL = (sampler_pass && p->sampler_bf16x2 && span_chunks(p->sdf, SPAN_FWD2H) > 0) ? 2 : 3;
    const Span s3 = span(p, packed, p->sdf, PL == 2 ? SPAN_FWD2H : SPAN_FWD3H_SDF);
    if (!s3.n_stages) return I2SDF_EINVAL;
    i2sdf_launch_sdf_fwd3h(s3.w, s3.n_stages, d.n_lin, d.skip_layer, points, skip_flag, M, sdf_out, PL, st);
    return i2sdf_hip_check(hipGetLastError(), "sdf_forward (bf16x3, 16-point waves) launch");
  }
  if (!full && sdf_out != nullptr && kind == SDF_FWD_X3_64) {
    const Span s3 = span(p, packed, p->sdf, SPAN_FWD3);
    if (!s3.n_stages) return I2SDF_EINVAL;
    i2sdf_launch_sdf_fwd3(H, s3.w, s3.n_stages, d.n_lin, d.skip_layer, points, skip_flag, M, sdf_out, grid, st);
    return i2sdf_hip_check(hipGetLastError(), "sdf_forward (bf16x3) launch");
  }
  if (full && kind == SDF_FWD_X3H_256) {
    // [sdf | feature] rows (ImplicitNetwork.forward: the meshing callers, model/eval/recon.py:51,90, utils/plots.py:52): the 16-point-wave
    // forward of the training path without its saves -- the same kernel, so the 257 columns are the values a training step computes
    const Span s3 = span(p, packed, p->sdf, SPAN_FWD3H);
    if (!s3.n_stages || skip_flag != nullptr) return I2SDF_EINVAL;      // (the sampler never asks for features)
    SdfTrainFwdArgs a{};
    a.fwd = s3.w; a.n_fwd = s3.n_stages;
    a.L = d.n_lin; a.skip = d.skip_layer; a.pts = points; a.M = M; a.Mp = M; a.sdf = sdf_out; a.feat = feat_out; a.ldf = ld_feat;
    i2sdf_launch_train_fwd3h(a, grid, st);
    return i2sdf_hip_check(hipGetLastError(), "sdf_forward (features, bf16x3, 16-point waves) launch");
  }
  const Span s = span(p, packed, p->sdf, full ? SPAN_FWD : SPAN_FWD_SDF);
  if (!s.n_stages) return I2SDF_EINVAL;
  if (full)
    launch_lds(sdf_fwd_kernel<H, F, LF, true>, grid, st, s.w, s.n_stages, d.n_lin, d.skip_layer, points, skip_flag, M, sdf_out, feat_out, ld_feat);
  else
    launch_lds(sdf_fwd_kernel<H, F, LF, false>, grid, st, s.w, s.n_stages, d.n_lin, d.skip_layer, points, skip_flag, M, sdf_out, nullptr, 0);
  return i2sdf_hip_check(hipGetLastError(), "sdf_forward launch");
}

}  // namespace

extern "C" int i2sdf_sdf_forward(const i2sdf_plan* p, const float* packed, const float* points, int64_t M, float* sdf_out,
                                 float* feat_out, int64_t ld_feat, void* stream) {
  if (M == 0) return I2SDF_OK;                 // empty batch: nothing to validate, nothing to launch
  if (!p || !packed || !points || M < 0) return I2SDF_EINVAL;
  if (feat_out && (ld_feat < p->F || ld_feat % 4)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (p->sdf.d.multires != 6) return I2SDF_EINVAL;
  const PointSpec ps{points, nullptr, nullptr, nullptr, 0, 0, 1};
  if (p->H == 256 && p->F == 256) return launch_sdf_fwd<256, 256, 6>(p, packed, ps, nullptr, M, sdf_out, feat_out, ld_feat, st);
  if (p->H == 64 && p->F == 64) return launch_sdf_fwd<64, 64, 6>(p, packed, ps, nullptr, M, sdf_out, feat_out, ld_feat, st);
  return I2SDF_EINVAL;
}

// internal (mlp_args.h): the sampler's passes and the stepwise tracer's
int i2sdf_sdf_forward_rays_flagged(const i2sdf_plan* p, const float* packed, const float* cam, const float* dirs, const float* z, int64_t ldz,
                                   int32_t n_per_ray, int64_t B, float* sdf_out, const int* skip_flag, bool sampler_pass, void* stream) {
  if (p->sdf.d.multires != 6) return I2SDF_EINVAL;
  const int64_t M = B * n_per_ray;
  const PointSpec ps{nullptr, cam, dirs, z, ldz, M, n_per_ray};
  hipStream_t st = (hipStream_t)stream;
  if (p->H == 256 && p->F == 256) return launch_sdf_fwd<256, 256, 6>(p, packed, ps, skip_flag, M, sdf_out, nullptr, 0, st, sampler_pass);
  if (p->H == 64 && p->F == 64) return launch_sdf_fwd<64, 64, 6>(p, packed, ps, skip_flag, M, sdf_out, nullptr, 0, st, sampler_pass);
  return I2SDF_EINVAL;
}
