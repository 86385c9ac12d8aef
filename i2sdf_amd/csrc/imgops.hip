// Rendered views on the device: what VolumeRenderSystem.test_step / ViewInterpolateSystem.test_step (model/eval/recon.py) do with a
// finished view -- PSNR (utils/rend_util.py:get_psnr), SSIM (torchmetrics 0.11.4, restated from its source), the camera-space normal
// map and the 8-bit frames handed to the image writers (utils/plots.py).  Nothing is written to a file here.
//
// Layout: the render outputs' own.  Pixel-major, channel-last fp32, (n_views, H W, C) contiguous, pixel p = y W + x; C = 3 for rgb and
// normals, 1 for depth.  No transposes, no padded copies, no allocation; every call only enqueues.
//
// image_stats   per view, one pass: sse = sum over the 3 H W values of ((double)pred - (double)gt)^2 (exact differences of fp32 numbers,
//               fp64 squares and sums), min / max of pred and of gt, max of depth (fminf / fmaxf: a NaN is passed over).
//               Every workgroup strides over its view, a thread sums its own values in index order, the 64 lanes of a wave are
//               combined by an xor butterfly, the 4 waves in wave order, and the workgroup writes slot (view, workgroup) of the
//               workspace.  im_stats_finish adds a view's slots in a fixed order (ordered_sum below).  No floating-point atomics.
// image_ssim    per view the mean over (H - 10) x (W - 10) x 3 of
//                 ssim = ((2 E[p] E[t] + c1) (2 s_pt + c2)) / ((E[p]^2 + E[t]^2 + c1) (s_p + s_t + c2)),
//                 s_p = E[pp] - E[p]^2, s_t = E[tt] - E[t]^2, s_pt = E[pt] - E[p] E[t], c1 = (0.01 R)^2, c2 = (0.03 R)^2,
//               E[.] under the separable 11-tap Gaussian g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum (fp64 on the host, rounded to fp32),
//               for the pixels whose window lies inside the image: torchmetrics reflect-pads by 5 and crops 5 from the result, so no
//               padded value ever reaches the mean.  R = data_range, or when that is NaN max(max p - min p, max t - min t) of the view
//               in fp32 from the stats above (torchmetrics' data_range=None for a batch of one view).  c1, c2: fp64 from the fp32 R,
//               rounded to fp32.
//               Arithmetic: fp32, every product and sum rounded on its own.  Horizontal pass m_h = sum_k g[k] v[x + k], k ascending,
//               for v in (p, t, p p, t t, p t); vertical pass sum_j g[j] m_h[y + j], j ascending; then the formula as written.
//               One workgroup per I2SDF_SSIM_TILE_Y x I2SDF_SSIM_TILE_X (16 x 32) tile of the output and view: the 26 x 42 pixel
//               block of both images is staged in LDS as it lies in memory (rows of 126 interleaved floats, coalesced loads, zeros
//               outside the image), then per channel the horizontal pass goes to LDS and the vertical pass runs in registers (a
//               lane owns one column and two rows).  A thread adds its 6 values in fp64, lanes and waves are combined as above, the
//               workgroup writes slot (view, tile); im_ssim_finish adds them with ordered_sum and divides.  The optional map is
//               written by the same code path, so the mean does not depend on whether it was asked for.
// image_frames  elementwise, one lane per pixel, every output optional:
//                 rgb8    = trunc(clip(rgb * 255, 0, 255))                                         (plots.py:500-501, recon.py:273)
//                 n_cam_k = (R[0][k] n_0 + R[1][k] n_1) + R[2][k] n_2, R = pose[:3, :3]            (recon.py:184-186: R^T n)
//                           in fp64 (exact products of fp32 numbers), rounded to fp32 once: half an ulp of the value plus the
//                           2^-52-relative roundings of the two fp64 sums, also where the sum cancels
//                 normal8 = trunc(clip(((n_cam + 1) * 0.5) * 255, 0, 255))                         (recon.py:189-190, :280)
//                 depth8  = trunc(clip((d / (max_view(d) + 1e-6f)) * 255, 0, 255))                 (plots.py:551-552; the clip only
//                           matters for d < 0, where the reference's cast is undefined)
//                 depth_rgb8 = lut[depth8]                                                          (the caller's colour map)
//               A NaN becomes 0.
// linear_to_srgb  (i2sdf_linear_to_srgb) elementwise tone map of HDR validation views (utils/rend_util.py:linear_to_srgb behind an optional clamp to [0, 1]),
//               one lane per value, in place allowed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using i2sdf_blockops::wave_max;
using i2sdf_blockops::wave_min;
using i2sdf_blockops::wave_sum;

constexpr int IM_THREADS = 256;
constexpr int IM_WAVES = IM_THREADS / 64;
constexpr int IM_STAT_PIXELS = 1024;             // pixels per stats workgroup until IM_STAT_MAX workgroups per view are reached
constexpr int IM_STAT_MAX = 128;
constexpr int IM_STAT_SLOT = 6;                  // doubles per stats slot: sse, min p, max p, min t, max t, max depth
constexpr int TX = I2SDF_SSIM_TILE_X, TY = I2SDF_SSIM_TILE_Y;
constexpr int WIN = 11, HALO = WIN - 1;
constexpr int BX = TX + HALO, BY = TY + HALO;    // staged pixel block
constexpr int ROWF = 3 * BX;                     // floats per staged row
constexpr int ROWS_PER_LANE = TY * TX / IM_THREADS;
static_assert(TX == 32 && ROWS_PER_LANE * IM_THREADS == TY * TX, "the vertical pass maps a lane to column tid % 32");

struct Taps {
  float g[WIN];
};

struct Plan {
  int sb;                                        // stats workgroups (= slots) per view
  int tiles_x;
  int64_t tiles;                                 // SSIM tiles (= slots) per view, 0 below 11 x 11
  int64_t off_ssim, bytes;
};

bool plan(int32_t n_views, int32_t H, int32_t W, Plan& P) {
  if (n_views < 1 || n_views > 65535 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX) return false;
  const int64_t hw = (int64_t)H * W, sb = (hw + IM_STAT_PIXELS - 1) / IM_STAT_PIXELS;
  P.sb = (int)(sb < IM_STAT_MAX ? sb : IM_STAT_MAX);
  P.tiles_x = W >= WIN ? (W - HALO + TX - 1) / TX : 0;
  P.tiles = H >= WIN ? (int64_t)P.tiles_x * ((H - HALO + TY - 1) / TY) : 0;
  P.off_ssim = (int64_t)n_views * P.sb * IM_STAT_SLOT * 8;
  P.bytes = P.off_ssim + (int64_t)n_views * P.tiles * 8;      // (monotone in n_views, H and W)
  return true;
}

// One wave.  The n slots are cut into 64 runs of ceil(n / 64) consecutive slots; lane l adds run l in index order, lane 0 adds the 64
// run sums in lane order.  `stride` doubles between slots.  The result is valid in lane 0.
__device__ double ordered_sum(const double* __restrict__ slots, int64_t n, int stride, double* lds) {
  const int lane = threadIdx.x;
  const int64_t per = (n + 63) / 64, lo = lane * per, hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) s += slots[i * stride];
  lds[lane] = s;
  __syncthreads();
  double t = 0.0;
  if (lane == 0)
    for (int l = 0; l < 64; ++l) t += lds[l];
  return t;
}

__global__ __launch_bounds__(IM_THREADS) void im_stats(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const float* __restrict__ depth, int64_t hw, double* __restrict__ part) {
  __shared__ double red[IM_WAVES][IM_STAT_SLOT];
  const int v = blockIdx.y, sb = gridDim.x;
  const int64_t first = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, step = (int64_t)sb * IM_THREADS;
  double sse = 0.0;
  float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY, dmax = -INFINITY;
  if (pred) {
    const int64_t n3 = 3 * hw;
    const float* p = pred + (int64_t)v * n3;
    const float* t = gt + (int64_t)v * n3;
    for (int64_t i = first; i < n3; i += step) {
      const float a = p[i], b = t[i];
      const double d = (double)a - (double)b;
      sse += d * d;
      pmin = fminf(pmin, a); pmax = fmaxf(pmax, a);
      tmin = fminf(tmin, b); tmax = fmaxf(tmax, b);
    }
  }
  if (depth) {
    const float* d = depth + (int64_t)v * hw;
    for (int64_t i = first; i < hw; i += step) dmax = fmaxf(dmax, d[i]);
  }
  sse = wave_sum(sse);
  pmin = wave_min(pmin); pmax = wave_max(pmax);
  tmin = wave_min(tmin); tmax = wave_max(tmax);
  dmax = wave_max(dmax);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = sse; red[wave][1] = pmin; red[wave][2] = pmax; red[wave][3] = tmin; red[wave][4] = tmax; red[wave][5] = dmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double o[IM_STAT_SLOT];
#pragma unroll
    for (int k = 0; k < IM_STAT_SLOT; ++k) o[k] = red[0][k];
    for (int w = 1; w < IM_WAVES; ++w) {
      o[0] += red[w][0];
      o[1] = fmin(o[1], red[w][1]); o[2] = fmax(o[2], red[w][2]);
      o[3] = fmin(o[3], red[w][3]); o[4] = fmax(o[4], red[w][4]);
      o[5] = fmax(o[5], red[w][5]);
    }
    double* dst = part + ((int64_t)v * sb + blockIdx.x) * IM_STAT_SLOT;
#pragma unroll
    for (int k = 0; k < IM_STAT_SLOT; ++k) dst[k] = o[k];
  }
}

// one wave per view
__global__ __launch_bounds__(64) void im_stats_finish(const double* __restrict__ part, int sb, double* __restrict__ stats) {
  __shared__ double lds[64];
  const int v = blockIdx.x, lane = threadIdx.x;
  const double* slots = part + (int64_t)v * sb * IM_STAT_SLOT;
  const double sse = ordered_sum(slots, sb, IM_STAT_SLOT, lds);
  float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY, dmax = -INFINITY;
  for (int i = lane; i < sb; i += 64) {
    const double* s = slots + (int64_t)i * IM_STAT_SLOT;
    pmin = fminf(pmin, (float)s[1]); pmax = fmaxf(pmax, (float)s[2]);
    tmin = fminf(tmin, (float)s[3]); tmax = fmaxf(tmax, (float)s[4]);
    dmax = fmaxf(dmax, (float)s[5]);
  }
  pmin = wave_min(pmin); pmax = wave_max(pmax);
  tmin = wave_min(tmin); tmax = wave_max(tmax);
  dmax = wave_max(dmax);
  if (lane == 0) {
    double* o = stats + (int64_t)v * I2SDF_IMAGE_STATS;
    o[0] = sse; o[1] = pmin; o[2] = pmax; o[3] = tmin; o[4] = tmax; o[5] = dmax; o[6] = 0.0; o[7] = 0.0;
  }
}

__global__ __launch_bounds__(IM_THREADS) void im_ssim(const float* __restrict__ pred, const float* __restrict__ gt, int H, int W,
                                                      int tiles_x, Taps G, float data_range, const double* __restrict__ stats,
                                                      double* __restrict__ part, float* __restrict__ map) {
  __shared__ float raw[2][BY][ROWF];
  __shared__ float hb[5][BY][TX];
  __shared__ double red[IM_WAVES];
  const int tid = threadIdx.x, v = blockIdx.y;
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x0 = tx * TX, y0 = ty * TY, OW = W - HALO, OH = H - HALO;
  const int64_t base = (int64_t)v * H * W * 3;
  const int row_floats = 3 * W, xf0 = 3 * x0;
  for (int i = tid; i < BY * ROWF; i += IM_THREADS) {
    const int r = i / ROWF, j = i - r * ROWF;
    const int y = y0 + r, xf = xf0 + j;
    float a = 0.0f, b = 0.0f;
    if (y < H && xf < row_floats) {
      const int64_t idx = base + (int64_t)y * row_floats + xf;
      a = pred[idx];
      b = gt[idx];
    }
    raw[0][r][j] = a;
    raw[1][r][j] = b;
  }
  float R = data_range;
  if (R != R) {
    const double* s = stats + (int64_t)v * I2SDF_IMAGE_STATS;
    R = fmaxf((float)s[2] - (float)s[1], (float)s[4] - (float)s[3]);
  }
  const float c1 = (float)((0.01 * (double)R) * (0.01 * (double)R)), c2 = (float)((0.03 * (double)R) * (0.03 * (double)R));
  const int x = tid & (TX - 1), yl = (tid / TX) * ROWS_PER_LANE;
  double acc = 0.0;
  __syncthreads();
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < BY * TX; i += IM_THREADS) {
      const int r = i / TX, q = i - r * TX;
      float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const float a = raw[0][r][3 * (q + k) + c], b = raw[1][r][3 * (q + k) + c], g = G.g[k];
        m[0] += g * a;
        m[1] += g * b;
        m[2] += g * (a * a);
        m[3] += g * (b * b);
        m[4] += g * (a * b);
      }
#pragma unroll
      for (int u = 0; u < 5; ++u) hb[u][r][q] = m[u];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROWS_PER_LANE; ++q) {
      const int yy = yl + q;
      float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < WIN; ++j) {
        const float g = G.g[j];
#pragma unroll
        for (int u = 0; u < 5; ++u) m[u] += g * hb[u][yy + j][x];
      }
      const float pp = m[0] * m[0], tt = m[1] * m[1], pt = m[0] * m[1];
      const float sp = m[2] - pp, st = m[3] - tt, spt = m[4] - pt;
      const float upper = 2.0f * spt + c2, lower = (sp + st) + c2;
      const float s = ((2.0f * pt + c1) * upper) / (((pp + tt) + c1) * lower);
      const int ox = x0 + x, oy = y0 + yy;
      if (ox < OW && oy < OH) {
        acc += (double)s;
        if (map) map[(((int64_t)v * OH + oy) * OW + ox) * 3 + c] = s;
      }
    }
    __syncthreads();
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < IM_WAVES; ++w) t += red[w];
    part[(int64_t)v * gridDim.x + tile] = t;
  }
}

// one wave per view
__global__ __launch_bounds__(64) void im_ssim_finish(const double* __restrict__ part, int64_t tiles, double count, double* __restrict__ out) {
  __shared__ double lds[64];
  const int v = blockIdx.x;
  const double t = ordered_sum(part + (int64_t)v * tiles, tiles, 1, lds);
  if (threadIdx.x == 0) out[v] = t / count;
}

struct Frames {
  const float *rgb, *normal, *depth, *pose;
  const double* stats;
  const uint8_t* lut;
  uint8_t *rgb8, *normal8, *depth8, *depth_rgb8;
  float* ncam;
  int64_t hw;
};

__device__ __forceinline__ uint8_t to_u8(float x) { return (uint8_t)(int)fminf(fmaxf(x, 0.0f), 255.0f); }

__global__ __launch_bounds__(IM_THREADS) void im_frames(Frames A) {
  const int64_t p = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (p >= A.hw) return;
  const int v = blockIdx.y;
  const int64_t i = (int64_t)v * A.hw + p;
  if (A.rgb8) {
#pragma unroll
    for (int k = 0; k < 3; ++k) A.rgb8[3 * i + k] = to_u8(A.rgb[3 * i + k] * 255.0f);
  }
  if (A.normal8 || A.ncam) {
    const float* P = A.pose + 16 * (int64_t)v;
    const float n0 = A.normal[3 * i], n1 = A.normal[3 * i + 1], n2 = A.normal[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float c = (float)(((double)P[k] * n0 + (double)P[4 + k] * n1) + (double)P[8 + k] * n2);
      if (A.ncam) A.ncam[3 * i + k] = c;
      if (A.normal8) A.normal8[3 * i + k] = to_u8(((c + 1.0f) * 0.5f) * 255.0f);
    }
  }
  if (A.depth8 || A.depth_rgb8) {
    const float m = (float)A.stats[(int64_t)v * I2SDF_IMAGE_STATS + 5] + 1e-6f;
    const uint8_t d8 = to_u8((A.depth[i] / m) * 255.0f);
    if (A.depth8) A.depth8[i] = d8;
    if (A.depth_rgb8) {
#pragma unroll
      for (int k = 0; k < 3; ++k) A.depth_rgb8[3 * i + k] = A.lut[3 * (int)d8 + k];
    }
  }
}

// (utils/rend_util.py:linear_to_srgb, optionally behind clamp(0, 1)); a lane reads its element before it writes it: in place is allowed
__global__ __launch_bounds__(IM_THREADS) void im_linear_to_srgb(const float* src, float* dst, int64_t n, int clamp01) {
  const int64_t i = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (i >= n) return;
  float x = src[i];
  if (clamp01) x = fminf(fmaxf(x, 0.0f), 1.0f);
  // 1.055 x^(1/2.4) - 0.055 written as 1.055 (x^(1/2.4) - 1) + 1: the same function, and 1 maps to 1 exactly (include/i2sdf.h)
  dst[i] = x <= 0.0031308f ? x * 12.92f : 1.055f * (powf(x, 1.0f / 2.4f) - 1.0f) + 1.0f;
}

bool bad_sizes(int32_t n_views, int32_t H, int32_t W, int min_side) {
  return n_views < 0 || n_views > 65535 || H < min_side || W < min_side || (int64_t)H * W > INT32_MAX;
}

}  // namespace

extern "C" int64_t i2sdf_image_workspace_bytes(int32_t n_views, int32_t H, int32_t W) {
  Plan P;
  return plan(n_views, H, W, P) ? P.bytes : 0;
}

extern "C" int i2sdf_image_stats(const float* pred, const float* gt, const float* depth, int32_t n_views, int32_t H, int32_t W,
                                 void* workspace, double* stats, void* stream) {
  if (bad_sizes(n_views, H, W, 1)) return I2SDF_EINVAL;
  if (n_views == 0) return I2SDF_OK;
  if (!workspace || !stats || (pred == nullptr) != (gt == nullptr) || (!pred && !depth)) return I2SDF_EINVAL;
  Plan P;
  if (!plan(n_views, H, W, P)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  im_stats<<<dim3((unsigned)P.sb, (unsigned)n_views), IM_THREADS, 0, st>>>(pred, gt, depth, (int64_t)H * W, part);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "im_stats")) return rc;
  im_stats_finish<<<(unsigned)n_views, 64, 0, st>>>(part, P.sb, stats);
  return i2sdf_hip_check(hipGetLastError(), "im_stats_finish");
}

extern "C" int i2sdf_image_ssim(const float* pred, const float* gt, int32_t n_views, int32_t H, int32_t W, float data_range,
                                const double* stats, void* workspace, double* ssim, float* map, void* stream) {
  if (bad_sizes(n_views, H, W, WIN)) return I2SDF_EINVAL;
  const bool from_stats = data_range != data_range;
  if (!from_stats && !(data_range > 0.0f && data_range < INFINITY)) return I2SDF_EINVAL;
  if (n_views == 0) return I2SDF_OK;
  if (!pred || !gt || !workspace || !ssim || (from_stats && !stats)) return I2SDF_EINVAL;
  Plan P;
  if (!plan(n_views, H, W, P) || P.tiles < 1 || P.tiles > INT32_MAX) return I2SDF_EINVAL;
  Taps G;
  double g[WIN], sum = 0.0;
  for (int i = 0; i < WIN; ++i) {
    const double d = (i - WIN / 2) / 1.5;
    g[i] = exp(-d * d / 2.0);
    sum += g[i];
  }
  for (int i = 0; i < WIN; ++i) G.g[i] = (float)(g[i] / sum);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)((char*)workspace + P.off_ssim);
  im_ssim<<<dim3((unsigned)P.tiles, (unsigned)n_views), IM_THREADS, 0, st>>>(pred, gt, H, W, P.tiles_x, G, data_range, stats, part, map);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "im_ssim")) return rc;
  const double count = 3.0 * (double)(H - HALO) * (double)(W - HALO);
  im_ssim_finish<<<(unsigned)n_views, 64, 0, st>>>(part, P.tiles, count, ssim);
  return i2sdf_hip_check(hipGetLastError(), "im_ssim_finish");
}

extern "C" int i2sdf_image_frames(const float* rgb, const float* normal, const float* depth, const float* pose, const double* stats,
                                  const uint8_t* lut, int32_t n_views, int32_t H, int32_t W, uint8_t* rgb8, uint8_t* normal8,
                                  float* normal_cam, uint8_t* depth8, uint8_t* depth_rgb8, void* stream) {
  if (bad_sizes(n_views, H, W, 1)) return I2SDF_EINVAL;
  if (n_views == 0) return I2SDF_OK;
  if (rgb8 && !rgb) return I2SDF_EINVAL;
  if ((normal8 || normal_cam) && (!normal || !pose)) return I2SDF_EINVAL;
  if ((depth8 || depth_rgb8) && (!depth || !stats)) return I2SDF_EINVAL;
  if (depth_rgb8 && !lut) return I2SDF_EINVAL;
  if (!rgb8 && !normal8 && !normal_cam && !depth8 && !depth_rgb8) return I2SDF_OK;
  const int64_t hw = (int64_t)H * W;
  const Frames A{rgb, normal, depth, pose, stats, lut, rgb8, normal8, depth8, depth_rgb8, normal_cam, hw};
  im_frames<<<dim3((unsigned)((hw + IM_THREADS - 1) / IM_THREADS), (unsigned)n_views), IM_THREADS, 0, (hipStream_t)stream>>>(A);
  return i2sdf_hip_check(hipGetLastError(), "im_frames");
}

extern "C" int i2sdf_linear_to_srgb(const float* src, float* dst, int64_t n, int32_t clamp01, void* stream) {
  if (n < 0) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  const int64_t blocks = (n + IM_THREADS - 1) / IM_THREADS;
  if (!src || !dst || blocks > INT32_MAX) return I2SDF_EINVAL;
  im_linear_to_srgb<<<(unsigned)blocks, IM_THREADS, 0, (hipStream_t)stream>>>(src, dst, n, clamp01 ? 1 : 0);
  return i2sdf_hip_check(hipGetLastError(), "im_linear_to_srgb");
}
