// Emitter clustering on the device: I2SDFNetwork.init_emission_groups (model/network/__init__.py:49-75) without its two host-bound
// helpers.  include/i2sdf.h ("Emitter clustering") states both laws; this file is their only implementation.
//
// i2sdf_kmeans_pp -- utils.kmeans_pp_centroid (utils/__init__.py:111-123): the next centroid is a data point drawn with probability
// proportional to its distance to the nearest centroid so far.  The reference builds an (n, i, 3) tensor per round and blocks the host
// on an argmax; here a round is ONE pass over the points (12 B of point and 4 B of d read, 4 B written): d_j = min(d_j, |p_j - c|), the
// exponential-race key E_j / d_j (philox.h, as bubble.hip) on Philox stream word 9, and the minimum of (key bits << 32 | j) -- a wave butterfly, four
// values in LDS, one 64-bit integer atomicMin per workgroup into the round's own slot.  The next round's launch reads that slot: the
// winner never reaches the host.
//
// i2sdf_kmeans_fit -- fast_pytorch_kmeans.KMeans.fit_predict with its defaults: per iteration one pass that labels every point (nearest
// centroid, lowest index on ties) and adds its coordinates to its cluster in 64-bit FIXED POINT (scale from the cloud's largest |coordinate|;
// integer adds commute, so neither the LDS nor the global atomics make the sums depend on arrival order), then one workgroup that turns
// the sums into means, measures the shift, counts the iteration and raises the stop flag.  Once the flag is up the remaining launches
// return at once.  No floating-point atomic, no grid-wide barrier, every grid known to the host.
//
// i2sdf_kmeans_assign -- the labelling pass alone (KMeans.predict), optionally with the squared distance to the chosen centroid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "philox.h"
#include "blockops.h"

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using i2sdf_philox::U4;
using i2sdf_philox::philox4x32_10;
using i2sdf_philox::NOT_ELIGIBLE;
using i2sdf_philox::key_bits;
using i2sdf_blockops::blocks;
using i2sdf_blockops::wave_max;
using i2sdf_blockops::wave_min;

constexpr unsigned long long NO_WINNER = ~0ull;     // a slot no workgroup has written: nothing was eligible -> index 0
constexpr unsigned STREAM_WORD = 9u;                // (philox.h lists the others)
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_BLOCKS_PP = 2048;                 // 256 CUs x 8 workgroups of 4 waves
constexpr int MAX_BLOCKS_FIT = 1024;                // every workgroup ends in up to 4k global atomics: fewer, longer workgroups
constexpr int MAX_K = I2SDF_KMEANS_MAX_K;

// workspace: Head | acc (k x 4 int64: sum x, sum y, sum z, count) | slots (k x uint64) | d (n x fp32)
struct Head {
  unsigned maxabs_bits;     // bits of the largest finite |coordinate| (integer atomicMax: the bits of floats >= 0 order like the floats)
  unsigned stop;            // error <= tol was seen: every later launch of this call returns at once
  unsigned pad[14];
};
static_assert(sizeof(Head) == 64, "workspace layout");
constexpr int64_t OFF_ACC = sizeof(Head);
inline int64_t off_slots(int64_t k) { return OFF_ACC + 32 * k; }
inline int64_t off_d(int64_t k) { return (off_slots(k) + 8 * k + 15) / 16 * 16; }

// (x-cx)^2 + (y-cy)^2 + (z-cz)^2, every operation rounded to fp32, summed left to right, nothing contracted into an FMA
__device__ __forceinline__ float dist2(float x, float y, float z, float cx, float cy, float cz) {
  const float dx = __fsub_rn(x, cx), dy = __fsub_rn(y, cy), dz = __fsub_rn(z, cz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ unsigned slot_index(unsigned long long s) { return s == NO_WINNER ? 0u : (unsigned)(s & 0xffffffffull); }

// ---- seeding ------------------------------------------------------------------------------------
__global__ void kmeans_pp_first_kernel(unsigned long long* __restrict__ slots, unsigned n, unsigned seed_lo, unsigned seed_hi) {
  const U4 r = philox4x32_10(U4{0u, 0u, STREAM_WORD, 0u}, seed_lo, seed_hi);
  slots[0] = ((unsigned long long)r.x * n) >> 32;
}

// round i >= 1: the centroid is the point round i - 1 chose.  Thread = four neighbouring points = one Philox call.
__global__ __launch_bounds__(THREADS) void kmeans_pp_round_kernel(const float* __restrict__ points, int64_t n, float* __restrict__ d,
                                                                  unsigned long long* __restrict__ slots, unsigned round,
                                                                  unsigned seed_lo, unsigned seed_hi, int vec) {
  __shared__ unsigned long long wmin[WAVES];
  const int64_t jc = slot_index(slots[round - 1]);
  const float cx = points[3 * jc], cy = points[3 * jc + 1], cz = points[3 * jc + 2];
  unsigned long long best = NO_WINNER;
  const int64_t nq = (n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < nq; q += (int64_t)gridDim.x * THREADS) {
    const int64_t j = 4 * q;
    const bool full = j + 3 < n;
    float p[12], dj[4];
    if (vec && full) {
      const float4* src = reinterpret_cast<const float4*>(points + 3 * j);
      const float4 a = src[0], b = src[1], c = src[2];
      p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w; p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
      p[8] = c.x; p[9] = c.y; p[10] = c.z; p[11] = c.w;
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e) p[e] = 3 * j + e < 3 * n ? points[3 * j + e] : 0.f;
    }
    if (round == 1) {
      dj[0] = dj[1] = dj[2] = dj[3] = __builtin_inff();      // d starts at +inf: the workspace is not read before it is written
    } else if (vec && full) {
      const float4 o = *reinterpret_cast<const float4*>(d + j);
      dj[0] = o.x; dj[1] = o.y; dj[2] = o.z; dj[3] = o.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) dj[e] = j + e < n ? d[j + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) dj[e] = fminf(dj[e], __fsqrt_rn(dist2(p[3 * e], p[3 * e + 1], p[3 * e + 2], cx, cy, cz)));
    if (vec && full) {
      *reinterpret_cast<float4*>(d + j) = make_float4(dj[0], dj[1], dj[2], dj[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e < n) d[j + e] = dj[e];
    }
    const U4 r = philox4x32_10(U4{(unsigned)q, (unsigned)((uint64_t)q >> 32), STREAM_WORD, round}, seed_lo, seed_hi);
    const unsigned x[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j + e >= n) continue;
      const unsigned kb = key_bits(x[e], dj[e], __builtin_inff());      // every key matters: nothing dropped
      if (kb == NOT_ELIGIBLE) continue;
      const unsigned long long comp = ((unsigned long long)kb << 32) | (unsigned long long)(unsigned)(j + e);
      best = comp < best ? comp : best;
    }
  }
  best = wave_min(best);
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w) best = wmin[w] < best ? wmin[w] : best;
    if (best != NO_WINNER) atomicMin(&slots[round], best);
  }
}

__global__ __launch_bounds__(THREADS) void kmeans_pp_emit_kernel(const float* __restrict__ points, const unsigned long long* __restrict__ slots,
                                                                 int k, int64_t* __restrict__ idx_out, float* __restrict__ centroids_out) {
  for (int i = threadIdx.x; i < k; i += THREADS) {
    const int64_t j = slot_index(slots[i]);
    idx_out[i] = j;
    centroids_out[3 * i] = points[3 * j]; centroids_out[3 * i + 1] = points[3 * j + 1]; centroids_out[3 * i + 2] = points[3 * j + 2];
  }
}

// ---- Lloyd ----------------------------------------------------------------------------------------
// largest finite |coordinate| of the cloud: per-thread maximum of the bits, wave butterfly, one integer atomicMax per wave
__global__ __launch_bounds__(THREADS) void kmeans_range_kernel(const float* __restrict__ points, int64_t n3, Head* __restrict__ head) {
  unsigned m = 0u;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n3; i += (int64_t)gridDim.x * THREADS) {
    const unsigned b = __float_as_uint(points[i]) & 0x7fffffffu;
    if (b < 0x7f800000u && b > m) m = b;
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(&head->maxabs_bits, m);
}

// the fixed-point scale 2^s: with 2^(e-1) <= maxabs < 2^e, s = 31 - e, so |x| 2^s <= 2^31 and a sum of fewer than 2^31 of them stays
// below 2^62.  (maxabs = 0 or a denormal: e = -126; any s does for a cloud of zeros.)
__device__ __forceinline__ int scale_exponent(unsigned maxabs_bits) { return 31 - ((int)(maxabs_bits >> 23) - 126); }
__device__ __forceinline__ double pow2(int s) { return __longlong_as_double((long long)(1023 + s) << 52); }      // -1022 <= s <= 1023

__device__ __forceinline__ long long to_fixed(float x, double scale, float maxabs) {
  return fabsf(x) <= maxabs ? __double2ll_rn((double)x * scale) : 0ll;      // a non-finite coordinate adds nothing
}

// labels (and dist2) of every point; ACCUM: also the per-cluster fixed-point sums and counts into acc
template <bool ACCUM>
__global__ __launch_bounds__(THREADS) void kmeans_assign_kernel(const float* __restrict__ points, int64_t n, const float* __restrict__ centroids,
                                                                int k, int64_t* __restrict__ labels, float* __restrict__ dist2_out,
                                                                const Head* __restrict__ head, unsigned long long* __restrict__ acc) {
  __shared__ float4 cs[MAX_K];
  __shared__ unsigned long long sums[ACCUM ? WAVES * MAX_K * 4 : 1];      // one copy per wave: a quarter of the contention
  if (ACCUM && head->stop) return;                                         // (uniform)
  for (int c = threadIdx.x; c < k; c += THREADS) cs[c] = make_float4(centroids[3 * c], centroids[3 * c + 1], centroids[3 * c + 2], 0.f);
  if (ACCUM)
    for (int c = threadIdx.x; c < WAVES * k * 4; c += THREADS) sums[c] = 0ull;
  __syncthreads();
  double scale = 0.0;
  float maxabs = 0.f;
  if (ACCUM) {
    const unsigned mb = head->maxabs_bits;
    scale = pow2(scale_exponent(mb));
    maxabs = __uint_as_float(mb);
  }
  unsigned long long* mine = sums + (ACCUM ? (threadIdx.x >> 6) * k * 4 : 0);
  for (int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * THREADS) {
    const float x = points[3 * j], y = points[3 * j + 1], z = points[3 * j + 2];
    float best = __builtin_inff();
    int lab = 0;
    for (int c = 0; c < k; ++c) {
      const float4 cc = cs[c];
      const float dd = dist2(x, y, z, cc.x, cc.y, cc.z);
      if (dd < best) { best = dd; lab = c; }                               // strict: ties (and NaN) keep the lower index
    }
    labels[j] = lab;
    if (dist2_out) dist2_out[j] = dist2(x, y, z, cs[lab].x, cs[lab].y, cs[lab].z);
    if (ACCUM) {
      atomicAdd(&mine[4 * lab], (unsigned long long)to_fixed(x, scale, maxabs));
      atomicAdd(&mine[4 * lab + 1], (unsigned long long)to_fixed(y, scale, maxabs));
      atomicAdd(&mine[4 * lab + 2], (unsigned long long)to_fixed(z, scale, maxabs));
      atomicAdd(&mine[4 * lab + 3], 1ull);
    }
  }
  if (ACCUM) {
    __syncthreads();
    for (int c = threadIdx.x; c < 4 * k; c += THREADS) {
      unsigned long long s = 0ull;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += sums[w * k * 4 + c];
      if (s) atomicAdd(&acc[c], s);
    }
  }
}

// one workgroup: means, shift, iteration count, stop flag; leaves acc cleared for the next iteration
__global__ __launch_bounds__(THREADS) void kmeans_update_kernel(Head* __restrict__ head, unsigned long long* __restrict__ acc,
                                                                float* __restrict__ centroids, int k, double tol, int32_t* __restrict__ n_iter) {
  __shared__ double err[THREADS];
  if (head->stop) return;
  const double inv = pow2(-scale_exponent(head->maxabs_bits));
  double e = 0.0;
  for (int c = threadIdx.x; c < k; c += THREADS) {                         // k <= 256: one cluster per thread
    const long long cnt = (long long)acc[4 * c + 3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float fresh = cnt > 0 ? (float)((double)(long long)acc[4 * c + a] * inv / (double)cnt) : 0.f;      // empty cluster: (0, 0, 0)
      const double diff = (double)fresh - (double)centroids[3 * c + a];
      e += diff * diff;
      centroids[3 * c + a] = fresh;
    }
    acc[4 * c] = acc[4 * c + 1] = acc[4 * c + 2] = acc[4 * c + 3] = 0ull;
  }
  err[threadIdx.x] = e;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {                              // fixed tree: the same sum in every run
    if (threadIdx.x < s) err[threadIdx.x] += err[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *n_iter += 1;
    if (err[0] <= tol) head->stop = 1u;
  }
}

__global__ void kmeans_fit_begin_kernel(int32_t* __restrict__ n_iter) { *n_iter = 0; }

bool sizes_ok(int64_t n, int64_t k) { return k >= 1 && k <= MAX_K && n >= 1 && n <= INT32_MAX; }

}  // namespace

extern "C" int64_t i2sdf_kmeans_workspace_bytes(int64_t n, int64_t k) {
  if (!sizes_ok(n, k) || k > n) return 0;
  return (off_d(k) + 4 * n + 15) / 16 * 16;
}

extern "C" int i2sdf_kmeans_pp(const float* points, int64_t n, int64_t k, uint64_t seed, void* workspace, int64_t* idx_out,
                               float* centroids_out, void* stream) {
  if (!sizes_ok(n, k) || k > n) return I2SDF_EINVAL;
  if (points == nullptr || idx_out == nullptr || centroids_out == nullptr) return I2SDF_EINVAL;
  if (workspace == nullptr || ((uintptr_t)workspace & 15) != 0) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* slots = (unsigned long long*)(ws + off_slots(k));
  float* d = (float*)(ws + off_d(k));
  const unsigned lo = (unsigned)seed, hi = (unsigned)(seed >> 32);
  const int vec = ((uintptr_t)points & 15) == 0 ? 1 : 0;                   // (d is 16-byte aligned by the layout)
  if (int rc = i2sdf_hip_check(hipMemsetAsync(slots, 0xff, (size_t)(8 * k), st), "kmeans_pp clear")) return rc;
  kmeans_pp_first_kernel<<<1, 1, 0, st>>>(slots, (unsigned)n, lo, hi);
  const unsigned nb = blocks((n + 3) / 4, THREADS, MAX_BLOCKS_PP);
  for (int64_t i = 1; i < k; ++i) kmeans_pp_round_kernel<<<nb, THREADS, 0, st>>>(points, n, d, slots, (unsigned)i, lo, hi, vec);
  kmeans_pp_emit_kernel<<<1, THREADS, 0, st>>>(points, slots, (int)k, idx_out, centroids_out);
  return i2sdf_hip_check(hipGetLastError(), "kmeans_pp");
}

extern "C" int i2sdf_kmeans_fit(const float* points, int64_t n, int64_t k, float* centroids, int32_t max_iter, double tol, void* workspace,
                                int64_t* labels, int32_t* n_iter, void* stream) {
  if (!sizes_ok(n, k) || k > n || max_iter < 1 || !(tol >= 0.0)) return I2SDF_EINVAL;
  if (points == nullptr || centroids == nullptr || labels == nullptr || n_iter == nullptr) return I2SDF_EINVAL;
  if (workspace == nullptr || ((uintptr_t)workspace & 15) != 0) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Head* head = (Head*)ws;
  unsigned long long* acc = (unsigned long long*)(ws + OFF_ACC);
  if (int rc = i2sdf_hip_check(hipMemsetAsync(ws, 0, (size_t)off_slots(k), st), "kmeans_fit clear")) return rc;
  kmeans_fit_begin_kernel<<<1, 1, 0, st>>>(n_iter);
  kmeans_range_kernel<<<blocks(3 * n, THREADS, MAX_BLOCKS_FIT), THREADS, 0, st>>>(points, 3 * n, head);
  const unsigned nb = blocks(n, THREADS, MAX_BLOCKS_FIT);
  for (int32_t it = 0; it < max_iter; ++it) {
    kmeans_assign_kernel<true><<<nb, THREADS, 0, st>>>(points, n, centroids, (int)k, labels, nullptr, head, acc);
    kmeans_update_kernel<<<1, THREADS, 0, st>>>(head, acc, centroids, (int)k, tol, n_iter);
  }
  return i2sdf_hip_check(hipGetLastError(), "kmeans_fit");
}

extern "C" int i2sdf_kmeans_assign(const float* points, int64_t n, const float* centroids, int64_t k, int64_t* labels, float* dist2,
                                   void* stream) {
  if (k < 1 || k > MAX_K || n < 0 || n > INT32_MAX) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  if (points == nullptr || centroids == nullptr || labels == nullptr) return I2SDF_EINVAL;
  kmeans_assign_kernel<false><<<blocks(n, THREADS, MAX_BLOCKS_PP), THREADS, 0, (hipStream_t)stream>>>(points, n, centroids, (int)k, labels, dist2,
                                                                                               nullptr, nullptr);
  return i2sdf_hip_check(hipGetLastError(), "kmeans_assign");
}
