// Workgroup primitives of the geometry translation units (mcubes, tsdf, meshops, bubble, pointops, imgops, kmeans): wave and
// workgroup scans and reductions in a fixed order, the multi-level reduce-then-scan built on them, and the small host helpers their
// callers size launches and workspaces with.  Additions, comparisons and shuffles only -- no product feeds a sum here, so a
// translation unit's `fp contract` setting does not reach into this file.  The training kernels (render, sampler, loss, pack,
// mlp_*, wgrad) have their own DPP scans and pinned summation orders and do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "../../include/i2sdf.h"

int i2sdf_hip_check(hipError_t e, const char* what);

namespace i2sdf_blockops {

// ---- host: launch and workspace sizes ---------------------------------------------------------------
inline bool fits(int64_t n) { return n >= 0 && n <= INT32_MAX; }
inline int64_t align16(int64_t x) { return (x + 15) / 16 * 16; }
inline unsigned blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }
inline unsigned blocks(int64_t n, int threads, int max_blocks) {      // grid-stride kernels: at least one workgroup, at most max_blocks
  const int64_t b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// ---- wave (64 lanes) --------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T shfl_up(T x, int d) { return __shfl_up(x, d, 64); }
__device__ __forceinline__ longlong2 shfl_up(longlong2 v, int d) { return make_longlong2(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)); }

// inclusive prefix in lane order
template <class T>
__device__ __forceinline__ T wave_incl_scan(T x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// xor butterfly: every lane ends with op over the wave's 64 values, combined in the same tree in every run
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <class T>
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <class T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }
__device__ __forceinline__ float wave_min(float v) { return wave_reduce(v, [](float a, float b) { return fminf(a, b); }); }   // (a NaN is passed over)
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }

// ---- workgroup --------------------------------------------------------------------------------------
// Contract of the two functions below: EVERY thread of the workgroup calls them (they hold barriers); THREADS is the workgroup size, a
// multiple of 64; each instantiation owns THREADS / 64 values of LDS.  Both end in a barrier, so calls may follow one another, or sit
// in a loop, without help from the caller.

// Exclusive prefix of x in thread order; `total` = the workgroup's sum, in every thread.  T: int, int64_t, double, longlong2 (a pair
// of int64 added per component).  The exclusive value is the wave base + the left neighbour's inclusive value (lane 0: the base) --
// for integers the same number as base + inclusive - x, for floating point the only form whose value is a sum of the items before.
template <int THREADS, class T>
__device__ T block_excl_scan(T x, T& total) {
  static_assert(THREADS % 64 == 0, "whole waves");
  __shared__ T ws[THREADS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T inc = wave_incl_scan(x, lane);
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  T base{}, tot{};
#pragma unroll
  for (int u = 0; u < THREADS / 64; ++u) {
    if (u < w) base += ws[u];
    tot += ws[u];
  }
  __syncthreads();                                 // ws is reused by the next call
  total = tot;
  const T left = shfl_up(inc, 1);
  return lane ? base + left : base;
}

// Sum of x over the workgroup, in every thread: xor butterfly within a wave, then the wave sums added in wave order.
template <int THREADS, class T>
__device__ T block_sum(T x) {
  static_assert(THREADS % 64 == 0, "whole waves");
  __shared__ T ws[THREADS / 64];
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = x;
  __syncthreads();
  T t{};
#pragma unroll
  for (int u = 0; u < THREADS / 64; ++u) t += ws[u];
  __syncthreads();
  return t;
}

// ---- multi-level scan -------------------------------------------------------------------------------
// Reduce-then-scan over workgroups in separate launches: SCAN_CHUNK items per workgroup per level, level l + 1 holds one sum per
// chunk of level l, the top level is the first one that a single workgroup scans.  Fixed order, no atomics, no flags between
// workgroups.
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;
constexpr int SCAN_MAX_LEVELS = 8;

struct ScanLevels {
  int n_levels;
  int64_t level_off[SCAN_MAX_LEVELS], level_n[SCAN_MAX_LEVELS];      // byte offset into the workspace, values
  int64_t bytes;                                                     // end of the last level
};

// levels of elem_bytes-sized values from byte first_offset on, level 0 with n_level0 values; false: more than SCAN_MAX_LEVELS levels
inline bool scan_levels(int64_t n_level0, int64_t elem_bytes, int64_t first_offset, ScanLevels& L) {
  L.n_levels = 0;
  int64_t o = first_offset;
  for (int64_t m = n_level0;; m = (m + SCAN_CHUNK - 1) / SCAN_CHUNK) {
    if (L.n_levels == SCAN_MAX_LEVELS) return false;
    L.level_off[L.n_levels] = o;
    L.level_n[L.n_levels] = m;
    ++L.n_levels;
    o += elem_bytes * m;
    if (m <= SCAN_CHUNK) break;
  }
  L.bytes = o;
  return true;
}

template <class T>
struct ScanSrc {                                   // the items of a level as they lie in the workspace
  const T* x;
  __device__ T operator()(int64_t i) const { return x[i]; }
};

// sums[b] = src(b SCAN_CHUNK) + ... + src((b + 1) SCAN_CHUNK - 1), items past n left out
template <class Src, class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(Src src, int64_t n, T* __restrict__ sums) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
  T x{};
#pragma unroll
  for (int u = 0; u < SCAN_ITEMS; ++u)
    if (base + u < n) x += src(base + u);
  T tot;
  (void)block_excl_scan<SCAN_THREADS>(x, tot);     // (its total, not block_sum: the order the scan below adds in)
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// out[chunk b] <- prefix within the chunk + add[b] (add NULL: 0); INCLUSIVE: item i included (the running sum), else excluded.
// out may be the array src reads (each thread reads its items before it writes them).  total (NULL, or one workgroup only): the sum.
template <class Src, class T, bool INCLUSIVE>
__global__ __launch_bounds__(SCAN_THREADS) void scan_chunks_kernel(Src src, int64_t n, const T* __restrict__ add, T* out,
                                                                    T* __restrict__ total) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
  T it[SCAN_ITEMS];
  T x{};
#pragma unroll
  for (int u = 0; u < SCAN_ITEMS; ++u) {
    it[u] = base + u < n ? src(base + u) : T{};
    x += it[u];
  }
  T tot;
  T o = block_excl_scan<SCAN_THREADS>(x, tot);
  if (add) o += add[blockIdx.x];
#pragma unroll
  for (int u = 0; u < SCAN_ITEMS; ++u) {
    if (INCLUSIVE) o += it[u];
    if (base + u < n) out[base + u] = o;
    if (!INCLUSIVE) o += it[u];
  }
  if (total && threadIdx.x == 0) *total = tot;
}

// Level 0 of L (already in the workspace) becomes its exclusive prefix in place, and so does every level above it: sums up the
// levels, the top level scanned by one workgroup, then every lower level with its chunk offsets.  total (device, or NULL): the sum of
// level 0.
template <class T>
int scan_levels_exclusive(void* workspace, const ScanLevels& L, T* total, hipStream_t st) {
  T* lv[SCAN_MAX_LEVELS];
  for (int l = 0; l < L.n_levels; ++l) lv[l] = (T*)((char*)workspace + L.level_off[l]);
  const int top = L.n_levels - 1;
  for (int l = 0; l < top; ++l) {
    scan_reduce_kernel<ScanSrc<T>, T><<<(unsigned)L.level_n[l + 1], SCAN_THREADS, 0, st>>>(ScanSrc<T>{lv[l]}, L.level_n[l], lv[l + 1]);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "scan_reduce_kernel")) return rc;
  }
  for (int l = top; l >= 0; --l) {
    scan_chunks_kernel<ScanSrc<T>, T, false><<<l == top ? 1u : (unsigned)L.level_n[l + 1], SCAN_THREADS, 0, st>>>(
        ScanSrc<T>{lv[l]}, L.level_n[l], l == top ? nullptr : lv[l + 1], lv[l], l == top ? total : nullptr);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "scan_chunks_kernel")) return rc;
  }
  return I2SDF_OK;
}

}  // namespace i2sdf_blockops
