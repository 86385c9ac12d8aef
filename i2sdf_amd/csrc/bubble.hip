// Bubble points on the device (the rest of the row): the draw by the PDF and the point cloud it indexes.
//
// i2sdf_bubble_sample -- VolumeRenderSystem.sample_bubble (model/trainer/recon.py:154-170): k of n without replacement, proportional
// to the PDF.  The reference runs torch.where (blocks the host), two gathers and torch.multinomial (exponential fill, divide, top-k over
// every positive entry; refuses more than 2^24 of them).  Here entry i gets the key E_i / pdf[i] with E_i exponential from Philox at
// counter i -- the k smallest keys ARE a successive-sampling draw -- and the k smallest are found by an exact radix select over the
// key bits.  The keys are a pure function of (i, pdf[i]): every pass recomputes them, so pdf is the only n-sized stream, nothing
// n-sized is written, and the histograms are integer sums that do not depend on arrival order.
//   pass A/B/C  per-workgroup LDS histogram of key bits 30..19 / 18..9 / 8..0 among the entries that match the prefix found so
//               far, one global integer atomic per non-empty bin; then a one-wave pick of the bin where the running count crosses k
//               -- and as soon as no more than 2k entries lie at or below the chosen bin's upper end the select is done: the later
//               passes return at once (keys near the small end are evenly spread, so in practice pass A alone decides: 2 passes
//               over the weights, not 4; the count of a call is left in State.passes)
//   collect     every entry with key <= the threshold goes to a buffer of 2k (key bits, index) records; a key whose uniform v
//               already exceeds threshold x weight is dropped before its log1p and divide (E >= v)
//   finish      one workgroup sorts the records in LDS by (key bits, index) and writes idx / points / sample_count / status
// All launches have host-known grids; the number of eligible entries never reaches the host.
//
// i2sdf_depth_unproject_* -- dataset/train_dataset.py:112-141: depth maps -> point cloud + pixel<->point links, a stream compaction in
// image-major pixel order: per-block counts, a single-workgroup exclusive scan, then the writes.
#include <hip/hip_runtime.h>
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
using i2sdf_philox::KEY_MAX;
using i2sdf_philox::key_bits;
using i2sdf_blockops::block_excl_scan;
using i2sdf_blockops::wave_incl_scan;

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;                      // 256 CUs x 8 workgroups of 4 waves
// digits of the select, most significant first (bit 31 of a key >= 0 is 0)
constexpr int SHIFT_A = 19, BITS_A = 12, SHIFT_B = 9, BITS_B = 10, SHIFT_C = 0, BITS_C = 9;
constexpr int NB_A = 1 << BITS_A, NB_B = 1 << BITS_B, NB_C = 1 << BITS_C;
constexpr int SORT_THREADS = 1024, MAX_RECORDS = 2 * I2SDF_BUBBLE_MAX_K;

// workspace: State | hist A | hist B | hist C | records (2k x 8 bytes).  State and the histograms are cleared by every call.
struct State {
  unsigned prefix;      // key bits fixed so far; after pass C the k-th smallest key
  unsigned want;        // rank still to find inside the chosen bin (1-based)
  unsigned done;        // the threshold is final: fewer than k eligible entries, or at most 2k entries at or below it
  unsigned count;       // records appended by the collect pass (may exceed the capacity; the excess is not stored)
  unsigned m;           // eligible entries (pass A's total)
  unsigned T;           // the collect pass takes every key <= T
  unsigned passes;      // passes that read the weights in this call: the histogram passes that ran and the collect pass (2 to 4)
  unsigned pad[9];
};
static_assert(offsetof(State, passes) == I2SDF_BUBBLE_WS_PASSES_OFFSET, "the header documents where the pass count lies");
constexpr int64_t OFF_HIST_A = sizeof(State), OFF_HIST_B = OFF_HIST_A + 4 * NB_A, OFF_HIST_C = OFF_HIST_B + 4 * NB_B,
                  OFF_RECORDS = OFF_HIST_C + 4 * NB_C;
static_assert(sizeof(State) == 64 && OFF_RECORDS % 16 == 0, "workspace layout");

struct Src {
  const float* w;       // NULL: all ones
  int64_t n;
  unsigned seed_lo, seed_hi, draw;
  int vec;              // w is 16-byte aligned: full quads are one load
};

// a bound of FLT_MAX or more goes to key_bits (philox.h) as +inf: an overflowing key is clamped to FLT_MAX and so does NOT exceed it
__device__ __forceinline__ float above_of(unsigned bits) { return bits >= KEY_MAX ? __builtin_inff() : __uint_as_float(bits); }

// keys of entries 4q .. 4q+3 (NOT_ELIGIBLE past n); false when none is eligible (Philox is skipped then)
__device__ __forceinline__ bool quad_keys(const Src& s, int64_t q, float above, unsigned& b0, unsigned& b1, unsigned& b2, unsigned& b3) {
  const int64_t i = 4 * q;
  float w0, w1, w2, w3;
  if (s.w == nullptr) {
    w0 = 1.f; w1 = i + 1 < s.n ? 1.f : 0.f; w2 = i + 2 < s.n ? 1.f : 0.f; w3 = i + 3 < s.n ? 1.f : 0.f;
  } else if (s.vec && i + 3 < s.n) {
    const float4 f = *reinterpret_cast<const float4*>(s.w + i);
    w0 = f.x; w1 = f.y; w2 = f.z; w3 = f.w;
  } else {
    w0 = s.w[i]; w1 = i + 1 < s.n ? s.w[i + 1] : 0.f; w2 = i + 2 < s.n ? s.w[i + 2] : 0.f; w3 = i + 3 < s.n ? s.w[i + 3] : 0.f;
  }
  const bool e0 = w0 > 0.f && w0 < __builtin_inff(), e1 = w1 > 0.f && w1 < __builtin_inff(), e2 = w2 > 0.f && w2 < __builtin_inff(),
             e3 = w3 > 0.f && w3 < __builtin_inff();
  b0 = b1 = b2 = b3 = NOT_ELIGIBLE;
  if (!(e0 || e1 || e2 || e3)) return false;
  const U4 r = philox4x32_10(U4{(unsigned)q, (unsigned)((uint64_t)q >> 32), 7u, s.draw}, s.seed_lo, s.seed_hi);
  b0 = key_bits(r.x, w0, above); b1 = key_bits(r.y, w1, above); b2 = key_bits(r.z, w2, above); b3 = key_bits(r.w, w3, above);
  return true;
}

__global__ __launch_bounds__(THREADS) void bubble_keys_kernel(Src s, float* __restrict__ out) {
  const int64_t nq = (s.n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < nq; q += (int64_t)gridDim.x * THREADS) {
    unsigned b0, b1, b2, b3;
    quad_keys(s, q, __builtin_inff(), b0, b1, b2, b3);
    const int64_t i = 4 * q;
    out[i] = __uint_as_float(b0);
    if (i + 1 < s.n) out[i + 1] = __uint_as_float(b1);
    if (i + 2 < s.n) out[i + 2] = __uint_as_float(b2);
    if (i + 3 < s.n) out[i + 3] = __uint_as_float(b3);
  }
}

// histogram of digit (SHIFT, BITS) among the eligible entries whose higher bits equal the prefix
template <int SHIFT, int BITS>
__global__ __launch_bounds__(THREADS) void bubble_hist_kernel(Src s, const State* __restrict__ st, unsigned* __restrict__ ghist) {
  constexpr int NB = 1 << BITS, HI = SHIFT + BITS;      // HI <= 31
  __shared__ unsigned h[NB];
  if (HI < 31 && st->done) return;                       // (uniform) the threshold is final: nothing left to refine
  const unsigned want_hi = HI < 31 ? st->prefix >> HI : 0u;
  // keys above the upper end of the prefix's range are not counted here (pass A counts every eligible entry: its total is m)
  const float above = HI < 31 ? above_of(st->prefix | ((1u << HI) - 1u)) : __builtin_inff();
  for (int b = threadIdx.x; b < NB; b += THREADS) h[b] = 0u;
  __syncthreads();
  const int64_t nq = (s.n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < nq; q += (int64_t)gridDim.x * THREADS) {
    unsigned b0, b1, b2, b3;
    if (!quad_keys(s, q, above, b0, b1, b2, b3)) continue;
    if (b0 != NOT_ELIGIBLE && (b0 >> HI) == want_hi) atomicAdd(&h[(b0 >> SHIFT) & (NB - 1)], 1u);
    if (b1 != NOT_ELIGIBLE && (b1 >> HI) == want_hi) atomicAdd(&h[(b1 >> SHIFT) & (NB - 1)], 1u);
    if (b2 != NOT_ELIGIBLE && (b2 >> HI) == want_hi) atomicAdd(&h[(b2 >> SHIFT) & (NB - 1)], 1u);
    if (b3 != NOT_ELIGIBLE && (b3 >> HI) == want_hi) atomicAdd(&h[(b3 >> SHIFT) & (NB - 1)], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += THREADS) {
    const unsigned c = h[b];
    if (c) atomicAdd(&ghist[b], c);
  }
}

// one wave: the bin in which the running count crosses the wanted rank
template <int SHIFT, int BITS>
__global__ __launch_bounds__(64) void bubble_pick_kernel(State* __restrict__ st, const unsigned* __restrict__ ghist, unsigned k,
                                                         unsigned cap) {
  constexpr int NB = 1 << BITS, PER = NB / 64;
  constexpr bool TOP = SHIFT + BITS == 31;
  if (!TOP && st->done) return;
  const unsigned want = TOP ? k : st->want;
  const int lane = threadIdx.x;
  if (lane == 0) st->passes += 1u;                       // this digit's histogram pass read the weights
  unsigned sum = 0;
  for (int j = 0; j < PER; ++j) sum += ghist[lane * PER + j];
  const unsigned incl = wave_incl_scan(sum, lane);
  const unsigned total = __shfl(incl, 63);
  if (TOP) {
    if (lane == 0) {
      st->m = total;
      if (total < want) { st->done = 1u; st->T = KEY_MAX; }
    }
    if (total < want) return;                            // fewer than k eligible entries: all of them are taken
  }
  unsigned c = incl - sum;
  if (c < want && want <= incl) {
    for (int j = 0; j < PER; ++j) {
      const unsigned hb = ghist[lane * PER + j];
      if (c + hb >= want) {
        const unsigned prefix = (TOP ? 0u : st->prefix) | ((unsigned)(lane * PER + j) << SHIFT);
        st->prefix = prefix;
        st->want = want - c;
        // k - want entries lie below the prefix's range and c + hb inside it up to this bin: if the buffer holds them all, the bin's
        // upper end is the threshold and the finish kernel's sort finds the k smallest among them
        if (SHIFT == 0 || (k - want) + c + hb <= cap) { st->done = 1u; st->T = prefix | ((1u << SHIFT) - 1u); }
        break;
      }
      c += hb;
    }
  }
}

__global__ __launch_bounds__(THREADS) void bubble_collect_kernel(Src s, State* __restrict__ st, unsigned long long* __restrict__ rec,
                                                                unsigned cap) {
  const unsigned T = st->T;                             // <= KEY_MAX
  if (blockIdx.x == 0 && threadIdx.x == 0) st->passes += 1u;
  const float above = above_of(T);
  const int64_t nq = (s.n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * THREADS + threadIdx.x; q < nq; q += (int64_t)gridDim.x * THREADS) {
    unsigned b[4];
    if (!quad_keys(s, q, above, b[0], b[1], b[2], b[3])) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (b[e] <= T) {                                   // (T <= KEY_MAX < NOT_ELIGIBLE)
        const unsigned pos = atomicAdd(&st->count, 1u);
        if (pos < cap) rec[pos] = ((unsigned long long)b[e] << 32) | (unsigned long long)(unsigned)(4 * q + e);
      }
  }
}

// one workgroup: bitonic sort of the captured records by (key bits, index), then the outputs
__global__ __launch_bounds__(SORT_THREADS) void bubble_finish_kernel(const State* __restrict__ st, const unsigned long long* __restrict__ rec,
                                                                     unsigned cap, unsigned k, const float* __restrict__ pointcloud,
                                                                     int64_t* __restrict__ idx, float* __restrict__ points,
                                                                     float* __restrict__ sample_count, int32_t* __restrict__ status) {
  __shared__ unsigned long long s[MAX_RECORDS];
  const unsigned count = st->count;
  const unsigned c = count < cap ? count : cap;          // cap = 2k <= MAX_RECORDS
  unsigned P = 1;
  while (P < c) P <<= 1;
  for (unsigned i = threadIdx.x; i < P; i += SORT_THREADS) s[i] = i < c ? rec[i] : ~0ull;
  __syncthreads();
  for (unsigned size = 2; size <= P; size <<= 1)
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      for (unsigned t = threadIdx.x; t < (P >> 1); t += SORT_THREADS) {
        const unsigned lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const unsigned long long a = s[lo], b = s[hi];
        const bool up = (lo & size) == 0;
        if ((a > b) == up) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  const unsigned mm = c < k ? c : k;                     // real draws
  for (unsigned j = threadIdx.x; j < k; j += SORT_THREADS) {
    if (mm == 0) {
      idx[j] = -1;
      if (points) { points[3 * j] = 0.f; points[3 * j + 1] = 0.f; points[3 * j + 2] = 0.f; }
      continue;
    }
    const int64_t i = (int64_t)(unsigned)(s[j < mm ? j : j % mm] & 0xffffffffull);
    idx[j] = i;
    if (points) { points[3 * j] = pointcloud[3 * i]; points[3 * j + 1] = pointcloud[3 * i + 1]; points[3 * j + 2] = pointcloud[3 * i + 2]; }
    if (sample_count && j < mm) sample_count[i] += 1.f;
  }
  if (threadIdx.x == 0 && status) {
    int add = (int)(k - mm);
    if (count > cap) add += 1;
    if (add) atomicAdd(status, add);
  }
}

// ---- depth un-projection ----------------------------------------------------------------------
constexpr int UP_THREADS = 256, UP_PER = 4, UP_BLOCK = UP_THREADS * UP_PER;      // pixels per workgroup

__device__ __forceinline__ bool depth_ok(float d, float lo, float hi) { return d > lo && d < hi; }

__global__ __launch_bounds__(UP_THREADS) void unproject_count_kernel(const float* __restrict__ depth, int64_t total, float lo, float hi,
                                                                     int32_t* __restrict__ counts, uint8_t* __restrict__ masks) {
  const int64_t p0 = (int64_t)blockIdx.x * UP_BLOCK + (int64_t)threadIdx.x * UP_PER;
  int c = 0;
#pragma unroll
  for (int e = 0; e < UP_PER; ++e)
    if (p0 + e < total) {
      const bool ok = depth_ok(depth[p0 + e], lo, hi);
      if (masks) masks[p0 + e] = ok ? 1 : 0;
      c += ok ? 1 : 0;
    }
  int tot;
  (void)block_excl_scan<UP_THREADS>(c, tot);
  if (threadIdx.x == 0) counts[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the per-block counts, total at offsets[nb]
__global__ __launch_bounds__(UP_THREADS) void unproject_scan_kernel(const int32_t* __restrict__ counts, int64_t nb, int64_t* __restrict__ offsets) {
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += UP_THREADS) {
    const int64_t b = b0 + threadIdx.x;
    const int v = b < nb ? counts[b] : 0;
    int tot;
    const int ex = block_excl_scan<UP_THREADS>(v, tot);
    if (b < nb) offsets[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) offsets[nb] = carry;
}

__global__ __launch_bounds__(UP_THREADS) void unproject_write_kernel(const float* __restrict__ depth, const float* __restrict__ intrinsics,
                                                                     const float* __restrict__ pose, int64_t total, int32_t HW, int32_t W,
                                                                     float lo, float hi, const int64_t* __restrict__ offsets, int64_t n_points,
                                                                     int64_t* __restrict__ pointlinks, int64_t* __restrict__ pixlinks,
                                                                     float* __restrict__ cloud) {
  const int64_t p0 = (int64_t)blockIdx.x * UP_BLOCK + (int64_t)threadIdx.x * UP_PER;
  float d[UP_PER];
  bool ok[UP_PER];
  int c = 0;
#pragma unroll
  for (int e = 0; e < UP_PER; ++e) {
    d[e] = p0 + e < total ? depth[p0 + e] : 0.f;
    ok[e] = p0 + e < total && depth_ok(d[e], lo, hi);
    c += ok[e] ? 1 : 0;
  }
  int tot;
  int64_t at = offsets[blockIdx.x] + block_excl_scan<UP_THREADS>(c, tot);
#pragma unroll
  for (int e = 0; e < UP_PER; ++e) {
    const int64_t g = p0 + e;
    if (g >= total) continue;
    if (!ok[e]) { if (pointlinks) pointlinks[g] = -1; continue; }
    const int64_t pt = at++;
    if (pointlinks) pointlinks[g] = pt < n_points ? pt : -1;
    if (pt >= n_points) continue;
    if (pixlinks) pixlinks[pt] = g;
    if (cloud) {
      const int64_t img = g / HW;
      const int32_t p = (int32_t)(g - img * HW);
      const float u = (float)(p % W), v = (float)(p / W);
      const float* K = intrinsics + 16 * img;
      const float* M = pose + 16 * img;
      const float fx = K[0], sk = K[1], cx = K[2], fy = K[5], cy = K[6];
      const float xl = (u - cx + cy * sk / fy - sk * v / fy) / fx * d[e], yl = (v - cy) / fy * d[e], zl = d[e];
      const float X = M[0] * xl + M[1] * yl + M[2] * zl + M[3], Y = M[4] * xl + M[5] * yl + M[6] * zl + M[7],
                  Z = M[8] * xl + M[9] * yl + M[10] * zl + M[11], Wh = M[12] * xl + M[13] * yl + M[14] * zl + M[15];
      cloud[3 * pt] = X / Wh; cloud[3 * pt + 1] = Y / Wh; cloud[3 * pt + 2] = Z / Wh;
    }
  }
}

bool unproject_sizes(int64_t n_img, int32_t H, int32_t W, int64_t& total, int64_t& nb) {
  if (n_img < 0 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX) return false;
  if (n_img > (((int64_t)1 << 36) - 1) / ((int64_t)H * W)) return false;
  total = n_img * H * W;
  nb = (total + UP_BLOCK - 1) / UP_BLOCK;
  return true;
}

unsigned stream_blocks(int64_t n) { return i2sdf_blockops::blocks((n + 3) / 4, THREADS, MAX_BLOCKS); }      // a thread per quad

Src make_src(const float* w, int64_t n, uint64_t seed, uint32_t draw) {
  return Src{w, n, (unsigned)seed, (unsigned)(seed >> 32), draw, ((uintptr_t)w & 15) == 0 ? 1 : 0};
}

}  // namespace

extern "C" int64_t i2sdf_bubble_sample_workspace_bytes(int64_t k) {
  if (k < 1 || k > I2SDF_BUBBLE_MAX_K) return 0;
  return OFF_RECORDS + 2 * k * 8;
}

extern "C" int i2sdf_bubble_keys(const float* weights, int64_t n, uint64_t seed, uint32_t draw, float* keys_out, void* stream) {
  if (n < 0 || n > INT32_MAX) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  if (keys_out == nullptr) return I2SDF_EINVAL;
  bubble_keys_kernel<<<stream_blocks(n), THREADS, 0, (hipStream_t)stream>>>(make_src(weights, n, seed, draw), keys_out);
  return i2sdf_hip_check(hipGetLastError(), "bubble_keys");
}

extern "C" int i2sdf_bubble_sample(const float* weights, int64_t n, const float* pointcloud, int64_t k, uint64_t seed, uint32_t draw,
                                   void* workspace, int64_t* idx, float* points, float* sample_count, int32_t* status, void* stream) {
  if (k < 1 || k > I2SDF_BUBBLE_MAX_K || n < 0 || n > INT32_MAX) return I2SDF_EINVAL;
  if (idx == nullptr || workspace == nullptr || ((uintptr_t)workspace & 15) != 0) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  State* state = (State*)ws;
  unsigned* hA = (unsigned*)(ws + OFF_HIST_A);
  unsigned* hB = (unsigned*)(ws + OFF_HIST_B);
  unsigned* hC = (unsigned*)(ws + OFF_HIST_C);
  unsigned long long* rec = (unsigned long long*)(ws + OFF_RECORDS);
  const Src s = make_src(weights, n, seed, draw);
  const unsigned nb = stream_blocks(n), kk = (unsigned)k, cap = 2u * kk;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(ws, 0, (size_t)OFF_RECORDS, st), "bubble_sample clear")) return rc;
  bubble_hist_kernel<SHIFT_A, BITS_A><<<nb, THREADS, 0, st>>>(s, state, hA);
  bubble_pick_kernel<SHIFT_A, BITS_A><<<1, 64, 0, st>>>(state, hA, kk, cap);
  bubble_hist_kernel<SHIFT_B, BITS_B><<<nb, THREADS, 0, st>>>(s, state, hB);
  bubble_pick_kernel<SHIFT_B, BITS_B><<<1, 64, 0, st>>>(state, hB, kk, cap);
  bubble_hist_kernel<SHIFT_C, BITS_C><<<nb, THREADS, 0, st>>>(s, state, hC);
  bubble_pick_kernel<SHIFT_C, BITS_C><<<1, 64, 0, st>>>(state, hC, kk, cap);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "bubble_sample select")) return rc;
  bubble_collect_kernel<<<nb, THREADS, 0, st>>>(s, state, rec, cap);
  bubble_finish_kernel<<<1, SORT_THREADS, 0, st>>>(state, rec, cap, kk, pointcloud, idx, pointcloud ? points : nullptr, sample_count, status);
  return i2sdf_hip_check(hipGetLastError(), "bubble_sample finish");
}

extern "C" int64_t i2sdf_depth_unproject_workspace_bytes(int64_t n_img, int32_t H, int32_t W) {
  int64_t total, nb;
  if (!unproject_sizes(n_img, H, W, total, nb)) return 0;
  return 8 * (nb + 1) + 4 * nb + 16;        // offsets (nb + 1) int64 | counts (nb) int32
}

extern "C" int i2sdf_depth_unproject_count(const float* depth, int64_t n_img, int32_t H, int32_t W, float lo, float hi, void* workspace,
                                           uint8_t* depth_masks, int64_t* n_points, void* stream) {
  int64_t total, nb;
  if (!unproject_sizes(n_img, H, W, total, nb) || n_points == nullptr) return I2SDF_EINVAL;
  *n_points = 0;
  if (total == 0) return I2SDF_OK;
  if (depth == nullptr || workspace == nullptr || ((uintptr_t)workspace & 7) != 0) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int64_t* offsets = (int64_t*)workspace;
  int32_t* counts = (int32_t*)(offsets + nb + 1);
  unproject_count_kernel<<<(unsigned)nb, UP_THREADS, 0, st>>>(depth, total, lo, hi, counts, depth_masks);
  unproject_scan_kernel<<<1, UP_THREADS, 0, st>>>(counts, nb, offsets);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "depth_unproject count")) return rc;
  if (int rc = i2sdf_hip_check(hipMemcpyAsync(n_points, offsets + nb, 8, hipMemcpyDeviceToHost, st), "depth_unproject n_points")) return rc;
  return i2sdf_hip_check(hipStreamSynchronize(st), "depth_unproject n_points");
}

extern "C" int i2sdf_depth_unproject_write(const float* depth, const float* intrinsics, const float* pose, int64_t n_img, int32_t H,
                                           int32_t W, float lo, float hi, const void* workspace, int64_t n_points, int64_t* pointlinks,
                                           int64_t* pixlinks, float* pointcloud, void* stream) {
  int64_t total, nb;
  if (!unproject_sizes(n_img, H, W, total, nb) || n_points < 0 || n_points > total) return I2SDF_EINVAL;
  if (total == 0) return I2SDF_OK;
  if (depth == nullptr || workspace == nullptr || ((uintptr_t)workspace & 7) != 0) return I2SDF_EINVAL;
  if (pointcloud != nullptr && (intrinsics == nullptr || pose == nullptr)) return I2SDF_EINVAL;
  if (pixlinks == nullptr && pointcloud == nullptr && pointlinks == nullptr) return I2SDF_OK;
  unproject_write_kernel<<<(unsigned)nb, UP_THREADS, 0, (hipStream_t)stream>>>(depth, intrinsics, pose, total, H * W, W, lo, hi,
                                                                              (const int64_t*)workspace, n_points, pointlinks, pixlinks,
                                                                              pointcloud);
  return i2sdf_hip_check(hipGetLastError(), "depth_unproject write");
}
