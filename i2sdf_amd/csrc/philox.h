// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's known answers: counter 0 / key 0 ->
// 6627e8d5 e169c58d bc57ac4c 9b00dbd8, all-ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd): one call gives four 32-bit words for one 128-bit counter.
// With it, what the callers make of a word: a uniform (draws.hip, shade.hip) and an exponential-race key (bubble.hip, kmeans.hip).
// Stream words (counter word z): 1..6 draws.hip, 7 bubble.hip, 8 shade.hip, 9 kmeans.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace i2sdf_philox {

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
    c = U4{(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c;
}

// [0, 1) with 24 bits, like torch.rand
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }

// Exponential-race key of an entry of weight w: the bits of E / w, E = -log1pf(-v), v = (x + 0.5) 2^-32, clamped to FLT_MAX = KEY_MAX;
// the k smallest keys are a draw of k entries without replacement, proportional to w.  w not in (0, inf): NOT_ELIGIBLE.
// `above`: keys greater than this do not matter to the caller and may come back as NOT_ELIGIBLE.  E >= v, so a key is at least v / w:
// with v > 1.001 above w it exceeds `above` whatever the rounding of log1pf (2 ulp) and of the divide -- and then neither is computed.
// With above = +inf that early-out is never taken for an eligible w (above w = +inf), so nothing is dropped and the bits are those of
// the plain E / w: what a caller that needs every key passes (kmeans.hip; bubble.hip's first pass).  The test names +inf itself, so
// that it folds away where the caller passes the constant.
constexpr unsigned NOT_ELIGIBLE = 0x7f800000u;      // bits(+inf)
constexpr unsigned KEY_MAX = 0x7f7fffffu;
__device__ __forceinline__ unsigned key_bits(unsigned x, float w, float above) {
  if (!(w > 0.f && w < __builtin_inff())) return NOT_ELIGIBLE;
  const float v = ((float)x + 0.5f) * 2.3283064365386963e-10f;      // 2^-32
  if (above < __builtin_inff() && v > 1.001f * (above * w)) return NOT_ELIGIBLE;
  const float key = fminf(-log1pf(-v) / w, 3.4028234663852886e38f);
  return __float_as_uint(key);
}

}  // namespace i2sdf_philox
