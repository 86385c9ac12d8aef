// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's known answers: counter 0 / key 0 ->
// 6627e8d5 e169c58d bc57ac4c 9b00dbd8, all-ones -> 408f276d 41c83b0e a20bc7c6 6d5451fd).  Shared by the training draws (draws.hip)
// and the bubble sampler (bubble.hip): one call gives four 32-bit words for one 128-bit counter.
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

}  // namespace i2sdf_philox
