// Lock-free union-find on int32 indices, the scheme of meshops.hip's face components: a root is hooked under a SMALLER root by an
// integer compare-and-swap, so every tree's root is its smallest member and the final roots do not depend on the order of the unions.
// A retry follows only a compare-and-swap that lost to another thread's progress; nobody waits for anybody.
//
// Invariant the loop bounds rest on: parent[x] <= x for every x, at any time (initially parent[x] = x; a hook stores a smaller index;
// path halving stores an ancestor, which is smaller still).  So a walk from x to its root takes at most x steps, and every retry of
// unite() starts from a strictly smaller pair maximum, at most max(a, b) times.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace i2sdf_unionfind {

#define I2SDF_UF_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// root of x, halving the path on the way (a non-root never becomes a root again and only ever points to an ancestor, so a
// racing store of a grandparent is harmless)
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
  int32_t p = __hip_atomic_load(parent + x, I2SDF_UF_RLX);
  for (int32_t left = x; p != x && left > 0; --left) {      // (every step descends: at most x of them)
    const int32_t g = __hip_atomic_load(parent + p, I2SDF_UF_RLX);
    if (g != p) __hip_atomic_store(parent + x, g, I2SDF_UF_RLX);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
  for (int32_t left = a > b ? a : b; left >= 0; --left) {   // (a lost swap continues below the index it lost at)
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;                                       // hi was hooked by somebody else meanwhile: go on from its new parent
    b = lo;
  }
}

}  // namespace i2sdf_unionfind
