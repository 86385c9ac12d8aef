// The records of the linear BVH (include/i2sdf.h, "Ray casting": header, nodes, leaves, build links) and the face loader, shared by the
// units that build and walk the tree: bvh.hip (build, ray trace) and closest.hip (closest point).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "tri_isect.h"

namespace i2sdf_bvh {

using i2sdf_blockops::align16;

constexpr int64_t BVH_HEADER = 256;

struct Header {
  uint32_t bounds[8];          // [0..2] minima, [4..6] maxima of the valid faces' vertices (order-preserving images)
  int32_t flags;               // I2SDF_RAYCAST_BAD_FACE, or 0
  int32_t pad[3];
};

struct __attribute__((aligned(16))) Node {      // 64 bytes
  float lo0[3], hi0[3], lo1[3], hi1[3];
  int32_t child[2];            // >= 0: internal node; < 0: leaf ~child
  int32_t pad[2];
};
struct __attribute__((aligned(16))) Leaf {      // 48 bytes
  float v[9];
  int32_t face;                // -1: never hit
  int32_t pad[2];
};
static_assert(sizeof(Node) == 64 && sizeof(Leaf) == 48, "record sizes are part of include/i2sdf.h");

struct Layout { int64_t nodes, leaves, nparent, lparent, counter, bytes; };

inline bool size_ok(int64_t F) { return F >= 0 && F <= I2SDF_BVH_MAX_FACES; }
inline Layout layout(int64_t F) {
  Layout w;
  int64_t o = BVH_HEADER;
  w.nodes = o;   o += 64 * F;                      // F - 1 are used
  w.leaves = o;  o += 48 * F;
  w.nparent = o; o = align16(o + 4 * F);           // parent << 1 | slot of internal node i (node 0: unused)
  w.lparent = o; o = align16(o + 4 * F);           // the same of leaf j
  w.counter = o; o = align16(o + 4 * F);           // arrivals at internal node i
  w.bytes = o;
  return w;
}

__device__ __forceinline__ uint32_t f_enc(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float f_dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
__device__ __forceinline__ float min_f(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max_f(float a, float b) { return b > a ? b : a; }

// the nine coordinates of face f, or false for a face that is never hit
__device__ __forceinline__ bool load_face(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t f, float v[9]) {
  const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = verts[3 * (int64_t)i0 + k];
    v[3 + k] = verts[3 * (int64_t)i1 + k];
    v[6 + k] = verts[3 * (int64_t)i2 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && i2sdf::finite_f(v[k]);
  return ok;
}

inline bool aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
inline bool mesh_ok(const float* verts, int64_t V, const int32_t* faces, int64_t F) {
  return size_ok(F) && V >= 0 && V <= INT32_MAX && (F == 0 || (aligned(verts, 4) && aligned(faces, 4)));
}

}  // namespace i2sdf_bvh
