// Ray casting against a triangle mesh on the device: a linear BVH (Karras 2012) over the faces and a watertight trace through it --
// the external ray caster the reference's `intersect_func` hook is meant for, on the mesh this library extracts itself.  include/i2sdf.h,
// section "Ray casting", states the law and derives the box test; tri_isect.h holds the per-face rule and the box test (shared with host
// code); tests/raycast_ref.py restates rule, keys and topology in numpy.
//
//   bounds    min / max of the vertices of the valid faces: wave reductions, then 32-bit atomicMin / Max on order-preserving images.
//   keys      centroid -> 10 bits per axis inside those bounds (fp64) -> 30-bit Morton code -> key = code << 32 | face.  A face with
//             an index outside [0, V) or a non-finite vertex takes code 2^30: such faces sort last and own subtrees with empty boxes.
//             The CALLER sorts the keys (they are unique; the face index rides in the low word, no permutation is needed).
//   leaves    sorted entry j -> one 48-byte record: the three vertices and the face index (-1: never hit).
//   topology  Karras' construction: one thread per internal node finds its range and split by binary searches on the common-prefix
//             length of the sorted keys; node 0 is the root.  Children and parent links only, no box yet.
//   boxes     one thread per leaf walks up; at every internal node it stores the box it brings into that child's slot of the node and
//             counts itself in; the first to arrive leaves, the second (fence, then reads the sibling's slot) carries the union up.
//             No thread waits for another.  min and max are `b < a ? b : a` in slot order, so a box does not depend on who arrived first.
//   trace     one lane per ray; a node is one 64-byte fetch (both children's boxes and links), a leaf one 48-byte fetch; the nearer
//             child first, the farther one pushed on the lane's stack: 64 int32 slots per lane in LDS, interleaved by lane (slot s of lane
//             l at [s * 128 + l]: no bank conflicts), 32 KiB per 128-thread workgroup, five workgroups per CU by LDS.  The key has 63
//             significant bits, so the tree is at most 63 deep and the stack never holds more than that.  No scratch.
//   brute     every ray against every face through the same tri_hit: 256 faces at a time staged in LDS and read by all lanes at once
//             (one address per wave: a broadcast).
// Every result is an order-free function of the inputs: the smallest t, then the smallest face index.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "tri_isect.h"
#include "bvh_tree.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;
using namespace i2sdf_bvh;
using i2sdf::RayShear;

constexpr int BV_THREADS = 256, BV_MAX_BLOCKS = 4096;
constexpr int TR_THREADS = 128, TR_STACK = 64;
constexpr int BR_THREADS = 256;
constexpr uint32_t BAD_CODE = 1u << 30;

// ---------------------------------------------------------------------------------------------- bounds and keys
__global__ __launch_bounds__(BV_THREADS) void bvh_bounds_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                int64_t F, Header* h) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * BV_THREADS) {
    float v[9];
    if (!load_face(verts, V, faces, f, v)) { bad = 1; continue; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], fminf(v[k], fminf(v[3 + k], v[6 + k])));
      hi[k] = fmaxf(hi[k], fmaxf(v[k], fmaxf(v[3 + k], v[6 + k])));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float l = wave_min(lo[k]), m = wave_max(hi[k]);
    if ((threadIdx.x & 63) == 0 && l <= m) {
      atomicMin(&h->bounds[k], f_enc(l));
      atomicMax(&h->bounds[4 + k], f_enc(m));
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&h->flags, I2SDF_RAYCAST_BAD_FACE);
}

__device__ __forceinline__ uint32_t spread10(uint32_t x) {      // abcdefghij -> a00b00c00...j
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

__global__ __launch_bounds__(BV_THREADS) void bvh_keys_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                              int64_t F, const Header* h, int64_t* __restrict__ keys) {
  double lo[3], ext[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = (double)f_dec(h->bounds[k]);
    ext[k] = (double)f_dec(h->bounds[4 + k]) - lo[k];
  }
  for (int64_t f = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * BV_THREADS) {
    float v[9];
    uint32_t code = BAD_CODE;
    if (load_face(verts, V, faces, f, v)) {
      uint32_t q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double c = (((double)v[k] + (double)v[3 + k]) + (double)v[6 + k]) / 3.0;
        double s = ext[k] > 0.0 ? floor(((c - lo[k]) / ext[k]) * 1024.0) : 0.0;
        s = s >= 0.0 ? s : 0.0;                  // (a NaN quotient too)
        q[k] = s > 1023.0 ? 1023u : (uint32_t)s;
      }
      code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    }
    keys[f] = (int64_t)(((uint64_t)code << 32) | (uint64_t)(uint32_t)f);
  }
}

// ---------------------------------------------------------------------------------------------- leaves, topology, boxes
__global__ __launch_bounds__(BV_THREADS) void bvh_leaves_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                int64_t F, const int64_t* __restrict__ skeys, Leaf* __restrict__ leaves,
                                                                int32_t* __restrict__ counter) {
  const float nan = __uint_as_float(0x7fc00000u);
  for (int64_t j = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; j < F; j += (int64_t)gridDim.x * BV_THREADS) {
    const int64_t f = (int64_t)(uint32_t)((uint64_t)skeys[j] & 0xffffffffu);
    Leaf l;
    l.pad[0] = l.pad[1] = 0;
    const bool ok = f < F && load_face(verts, V, faces, f, l.v);      // (keys that are not this mesh's: the leaf holds no face)
    l.face = ok ? (int32_t)f : -1;
    if (!ok) {
#pragma unroll
      for (int k = 0; k < 9; ++k) l.v[k] = nan;
    }
    leaves[j] = l;
    counter[j] = 0;
  }
}

// length of the common prefix of sorted keys i and j, -1 when j is outside the array
__device__ __forceinline__ int delta(const int64_t* __restrict__ k, int64_t F, int64_t i, int64_t j) {
  if (j < 0 || j >= F) return -1;
  const uint64_t x = (uint64_t)k[i] ^ (uint64_t)k[j];
  return x ? __clzll((long long)x) : 64;         // (equal keys cannot come from i2sdf_bvh_keys; 64 keeps the searches finite)
}

__global__ __launch_bounds__(BV_THREADS) void bvh_topology_kernel(const int64_t* __restrict__ k, int64_t F, Node* __restrict__ nodes,
                                                                  int32_t* __restrict__ nparent, int32_t* __restrict__ lparent) {
  for (int64_t i = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; i < F - 1; i += (int64_t)gridDim.x * BV_THREADS) {
    const int64_t d = delta(k, F, i, i + 1) - delta(k, F, i, i - 1) < 0 ? -1 : 1;
    const int dmin = delta(k, F, i, i - d);
    int64_t lmax = 2;
    while (delta(k, F, i, i + lmax * d) > dmin) lmax *= 2;           // (ends: beyond the array delta is -1 <= dmin)
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
      if (delta(k, F, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = delta(k, F, i, j);
    int64_t s = 0, t = l;
    do {
      t = (t + 1) / 2;
      if (delta(k, F, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);
    const int64_t first = i < j ? i : j, last = i < j ? j : i;
    if (g < 0 || g + 1 >= F) continue;             // (cannot happen with sorted unique keys)
    const int32_t me0 = (int32_t)(i << 1), me1 = (int32_t)(i << 1) | 1;
    if (first == g) { nodes[i].child[0] = ~(int32_t)g; lparent[g] = me0; } else { nodes[i].child[0] = (int32_t)g; nparent[g] = me0; }
    if (last == g + 1) { nodes[i].child[1] = ~(int32_t)(g + 1); lparent[g + 1] = me1; } else { nodes[i].child[1] = (int32_t)(g + 1); nparent[g + 1] = me1; }
    nodes[i].pad[0] = nodes[i].pad[1] = 0;
  }
}

__global__ __launch_bounds__(BV_THREADS) void bvh_boxes_kernel(const Leaf* __restrict__ leaves, int64_t F, Node* nodes,
                                                               const int32_t* __restrict__ nparent, const int32_t* __restrict__ lparent,
                                                               int32_t* counter) {
  for (int64_t j = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; j < F; j += (int64_t)gridDim.x * BV_THREADS) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (leaves[j].face >= 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float a = leaves[j].v[k], b = leaves[j].v[3 + k], c = leaves[j].v[6 + k];
        lo[k] = min_f(min_f(a, b), c);
        hi[k] = max_f(max_f(a, b), c);
      }
    }
    int32_t link = lparent[j];
    for (int up = 0; up < 64; ++up) {              // (the tree is at most 63 deep)
      const int64_t p = link >> 1;
      const int slot = link & 1;
      if (p < 0 || p >= F - 1) break;
      float* mine = slot ? nodes[p].lo1 : nodes[p].lo0;      // lo then hi: six floats
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        __hip_atomic_store(mine + k, lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 3 + k, hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __threadfence();
      if (atomicAdd(&counter[p], 1) == 0) break;   // the sibling has not arrived: it will carry the union up
      __threadfence();
      const float* other = slot ? nodes[p].lo0 : nodes[p].lo1;
      float olo[3], ohi[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        olo[k] = __hip_atomic_load(other + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ohi[k] = __hip_atomic_load(other + 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {                // slot 0 first, whoever arrived first
        lo[k] = slot ? min_f(olo[k], lo[k]) : min_f(lo[k], olo[k]);
        hi[k] = slot ? max_f(ohi[k], hi[k]) : max_f(hi[k], ohi[k]);
      }
      if (p == 0) break;                           // the root
      link = nparent[p];
    }
  }
}

// ---------------------------------------------------------------------------------------------- rays
struct Ray {
  RayShear r;
  float t_min, t_max;
  bool ok;
};

__device__ __forceinline__ Ray load_ray(const float* __restrict__ orig, const float* __restrict__ dirs, const float* __restrict__ t_min,
                                        const float* __restrict__ t_max, int64_t i) {
  Ray y;
  y.t_min = t_min[i];
  y.t_max = t_max[i];
  y.ok = i2sdf::ray_shear(orig[3 * i], orig[3 * i + 1], orig[3 * i + 2], dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], y.r);
  if (y.t_min != y.t_min || y.t_max != y.t_max) y.ok = false;
  return y;
}

struct Best {
  float t, u, v;
  int32_t face;
};

__device__ __forceinline__ void offer(Best& b, float t, float u, float v, int32_t face) {
  if (t < b.t || b.face < 0 || face < b.face) {    // (tri_hit has already required t <= b.t)
    b.t = t; b.u = u; b.v = v; b.face = face;
  }
}

__device__ __forceinline__ void store_ray(const Best& b, int64_t i, int any_hit, float* __restrict__ t, int32_t* __restrict__ face,
                                          float* __restrict__ bary, uint8_t* __restrict__ hit) {
  hit[i] = b.face >= 0;
  if (any_hit) return;
  t[i] = b.t;
  face[i] = b.face;
  bary[2 * i] = b.u;
  bary[2 * i + 1] = b.v;
}

__global__ __launch_bounds__(TR_THREADS) void bvh_trace_kernel(const Header* __restrict__ h, const Node* __restrict__ nodes,
                                                               const Leaf* __restrict__ leaves, int64_t F, const float* __restrict__ orig,
                                                               const float* __restrict__ dirs, const float* __restrict__ t_min,
                                                               const float* __restrict__ t_max, int64_t n, int cull, int any_hit,
                                                               float* __restrict__ t_out, int32_t* __restrict__ face_out,
                                                               float* __restrict__ bary_out, uint8_t* __restrict__ hit_out, int32_t* status) {
  __shared__ int32_t stack[TR_STACK * TR_THREADS];
  const int64_t i = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i == 0 && h->flags) atomicOr(status, h->flags);
  if (i >= n) return;                              // (no barrier below)
  const Ray y = load_ray(orig, dirs, t_min, t_max, i);
  Best b{y.t_max, 0.0f, 0.0f, -1};
  if (!y.ok) atomicOr(status, I2SDF_RAYCAST_BAD_RAY);
  if (y.ok && F > 0) {
    int32_t* my = stack + threadIdx.x;
    int sp = 0;
    int32_t cur = F == 1 ? ~0 : 0;
    for (int64_t visit = 0; visit < 2 * F; ++visit) {        // a tree of F leaves has 2 F - 1 nodes: a malformed buffer cannot loop
      bool pop = true;
      if (cur < 0) {
        const int64_t j = ~cur;
        if (j < F) {
          const float4* p = (const float4*)(leaves + j);
          const float4 a = p[0], c = p[1], e = p[2];
          const int32_t face = __float_as_int(e.y);
          float t, u, v;
          if (face >= 0 && i2sdf::tri_hit(y.r, a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x, y.t_min, b.t, cull, t, u, v)) {
            offer(b, t, u, v, face);
            if (any_hit) break;
          }
        }
      } else if (cur < F - 1) {
        const float4* p = (const float4*)(nodes + cur);
        const float4 a = p[0], c = p[1], e = p[2], g = p[3];
        float n0, n1;
        const bool h0 = i2sdf::box_may_hit(y.r, a.x, a.y, a.z, a.w, c.x, c.y, y.t_min, b.t, n0);
        const bool h1 = i2sdf::box_may_hit(y.r, c.z, c.w, e.x, e.y, e.z, e.w, y.t_min, b.t, n1);
        const int32_t c0 = __float_as_int(g.x), c1 = __float_as_int(g.y);
        if (h0 && h1) {
          const bool first0 = n0 <= n1;
          if (sp < TR_STACK) { my[sp * TR_THREADS] = first0 ? c1 : c0; ++sp; }
          cur = first0 ? c0 : c1;
          pop = false;
        } else if (h0 || h1) {
          cur = h0 ? c0 : c1;
          pop = false;
        }
      }
      if (pop) {
        if (sp == 0) break;
        --sp;
        cur = my[sp * TR_THREADS];
      }
    }
  }
  store_ray(b, i, any_hit, t_out, face_out, bary_out, hit_out);
}

__global__ __launch_bounds__(BV_THREADS) void mesh_faces_check_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                      int64_t F, int32_t* status) {
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * BV_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * BV_THREADS) {
    float v[9];
    if (!load_face(verts, V, faces, f, v)) bad = 1;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, I2SDF_RAYCAST_BAD_FACE);
}

__global__ __launch_bounds__(BR_THREADS) void mesh_trace_brute_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                      int64_t F, const float* __restrict__ orig, const float* __restrict__ dirs,
                                                                      const float* __restrict__ t_min, const float* __restrict__ t_max, int64_t n,
                                                                      int cull, int any_hit, float* __restrict__ t_out,
                                                                      int32_t* __restrict__ face_out, float* __restrict__ bary_out,
                                                                      uint8_t* __restrict__ hit_out, int32_t* status) {
  __shared__ float tile[BR_THREADS][10];           // nine coordinates and the valid flag of 256 faces
  const int64_t i = (int64_t)blockIdx.x * BR_THREADS + threadIdx.x;
  Ray y;
  y.ok = false;
  y.t_min = y.t_max = 0.0f;
  if (i < n) {
    y = load_ray(orig, dirs, t_min, t_max, i);
    if (!y.ok) atomicOr(status, I2SDF_RAYCAST_BAD_RAY);
  }
  Best b{y.t_max, 0.0f, 0.0f, -1};
  for (int64_t f0 = 0; f0 < F; f0 += BR_THREADS) {           // (every thread of the workgroup takes every turn: barriers inside)
    const int64_t f = f0 + threadIdx.x;
    float v[9];
    bool ok = false;
    if (f < F) ok = load_face(verts, V, faces, f, v);
#pragma unroll
    for (int k = 0; k < 9; ++k) tile[threadIdx.x][k] = ok ? v[k] : 0.0f;
    tile[threadIdx.x][9] = ok ? 1.0f : 0.0f;
    __syncthreads();
    const int m = (int)(F - f0 < BR_THREADS ? F - f0 : BR_THREADS);
    if (y.ok && !(any_hit && b.face >= 0)) {
      for (int k = 0; k < m; ++k) {
        const float* q = tile[k];
        float t, u, w;
        if (q[9] != 0.0f && i2sdf::tri_hit(y.r, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], y.t_min, b.t, cull, t, u, w))
          offer(b, t, u, w, (int32_t)(f0 + k));
      }
    }
    __syncthreads();
  }
  if (i < n) store_ray(b, i, any_hit, t_out, face_out, bary_out, hit_out);
}

inline unsigned face_blocks(int64_t F) { return blocks(F, BV_THREADS, BV_MAX_BLOCKS); }
inline bool rays_ok(const float* orig, const float* dirs, const float* t_min, const float* t_max, int64_t n, int32_t cull, int32_t any_hit,
                    const float* t, const int32_t* face, const float* bary, const uint8_t* hit, const int32_t* status) {
  if (n < 0 || n > INT32_MAX || (cull != I2SDF_RAYCAST_CULL_NONE && cull != I2SDF_RAYCAST_CULL_BACK) || (any_hit != 0 && any_hit != 1)) return false;
  if (!aligned(status, 4)) return false;
  if (n == 0) return true;
  if (!aligned(orig, 4) || !aligned(dirs, 4) || !aligned(t_min, 4) || !aligned(t_max, 4) || !hit) return false;
  return any_hit || (aligned(t, 4) && aligned(face, 4) && aligned(bary, 4));
}

}  // namespace

extern "C" int64_t i2sdf_bvh_bytes(int64_t F) {
  if (!size_ok(F)) return 0;
  return layout(F).bytes;
}

extern "C" int i2sdf_bvh_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, void* bvh, int64_t* keys, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !aligned(bvh, 16) || (F > 0 && !aligned(keys, 8))) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  Header* h = (Header*)bvh;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(h, 0, BVH_HEADER, st), "bvh header")) return rc;
  if (F == 0) return I2SDF_OK;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(h->bounds, 0xff, 16, st), "bvh bounds")) return rc;      // minima start at the top
  bvh_bounds_kernel<<<face_blocks(F), BV_THREADS, 0, st>>>(verts, V, faces, F, h);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "bvh_bounds_kernel")) return rc;
  bvh_keys_kernel<<<face_blocks(F), BV_THREADS, 0, st>>>(verts, V, faces, F, h, keys);
  return i2sdf_hip_check(hipGetLastError(), "bvh_keys_kernel");
}

extern "C" int i2sdf_bvh_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys, void* bvh,
                               void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !aligned(bvh, 16) || (F > 0 && !aligned(sorted_keys, 8))) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  hipStream_t st = (hipStream_t)stream;
  const Layout w = layout(F);
  char* base = (char*)bvh;
  Node* nodes = (Node*)(base + w.nodes);
  Leaf* leaves = (Leaf*)(base + w.leaves);
  int32_t *nparent = (int32_t*)(base + w.nparent), *lparent = (int32_t*)(base + w.lparent), *counter = (int32_t*)(base + w.counter);
  bvh_leaves_kernel<<<face_blocks(F), BV_THREADS, 0, st>>>(verts, V, faces, F, sorted_keys, leaves, counter);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "bvh_leaves_kernel")) return rc;
  if (F == 1) return I2SDF_OK;                     // the tree is its leaf
  bvh_topology_kernel<<<face_blocks(F - 1), BV_THREADS, 0, st>>>(sorted_keys, F, nodes, nparent, lparent);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "bvh_topology_kernel")) return rc;
  bvh_boxes_kernel<<<face_blocks(F), BV_THREADS, 0, st>>>(leaves, F, nodes, nparent, lparent, counter);
  return i2sdf_hip_check(hipGetLastError(), "bvh_boxes_kernel");
}

extern "C" int i2sdf_bvh_trace(const void* bvh, int64_t F, const float* orig, const float* dirs, const float* t_min, const float* t_max,
                               int64_t n, int32_t cull, int32_t any_hit, float* t, int32_t* face, float* bary, uint8_t* hit, int32_t* status,
                               void* stream) {
  if (!size_ok(F) || !aligned(bvh, 16) || !rays_ok(orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "raycast status")) return rc;
  const Layout w = layout(F);
  const char* base = (const char*)bvh;
  // (n = 0 still launches one workgroup: the face bit of the build reaches *status)
  bvh_trace_kernel<<<blocks(n, TR_THREADS, INT32_MAX), TR_THREADS, 0, st>>>((const Header*)base, (const Node*)(base + w.nodes),
                                                                           (const Leaf*)(base + w.leaves), F, orig, dirs, t_min, t_max, n, cull,
                                                                           any_hit, t, face, bary, hit, status);
  return i2sdf_hip_check(hipGetLastError(), "bvh_trace_kernel");
}

extern "C" int i2sdf_mesh_trace_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* orig, const float* dirs,
                                      const float* t_min, const float* t_max, int64_t n, int32_t cull, int32_t any_hit, float* t, int32_t* face,
                                      float* bary, uint8_t* hit, int32_t* status, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !rays_ok(orig, dirs, t_min, t_max, n, cull, any_hit, t, face, bary, hit, status)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "raycast status")) return rc;
  if (F > 0) {
    mesh_faces_check_kernel<<<face_blocks(F), BV_THREADS, 0, st>>>(verts, V, faces, F, status);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "mesh_faces_check_kernel")) return rc;
  }
  if (n == 0) return I2SDF_OK;
  mesh_trace_brute_kernel<<<blocks(n, BR_THREADS), BR_THREADS, 0, st>>>(verts, V, faces, F, orig, dirs, t_min, t_max, n, cull, any_hit, t, face,
                                                                       bary, hit, status);
  return i2sdf_hip_check(hipGetLastError(), "mesh_trace_brute_kernel");
}
