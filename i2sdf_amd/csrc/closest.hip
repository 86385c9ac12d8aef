// Point-to-mesh queries on the device: the closest point of a triangle mesh, its distance, and the sign by angle-weighted
// pseudonormals (Baerentzen and Aanaes).  include/i2sdf.h, section "Closest point", states the law and derives the box slack;
// tri_closest.h holds the per-face rule and the box bound (shared with host code); tests/closest_ref.py restates both in numpy.
// The tree is the one bvh.hip builds (bvh_tree.h): nothing is added to its buffer.
//
//   tree      one lane per query; a node is one 64-byte fetch, a leaf one 48-byte fetch; the child with the smaller box distance
//             first, the other on the lane's stack: 64 int32 slots per lane in LDS, interleaved by lane as in bvh_trace_kernel
//             (32 KiB per 128-thread workgroup).  The skip threshold is recomputed (one sqrt) only when the best d^2 improves.
//   brute     every query against every face through the same tri_closest: 256 faces at a time staged in LDS, read by all lanes at
//             once (one address per wave: a broadcast).
//   normals   keys: one corner key (the vertex) and one half-edge key (min << 32 | max) per face corner, INT64_MAX for faces that
//             are never closest; the CALLER sorts each half stably with its permutation; reduce: the lane at the head of a run sums
//             the run in order (ascending corner index = ascending face index) in fp64 and rounds once.  No floating-point atomics.
// Every result is an order-free function of the inputs: the smallest d^2, then the smallest face index.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "bvh_tree.h"
#include "tri_closest.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;
using namespace i2sdf_bvh;
using i2sdf::ClosestHit;

constexpr int CP_THREADS = 128, CP_STACK = 64;
constexpr int CB_THREADS = 256;
constexpr int CN_THREADS = 256, CN_MAX_BLOCKS = 4096;
constexpr int64_t NO_KEY = INT64_MAX;

struct Best {
  double d2, c0, c1, c2;
  float u, v;
  int32_t face, feature;
};

__device__ __forceinline__ void take(Best& b, const ClosestHit& h, int32_t face) {
  b.d2 = h.d2; b.c0 = h.c0; b.c1 = h.c1; b.c2 = h.c2;
  b.u = (float)h.u; b.v = (float)h.v;
  b.face = face; b.feature = h.feature;
}

struct Query {
  double p0, p1, p2;
  bool ok;
};

__device__ __forceinline__ Query load_query(const float* __restrict__ points, int64_t i) {
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  Query q;
  q.p0 = (double)x; q.p1 = (double)y; q.p2 = (double)z;
  q.ok = i2sdf::finite_f(x) && i2sdf::finite_f(y) && i2sdf::finite_f(z);
  return q;
}

// one valid face against the query: the rule, then (only for a face that would displace the best) the zero-area test
__device__ __forceinline__ void offer(Best& b, const Query& q, double bound, float a0, float a1, float a2, float b0, float b1, float b2,
                                      float c0, float c1, float c2, int32_t face) {
  ClosestHit h;
  i2sdf::tri_closest(q.p0, q.p1, q.p2, a0, a1, a2, b0, b1, b2, c0, c1, c2, h);
  if (i2sdf::closest_takes(h.d2, face, bound, b.d2, b.face) && !i2sdf::tri_degenerate(a0, a1, a2, b0, b1, b2, c0, c1, c2)) take(b, h, face);
}

// the outputs of one query; the sign needs the face again (its vertex indices, and its own normal for the FACE feature)
__device__ __forceinline__ void store_query(const Best& b, const Query& q, int64_t i, const float* __restrict__ verts, int64_t V,
                                            const int32_t* __restrict__ faces, int64_t F, const float* __restrict__ vnormal,
                                            const float* __restrict__ enormal, float* __restrict__ dist, float* __restrict__ point,
                                            int32_t* __restrict__ face, float* __restrict__ bary, uint8_t* __restrict__ feature,
                                            float* __restrict__ sdist) {
  const bool hit = b.face >= 0;
  const float d = hit ? (float)sqrt(b.d2) : INFINITY;
  dist[i] = d;
  point[3 * i] = hit ? (float)b.c0 : 0.0f;
  point[3 * i + 1] = hit ? (float)b.c1 : 0.0f;
  point[3 * i + 2] = hit ? (float)b.c2 : 0.0f;
  face[i] = b.face;
  bary[2 * i] = hit ? b.u : 0.0f;
  bary[2 * i + 1] = hit ? b.v : 0.0f;
  feature[i] = hit ? (uint8_t)b.feature : (uint8_t)0;
  if (!sdist) return;
  if (!hit) { sdist[i] = INFINITY; return; }
  const int64_t f = b.face;
  if (f >= F) { sdist[i] = __uint_as_float(0x7fc00000u); return; }      // (a leaf that is not this mesh's)
  const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  // (a face that counted has valid indices -- unless the mesh changed under its tree: no sign then, and no read outside the tables)
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) { sdist[i] = __uint_as_float(0x7fc00000u); return; }
  double n0, n1, n2;
  if (b.feature == i2sdf::CP_FACE) {
    const float* A = verts + 3 * (int64_t)i0;
    const float* B = verts + 3 * (int64_t)i1;
    const float* C = verts + 3 * (int64_t)i2;
    i2sdf::tri_cross(A[0], A[1], A[2], B[0], B[1], B[2], C[0], C[1], C[2], n0, n1, n2);
  } else {
    const float* N;
    if (b.feature <= i2sdf::CP_EDGE_CA) N = enormal + 9 * f + 3 * (b.feature - i2sdf::CP_EDGE_AB);
    else N = vnormal + 3 * (int64_t)(b.feature == i2sdf::CP_VERT_A ? i0 : (b.feature == i2sdf::CP_VERT_B ? i1 : i2));
    n0 = (double)N[0]; n1 = (double)N[1]; n2 = (double)N[2];
  }
  ClosestHit h;
  h.c0 = b.c0; h.c1 = b.c1; h.c2 = b.c2;
  sdist[i] = (float)i2sdf::closest_sign(q.p0, q.p1, q.p2, h, n0, n1, n2) * d;
}

// ---------------------------------------------------------------------------------------------- the tree route
__global__ __launch_bounds__(CP_THREADS) void closest_bvh_kernel(const Header* __restrict__ h, const Node* __restrict__ nodes,
                                                                 const Leaf* __restrict__ leaves, int64_t F, const float* __restrict__ verts,
                                                                 int64_t V, const int32_t* __restrict__ faces,
                                                                 const float* __restrict__ points, int64_t n,
                                                                 float max_dist, const float* __restrict__ vnormal,
                                                                 const float* __restrict__ enormal, float* __restrict__ dist,
                                                                 float* __restrict__ point, int32_t* __restrict__ face_out,
                                                                 float* __restrict__ bary, uint8_t* __restrict__ feature,
                                                                 float* __restrict__ sdist, int32_t* status) {
  __shared__ int32_t stack[CP_STACK * CP_THREADS];
  const int64_t i = (int64_t)blockIdx.x * CP_THREADS + threadIdx.x;
  if (i == 0 && (h->flags & I2SDF_RAYCAST_BAD_FACE)) atomicOr(status, I2SDF_CLOSEST_BAD_FACE);
  if (i >= n) return;                              // (no barrier below)
  const Query q = load_query(points, i);
  const double bound = (double)max_dist * (double)max_dist;
  Best b{bound, 0.0, 0.0, 0.0, 0.0f, 0.0f, -1, 0};
  if (!q.ok) atomicOr(status, I2SDF_CLOSEST_BAD_POINT);
  if (q.ok && F > 0) {
    // the largest coordinate magnitude of the query and of the mesh's bounds (fmax ignores the NaN images of an empty mesh)
    double M = fmax(fabs(q.p0), fmax(fabs(q.p1), fabs(q.p2)));
#pragma unroll
    for (int k = 0; k < 3; ++k) M = fmax(M, fmax(fabs((double)f_dec(h->bounds[k])), fabs((double)f_dec(h->bounds[4 + k]))));
    double skip = i2sdf::box_skip_above(b.d2, M);
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
          if (face >= 0) {
            const int32_t before = b.face;
            const double d2_before = b.d2;
            offer(b, q, bound, a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x, face);
            if (b.face != before || b.d2 != d2_before) skip = i2sdf::box_skip_above(b.d2, M);
          }
        }
      } else if (cur < F - 1) {
        const float4* p = (const float4*)(nodes + cur);
        const float4 a = p[0], c = p[1], e = p[2], g = p[3];
        const double q0 = i2sdf::box_dist2(q.p0, q.p1, q.p2, a.x, a.y, a.z, a.w, c.x, c.y);
        const double q1 = i2sdf::box_dist2(q.p0, q.p1, q.p2, c.z, c.w, e.x, e.y, e.z, e.w);
        const bool h0 = !(q0 > skip), h1 = !(q1 > skip);
        const int32_t c0 = __float_as_int(g.x), c1 = __float_as_int(g.y);
        if (h0 && h1) {
          const bool first0 = q0 <= q1;
          if (sp < CP_STACK) { my[sp * CP_THREADS] = first0 ? c1 : c0; ++sp; }
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
        cur = my[sp * CP_THREADS];
      }
    }
  }
  store_query(b, q, i, verts, V, faces, F, vnormal, enormal, dist, point, face_out, bary, feature, sdist);
}

// ---------------------------------------------------------------------------------------------- the brute route
__global__ __launch_bounds__(CN_THREADS) void closest_faces_check_kernel(const float* __restrict__ verts, int64_t V,
                                                                         const int32_t* __restrict__ faces, int64_t F, int32_t* status) {
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * CN_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * CN_THREADS) {
    float v[9];
    if (!load_face(verts, V, faces, f, v)) bad = 1;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, I2SDF_CLOSEST_BAD_FACE);
}

__global__ __launch_bounds__(CB_THREADS) void closest_brute_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                   int64_t F, const float* __restrict__ points, int64_t n, float max_dist,
                                                                   const float* __restrict__ vnormal, const float* __restrict__ enormal,
                                                                   float* __restrict__ dist, float* __restrict__ point,
                                                                   int32_t* __restrict__ face_out, float* __restrict__ bary,
                                                                   uint8_t* __restrict__ feature, float* __restrict__ sdist, int32_t* status) {
  __shared__ float tile[CB_THREADS][10];           // nine coordinates and the valid flag of 256 faces
  const int64_t i = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
  Query q;
  q.ok = false;
  q.p0 = q.p1 = q.p2 = 0.0;
  if (i < n) {
    q = load_query(points, i);
    if (!q.ok) atomicOr(status, I2SDF_CLOSEST_BAD_POINT);
  }
  const double bound = (double)max_dist * (double)max_dist;
  Best b{bound, 0.0, 0.0, 0.0, 0.0f, 0.0f, -1, 0};
  for (int64_t f0 = 0; f0 < F; f0 += CB_THREADS) {           // (every thread of the workgroup takes every turn: barriers inside)
    const int64_t f = f0 + threadIdx.x;
    float v[9];
    bool ok = false;
    if (f < F) ok = load_face(verts, V, faces, f, v);
#pragma unroll
    for (int k = 0; k < 9; ++k) tile[threadIdx.x][k] = ok ? v[k] : 0.0f;
    tile[threadIdx.x][9] = ok ? 1.0f : 0.0f;
    __syncthreads();
    const int m = (int)(F - f0 < CB_THREADS ? F - f0 : CB_THREADS);
    if (q.ok) {
      for (int k = 0; k < m; ++k) {
        const float* t = tile[k];
        if (t[9] != 0.0f) offer(b, q, bound, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], (int32_t)(f0 + k));
      }
    }
    __syncthreads();
  }
  if (i < n) store_query(b, q, i, verts, V, faces, F, vnormal, enormal, dist, point, face_out, bary, feature, sdist);
}

// ---------------------------------------------------------------------------------------------- pseudonormal tables
// the nine coordinates (fp64 images) of a face that may be closest, or false
__device__ __forceinline__ bool load_face_d(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t f, double P[9]) {
  float v[9];
  if (!load_face(verts, V, faces, f, v)) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = (double)v[k];
  return !i2sdf::tri_degenerate(P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8]);
}

__global__ __launch_bounds__(CN_THREADS) void closest_normal_keys_kernel(const float* __restrict__ verts, int64_t V,
                                                                         const int32_t* __restrict__ faces, int64_t F,
                                                                         int64_t* __restrict__ keys, int32_t* status) {
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * CN_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * CN_THREADS) {
    float v[9];
    bool ok = load_face(verts, V, faces, f, v);
    if (!ok) bad = 1;
    ok = ok && !i2sdf::tri_degenerate(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const int64_t a[3] = {i0, i1, i2}, b[3] = {i1, i2, i0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t lo = a[k] < b[k] ? a[k] : b[k], hi = a[k] < b[k] ? b[k] : a[k];
      keys[3 * f + k] = ok ? a[k] : NO_KEY;                              // corner k: the vertex
      keys[3 * F + 3 * f + k] = ok ? ((lo << 32) | hi) : NO_KEY;         // half-edge k: AB, BC, CA
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, I2SDF_CLOSEST_BAD_FACE);
}

// the unit normal of a face that may be closest
__device__ __forceinline__ void unit_normal(const double P[9], double& n0, double& n1, double& n2) {
  i2sdf::tri_cross(P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], n0, n1, n2);
  const double len = sqrt(i2sdf::cp_dot(n0, n1, n2, n0, n1, n2));
  n0 = n0 / len; n1 = n1 / len; n2 = n2 / len;
}

__global__ __launch_bounds__(CN_THREADS) void closest_normal_reduce_kernel(const float* __restrict__ verts, int64_t V,
                                                                           const int32_t* __restrict__ faces, int64_t F,
                                                                           const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                                                                           float* __restrict__ vnormal, float* __restrict__ enormal) {
  const int64_t n3 = 3 * F;
  for (int64_t t = (int64_t)blockIdx.x * CN_THREADS + threadIdx.x; t < 2 * n3; t += (int64_t)gridDim.x * CN_THREADS) {
    const bool edge = t >= n3;
    const int64_t base = edge ? n3 : 0, j = t - base;      // each half was sorted on its own: perm counts inside the half
    const int64_t key = skeys[t];
    if (key == NO_KEY || (j > 0 && skeys[t - 1] == key)) continue;       // only the head of a run works
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int64_t end = j;
    for (; end < n3 && skeys[base + end] == key; ++end) {
      const int64_t c = perm[base + end];
      if (c < 0 || c >= n3) continue;              // (a permutation that is not this sort's)
      const int64_t f = c / 3;
      const int k = (int)(c - 3 * f);
      double P[9], n0, n1, n2;
      if (!load_face_d(verts, V, faces, f, P)) continue;
      unit_normal(P, n0, n1, n2);
      double w = 1.0;
      if (!edge) {                                 // the angle at corner k between the edges to the next and to the previous vertex
        const int o = 3 * k, o1 = 3 * (k == 2 ? 0 : k + 1), o2 = 3 * (k == 0 ? 2 : k - 1);
        const double e0 = P[o1] - P[o], e1 = P[o1 + 1] - P[o + 1], e2 = P[o1 + 2] - P[o + 2];
        const double g0 = P[o2] - P[o], g1 = P[o2 + 1] - P[o + 1], g2 = P[o2 + 2] - P[o + 2];
        const double x0 = e1 * g2 - e2 * g1, x1 = e2 * g0 - e0 * g2, x2 = e0 * g1 - e1 * g0;
        w = atan2(sqrt(i2sdf::cp_dot(x0, x1, x2, x0, x1, x2)), i2sdf::cp_dot(e0, e1, e2, g0, g1, g2));
      }
      s0 = s0 + w * n0; s1 = s1 + w * n1; s2 = s2 + w * n2;
    }
    if (!edge) {
      if (key < 0 || key >= V) continue;           // (keys that are not this mesh's)
      float* o = vnormal + 3 * key;
      o[0] = (float)s0; o[1] = (float)s1; o[2] = (float)s2;
    } else {
      for (int64_t r = j; r < end; ++r) {
        const int64_t c = perm[base + r];
        if (c < 0 || c >= n3) continue;
        float* o = enormal + 3 * c;                // [face][edge][3], c = 3 face + edge
        o[0] = (float)s0; o[1] = (float)s1; o[2] = (float)s2;
      }
    }
  }
}

inline unsigned face_blocks(int64_t F) { return blocks(F, CN_THREADS, CN_MAX_BLOCKS); }
inline bool dist_ok(float max_dist) { return max_dist >= 0.0f; }      // (+inf passes, a NaN does not)
inline bool query_ok(const float* points, int64_t n, float max_dist, const float* vnormal, const float* enormal, const float* dist,
                     const float* point, const int32_t* face, const float* bary, const uint8_t* feature, const float* sdist,
                     const int32_t* status) {
  if (n < 0 || n > INT32_MAX || !dist_ok(max_dist) || !aligned(status, 4)) return false;
  if ((vnormal != nullptr) != (enormal != nullptr) || (vnormal != nullptr) != (sdist != nullptr)) return false;       // all three or none
  if (vnormal && (!aligned(vnormal, 4) || !aligned(enormal, 4) || !aligned(sdist, 4))) return false;
  if (n == 0) return true;
  return aligned(points, 4) && aligned(dist, 4) && aligned(point, 4) && aligned(face, 4) && aligned(bary, 4) && feature;
}

}  // namespace

extern "C" int i2sdf_closest_bvh(const void* bvh, const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points,
                                 int64_t n, float max_dist, const float* vnormal, const float* enormal, float* dist, float* point,
                                 int32_t* face, float* bary, uint8_t* feature, float* sdist, int32_t* status, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !aligned(bvh, 16) ||
      !query_ok(points, n, max_dist, vnormal, enormal, dist, point, face, bary, feature, sdist, status))
    return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "closest status")) return rc;
  const Layout w = layout(F);
  const char* base = (const char*)bvh;
  // (n = 0 still launches one workgroup: the face bit of the build reaches *status)
  closest_bvh_kernel<<<blocks(n, CP_THREADS, INT32_MAX), CP_THREADS, 0, st>>>((const Header*)base, (const Node*)(base + w.nodes),
                                                                             (const Leaf*)(base + w.leaves), F, verts, V, faces, points, n,
                                                                             max_dist, vnormal, enormal, dist, point, face, bary, feature,
                                                                             sdist, status);
  return i2sdf_hip_check(hipGetLastError(), "closest_bvh_kernel");
}

extern "C" int i2sdf_closest_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points, int64_t n,
                                   float max_dist, const float* vnormal, const float* enormal, float* dist, float* point, int32_t* face,
                                   float* bary, uint8_t* feature, float* sdist, int32_t* status, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !query_ok(points, n, max_dist, vnormal, enormal, dist, point, face, bary, feature, sdist, status))
    return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "closest status")) return rc;
  if (F > 0) {
    closest_faces_check_kernel<<<face_blocks(F), CN_THREADS, 0, st>>>(verts, V, faces, F, status);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "closest_faces_check_kernel")) return rc;
  }
  if (n == 0) return I2SDF_OK;
  closest_brute_kernel<<<blocks(n, CB_THREADS), CB_THREADS, 0, st>>>(verts, V, faces, F, points, n, max_dist, vnormal, enormal, dist, point,
                                                                    face, bary, feature, sdist, status);
  return i2sdf_hip_check(hipGetLastError(), "closest_brute_kernel");
}

extern "C" int i2sdf_closest_normal_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, int64_t* keys, int32_t* status,
                                         void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !aligned(status, 4) || (F > 0 && !aligned(keys, 8))) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "closest status")) return rc;
  if (F == 0) return I2SDF_OK;
  closest_normal_keys_kernel<<<face_blocks(F), CN_THREADS, 0, st>>>(verts, V, faces, F, keys, status);
  return i2sdf_hip_check(hipGetLastError(), "closest_normal_keys_kernel");
}

extern "C" int i2sdf_closest_normals(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys,
                                     const int64_t* perm, float* vnormal, float* enormal, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || (F > 0 && (!aligned(sorted_keys, 8) || !aligned(perm, 8) || !aligned(enormal, 4))) ||
      (V > 0 && !aligned(vnormal, 4)))
    return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (V > 0)
    if (int rc = i2sdf_hip_check(hipMemsetAsync(vnormal, 0, 12 * (size_t)V, st), "closest vnormal")) return rc;
  if (F == 0) return I2SDF_OK;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(enormal, 0, 36 * (size_t)F, st), "closest enormal")) return rc;
  closest_normal_reduce_kernel<<<face_blocks(6 * F), CN_THREADS, 0, st>>>(verts, V, faces, F, sorted_keys, perm, vnormal, enormal);
  return i2sdf_hip_check(hipGetLastError(), "closest_normal_reduce_kernel");
}
