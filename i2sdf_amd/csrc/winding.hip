// Generalized winding numbers on the device: inside / outside for meshes that are open, cut or only seen from one side (Jacobson et al.
// 2013), evaluated through the tree of bvh.hip with the far field of Barill et al. 2018, orders 0 and 1.  include/i2sdf.h, section
// "Winding number", states the law; tri_solid_angle.h holds the per-face term, the face moments and the far-field rule (shared with host
// code); tests/winding_ref.py restates them in numpy.  The tree buffer is only read: the moments live in a buffer of their own.
//
//   moments   one thread per leaf walks up the tree's parent links with the raw sums (area, area x centroid, area vector, first moment
//             about the centre of the root box) of what it has below; at an internal node it stores them in that node's record and counts
//             itself in at the PARENT (counters behind the table); the first to arrive leaves, the second (fence, then reads the
//             sibling: its record, or its leaf) adds child 0 + child 1 in that order and goes on.  No thread waits for another and the
//             sums do not depend on who arrived first.  A second kernel, one thread per node, turns the raw sums into the record a query
//             reads: centroid, radius (from the node's own two child boxes), N0, N1 about the centroid.
//   tree      one lane per query; a node is one 128-byte record fetch, and 16 bytes of links when it is opened; a leaf one 48-byte fetch.
//             Child 0 first, child 1 on the lane's stack: 64 int32 slots per lane in LDS, interleaved by lane as in bvh_trace_kernel
//             (32 KiB per 128-thread workgroup).  The sum is fp64 in visit order: no atomics, no scratch.
//   brute     every query against every face in ascending face order through the same tri_solid_angle: 256 faces at a time staged in
//             LDS, read by all lanes at once (one address per wave: a broadcast).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "bvh_tree.h"
#include "tri_solid_angle.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;
using namespace i2sdf_bvh;
using i2sdf::WN_RECORD;

constexpr int WM_THREADS = 256, WM_MAX_BLOCKS = 4096;
constexpr int WT_THREADS = 128, WT_STACK = 64;
constexpr int WB_THREADS = 256;

inline int64_t table_bytes(int64_t F) { return F > 1 ? 8 * WN_RECORD * (F - 1) : 0; }
inline int64_t moments_bytes(int64_t F) { return table_bytes(F) + align16(4 * (F > 1 ? F - 1 : 0)) + 16; }      // (never 0: it has an address)

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

__device__ __forceinline__ void store_winding(double* __restrict__ w_out, int64_t i, const Query& q, double sum) {
  w_out[i] = q.ok ? sum / i2sdf::WN_FOUR_PI : __longlong_as_double(0x7ff8000000000000ll);
}

// the centre of the root box (NaN for a mesh without a valid face: its moments are never read, every radius is +inf)
__device__ __forceinline__ void root_centre(const Header* __restrict__ h, double o[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = ((double)f_dec(h->bounds[k]) + (double)f_dec(h->bounds[4 + k])) * 0.5;
}

// the raw sums of leaf j (zero for a leaf that holds no face)
__device__ __forceinline__ void leaf_moments(const Leaf* __restrict__ leaves, int64_t j, const double o[3], double m[WN_RECORD]) {
  const float4* p = (const float4*)(leaves + j);
  const float4 a = p[0], c = p[1], e = p[2];
  if (__float_as_int(e.y) >= 0) {
    i2sdf::tri_moments(a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x, o[0], o[1], o[2], m);
  } else {
#pragma unroll
    for (int k = 0; k < WN_RECORD; ++k) m[k] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------- the moments
__global__ __launch_bounds__(WM_THREADS) void winding_moments_kernel(const Header* __restrict__ h, const Node* __restrict__ nodes,
                                                                     const Leaf* __restrict__ leaves, const int32_t* __restrict__ nparent,
                                                                     const int32_t* __restrict__ lparent, int64_t F, double* table,
                                                                     int32_t* counter) {
  double o[3];
  root_centre(h, o);
  for (int64_t j = (int64_t)blockIdx.x * WM_THREADS + threadIdx.x; j < F; j += (int64_t)gridDim.x * WM_THREADS) {
    double m[WN_RECORD];
    leaf_moments(leaves, j, o, m);
    int32_t link = lparent[j];
    for (int up = 0; up < 64; ++up) {              // (the tree is at most 63 deep)
      const int64_t p = link >> 1;
      const int slot = link & 1;
      if (p < 0 || p >= F - 1) break;
      __threadfence();                             // what this thread stored below is visible before it is counted
      if ((atomicAdd(&counter[p], 1) & 1) == 0) break;       // the sibling has not arrived: it will carry the sum up
      __threadfence();
      const int32_t sib = nodes[p].child[slot ^ 1];
      double s[WN_RECORD];
      if (sib < 0) {
        const int64_t js = ~sib;
        if (js >= F) break;                        // (a buffer that is not this tree's)
        leaf_moments(leaves, js, o, s);
      } else {
        if (sib >= F - 1) break;
#pragma unroll
        for (int k = 0; k < WN_RECORD; ++k) s[k] = __hip_atomic_load(table + WN_RECORD * (int64_t)sib + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < WN_RECORD; ++k) m[k] = slot ? s[k] + m[k] : m[k] + s[k];      // child 0 + child 1, whoever arrived first
#pragma unroll
      for (int k = 0; k < WN_RECORD; ++k) __hip_atomic_store(table + WN_RECORD * p + k, m[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p == 0) break;                           // the root
      link = nparent[p];
    }
  }
}

__global__ __launch_bounds__(WM_THREADS) void winding_finish_kernel(const Header* __restrict__ h, const Node* __restrict__ nodes, int64_t F,
                                                                    double* __restrict__ table) {
  double o[3];
  root_centre(h, o);
  for (int64_t i = (int64_t)blockIdx.x * WM_THREADS + threadIdx.x; i < F - 1; i += (int64_t)gridDim.x * WM_THREADS) {
    const float4* p = (const float4*)(nodes + i);
    const float4 a = p[0], c = p[1], e = p[2];
    const float lo[3] = {min_f(a.x, c.z), min_f(a.y, c.w), min_f(a.z, e.x)};
    const float hi[3] = {max_f(a.w, e.y), max_f(c.x, e.z), max_f(c.y, e.w)};
    double m[WN_RECORD], t[WN_RECORD];
#pragma unroll
    for (int k = 0; k < WN_RECORD; ++k) m[k] = table[WN_RECORD * i + k];
    i2sdf::wn_finish(m, o[0], o[1], o[2], lo, hi, t);
#pragma unroll
    for (int k = 0; k < WN_RECORD; ++k) table[WN_RECORD * i + k] = t[k];
  }
}

// ---------------------------------------------------------------------------------------------- the tree route
__global__ __launch_bounds__(WT_THREADS) void winding_bvh_kernel(const Header* __restrict__ h, const Node* __restrict__ nodes,
                                                                 const Leaf* __restrict__ leaves, const double* __restrict__ table, int64_t F,
                                                                 const float* __restrict__ points, int64_t n, double beta2,
                                                                 double* __restrict__ w_out, int32_t* status) {
  __shared__ int32_t stack[WT_STACK * WT_THREADS];
  const int64_t i = (int64_t)blockIdx.x * WT_THREADS + threadIdx.x;
  if (i == 0 && (h->flags & I2SDF_RAYCAST_BAD_FACE)) atomicOr(status, I2SDF_WINDING_BAD_FACE);
  if (i >= n) return;                              // (no barrier below)
  const Query q = load_query(points, i);
  double sum = 0.0;
  if (!q.ok) atomicOr(status, I2SDF_WINDING_BAD_POINT);
  if (q.ok && F > 0) {
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
          if (__float_as_int(e.y) >= 0) sum = sum + i2sdf::tri_solid_angle(q.p0, q.p1, q.p2, a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w, e.x);
        }
      } else if (cur < F - 1) {
        const double2* r = (const double2*)(table + WN_RECORD * (int64_t)cur);
        double t[WN_RECORD];
#pragma unroll
        for (int k = 0; k < WN_RECORD / 2; ++k) {
          const double2 v = r[k];
          t[2 * k] = v.x; t[2 * k + 1] = v.y;
        }
        double omega;
        if (i2sdf::wn_far_field(q.p0, q.p1, q.p2, t, beta2, omega)) {
          sum = sum + omega;
        } else {
          const float4 g = ((const float4*)(nodes + cur))[3];
          if (sp < WT_STACK) { my[sp * WT_THREADS] = __float_as_int(g.y); ++sp; }
          cur = __float_as_int(g.x);
          pop = false;
        }
      }
      if (pop) {
        if (sp == 0) break;
        --sp;
        cur = my[sp * WT_THREADS];
      }
    }
  }
  store_winding(w_out, i, q, sum);
}

// ---------------------------------------------------------------------------------------------- the brute route
__global__ __launch_bounds__(WM_THREADS) void winding_faces_check_kernel(const float* __restrict__ verts, int64_t V,
                                                                         const int32_t* __restrict__ faces, int64_t F, int32_t* status) {
  int bad = 0;
  for (int64_t f = (int64_t)blockIdx.x * WM_THREADS + threadIdx.x; f < F; f += (int64_t)gridDim.x * WM_THREADS) {
    float v[9];
    if (!load_face(verts, V, faces, f, v)) bad = 1;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, I2SDF_WINDING_BAD_FACE);
}

__global__ __launch_bounds__(WB_THREADS) void winding_brute_kernel(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                                                   int64_t F, const float* __restrict__ points, int64_t n,
                                                                   double* __restrict__ w_out, int32_t* status) {
  __shared__ float tile[WB_THREADS][10];           // nine coordinates and the valid flag of 256 faces
  const int64_t i = (int64_t)blockIdx.x * WB_THREADS + threadIdx.x;
  Query q;
  q.ok = false;
  q.p0 = q.p1 = q.p2 = 0.0;
  if (i < n) {
    q = load_query(points, i);
    if (!q.ok) atomicOr(status, I2SDF_WINDING_BAD_POINT);
  }
  double sum = 0.0;
  for (int64_t f0 = 0; f0 < F; f0 += WB_THREADS) {           // (every thread of the workgroup takes every turn: barriers inside)
    const int64_t f = f0 + threadIdx.x;
    float v[9];
    bool ok = false;
    if (f < F) ok = load_face(verts, V, faces, f, v);
#pragma unroll
    for (int k = 0; k < 9; ++k) tile[threadIdx.x][k] = ok ? v[k] : 0.0f;
    tile[threadIdx.x][9] = ok ? 1.0f : 0.0f;
    __syncthreads();
    const int m = (int)(F - f0 < WB_THREADS ? F - f0 : WB_THREADS);
    if (q.ok) {
      for (int k = 0; k < m; ++k) {
        const float* t = tile[k];
        if (t[9] != 0.0f) sum = sum + i2sdf::tri_solid_angle(q.p0, q.p1, q.p2, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]);
      }
    }
    __syncthreads();
  }
  if (i < n) store_winding(w_out, i, q, sum);
}

inline unsigned face_blocks(int64_t F) { return blocks(F, WM_THREADS, WM_MAX_BLOCKS); }
inline bool query_ok(const float* points, int64_t n, const double* w_out, const int32_t* status) {
  if (n < 0 || n > INT32_MAX || !aligned(status, 4)) return false;
  return n == 0 || (aligned(points, 4) && aligned(w_out, 8));
}

}  // namespace

extern "C" int64_t i2sdf_winding_moments_bytes(int64_t F) {
  if (!size_ok(F)) return 0;
  return moments_bytes(F);
}

extern "C" int i2sdf_winding_moments(const void* bvh, int64_t F, void* moments, void* stream) {
  if (!size_ok(F) || !aligned(bvh, 16) || !aligned(moments, 16)) return I2SDF_EINVAL;
  if (F < 2) return I2SDF_OK;                      // no internal node: the table is empty
  hipStream_t st = (hipStream_t)stream;
  const Layout w = layout(F);
  const char* base = (const char*)bvh;
  const Header* h = (const Header*)base;
  const Node* nodes = (const Node*)(base + w.nodes);
  const Leaf* leaves = (const Leaf*)(base + w.leaves);
  double* table = (double*)moments;
  int32_t* counter = (int32_t*)((char*)moments + table_bytes(F));
  // (the whole buffer: a node whose subtree a malformed tree never reaches still holds a record that is descended, r = +inf)
  if (int rc = i2sdf_hip_check(hipMemsetAsync(moments, 0, (size_t)moments_bytes(F), st), "winding moments")) return rc;
  winding_moments_kernel<<<face_blocks(F), WM_THREADS, 0, st>>>(h, nodes, leaves, (const int32_t*)(base + w.nparent),
                                                                (const int32_t*)(base + w.lparent), F, table, counter);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "winding_moments_kernel")) return rc;
  winding_finish_kernel<<<face_blocks(F - 1), WM_THREADS, 0, st>>>(h, nodes, F, table);
  return i2sdf_hip_check(hipGetLastError(), "winding_finish_kernel");
}

extern "C" int i2sdf_winding_bvh(const void* bvh, const void* moments, int64_t F, const float* points, int64_t n, float beta, double* w_out,
                                 int32_t* status, void* stream) {
  if (!size_ok(F) || !aligned(bvh, 16) || !aligned(moments, 16) || !(beta >= 0.0f) || !query_ok(points, n, w_out, status)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "winding status")) return rc;
  const Layout w = layout(F);
  const char* base = (const char*)bvh;
  // (n = 0 still launches one workgroup: the face bit of the build reaches *status)
  winding_bvh_kernel<<<blocks(n, WT_THREADS, INT32_MAX), WT_THREADS, 0, st>>>((const Header*)base, (const Node*)(base + w.nodes),
                                                                             (const Leaf*)(base + w.leaves), (const double*)moments, F, points,
                                                                             n, (double)beta * (double)beta, w_out, status);
  return i2sdf_hip_check(hipGetLastError(), "winding_bvh_kernel");
}

extern "C" int i2sdf_winding_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points, int64_t n,
                                   double* w_out, int32_t* status, void* stream) {
  if (!mesh_ok(verts, V, faces, F) || !query_ok(points, n, w_out, status)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(status, 0, 4, st), "winding status")) return rc;
  if (F > 0) {
    winding_faces_check_kernel<<<face_blocks(F), WM_THREADS, 0, st>>>(verts, V, faces, F, status);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "winding_faces_check_kernel")) return rc;
  }
  if (n == 0) return I2SDF_OK;
  winding_brute_kernel<<<blocks(n, WB_THREADS), WB_THREADS, 0, st>>>(verts, V, faces, F, points, n, w_out, status);
  return i2sdf_hip_check(hipGetLastError(), "winding_brute_kernel");
}
