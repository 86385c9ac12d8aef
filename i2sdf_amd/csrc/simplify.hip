// Mesh simplification and cleaning on the device (include/i2sdf.h, "Mesh simplification"): vertex clustering with quadric placement
// (Lindstrom 2000; DeCoro and Tatarchuk 2007), the merging of bit-equal vertices, degenerate / zero-area / duplicate face removal, and
// the edge statistics of the topology report.  Its own unit, so that no other object changes.
//
//   cells       the grid is voxel_down_sample's (i2sdf_points_bounds / _voxel_keys / _voxel_heads, pointops.hip): the caller sorts the
//               vertex keys (stable) and scans the run heads; sm_vertex_cells turns that into a cell id per vertex and the start of every
//               cell's run of vertices.
//   corners     sm_corner_keys: the cell of every face corner (3 F keys) -> sorted by the caller (stable: a run stays in ascending
//               corner, hence face, order) -> sm_corner_runs: where every cell's run of corners begins and ends.
//   reduce      sm_cells, the hot kernel: ONE WAVE PER CELL.  Lane l adds the quadrics of corners l, l + 64, ... of the run, in that
//               order, into nine fp64 partials that start at 0; the 64 lanes are combined by blockops.h's xor butterfly (32, 16, ..., 1);
//               lanes 0..5 meanwhile add the cell's vertex positions and normals one component each in ascending vertex index; lane 0
//               solves (quadric.h) and writes.  No floating-point atomics, no LDS, no scratch.
//   faces       sm_face_keys: corners replaced through a vertex map, the dropped faces marked, the rotated-triple key of the others ->
//               two stable sorts by the caller -> sm_run_heads: the first of every run of equal keys is kept.
//   positions   sm_position_keys: the bits of a vertex (-0.0 as +0.0) as a key pair, for the merging of bit-equal vertices.
//   topology    sm_edge_keys: undirected edge key with the direction in bit 0 -> sorted by the caller -> sm_edge_runs counts the runs by
//               length and direction with integer atomics (order-free).
// Compaction is meshops.hip's (i2sdf_mesh_compact_mark / _gather).  Face indices are validated wherever they are used: a face with
// an index outside [0, n_verts) is never dereferenced; it sets the caller's status word instead.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "quadric.h"

// every product and sum rounded on its own, like the numpy restatement of the tests (no fused multiply-adds)
#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;
using i2sdf::QD_VALUES;

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_MAX_BLOCKS = 4096;                // the wave-per-cell kernel strides beyond that
constexpr int VOXEL_BITS = 21;                     // pointops.hip's key: ix << 42 | iy << 21 | iz
constexpr int64_t DROPPED = INT64_MAX;             // both keys of a face that is not kept

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ float f_dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ faces, int64_t f, int32_t n_verts, int v[3]) {
  v[0] = faces[3 * f]; v[1] = faces[3 * f + 1]; v[2] = faces[3 * f + 2];
  return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] < n_verts && v[1] < n_verts && v[2] < n_verts;
}

// ---------------------------------------------------------------------------------------------- cells
__global__ __launch_bounds__(SM_THREADS) void sm_vertex_cells(const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                                                              const int32_t* __restrict__ head_scan, int64_t V, int64_t M,
                                                              int32_t* __restrict__ vcell, int32_t* __restrict__ cell_start) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i == 0) cell_start[M] = (int32_t)V;
  if (i >= V) return;
  int64_t m = (int64_t)head_scan[i] - 1;           // inclusive scan: cell + 1
  if (m < 0 || m >= M) m = -1;
  const int64_t src = perm[i];
  if (src >= 0 && src < V) vcell[src] = (int32_t)m;
  if (m >= 0 && (i == 0 || skeys[i - 1] != skeys[i])) cell_start[m] = (int32_t)i;
}

__global__ __launch_bounds__(SM_THREADS) void sm_corner_keys(const int32_t* __restrict__ faces, int64_t F, int32_t n_verts,
                                                             const int32_t* __restrict__ vcell, int32_t M, int32_t* __restrict__ ckeys,
                                                             int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (f >= F) return;
  int v[3];
  const bool ok = face_ok(faces, f, n_verts, v);
  if (!ok) atomicOr(status, I2SDF_SIMPLIFY_BAD_FACE);
  for (int c = 0; c < 3; ++c) {
    int32_t k = ok ? vcell[v[c]] : M;
    if (k < 0 || k > M) k = M;                     // (a cell id the caller's tables do not hold: the corner joins no run)
    ckeys[3 * f + c] = k;
  }
}

__global__ __launch_bounds__(SM_THREADS) void sm_corner_runs(const int32_t* __restrict__ sck, int64_t n, int32_t M, int32_t* __restrict__ crun) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t k = sck[i];
  if (k < 0 || k >= M) return;
  if (i == 0 || sck[i - 1] != k) crun[2 * (int64_t)k] = (int32_t)i;
  if (i == n - 1 || sck[i + 1] != k) crun[2 * (int64_t)k + 1] = (int32_t)(i + 1);
}

// ---------------------------------------------------------------------------------------------- reduce and solve
struct CellArgs {
  const float* verts;
  const float* normals;          // NULL: none
  const int32_t* faces;
  const uint32_t* bounds;        // i2sdf_points_bounds
  const int64_t* skeys;          // sorted vertex keys
  const int64_t* vperm;          // the vertex of every sorted position
  const int32_t* cell_start;     // M + 1
  const int64_t* cperm;          // the corner of every sorted corner position
  const int32_t* crun;           // 2 M: begin, end of the cell's corners in cperm
  float* out_verts;
  float* out_normals;
  uint8_t* fallback;
  double h, reg;
  int64_t V, F, M;
  int32_t average;
};

__global__ __launch_bounds__(SM_THREADS) void sm_cells(const CellArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * SM_WAVES;
  const double lo[3] = {(double)f_dec(a.bounds[0]) - 0.5 * a.h, (double)f_dec(a.bounds[1]) - 0.5 * a.h,
                        (double)f_dec(a.bounds[2]) - 0.5 * a.h};
  const int64_t mask = ((int64_t)1 << VOXEL_BITS) - 1;
  for (int64_t m = (int64_t)blockIdx.x * SM_WAVES + (threadIdx.x >> 6); m < a.M; m += n_waves) {
    int64_t vs = a.cell_start[m], ve = a.cell_start[m + 1];
    if (vs < 0) vs = 0;
    if (ve > a.V) ve = a.V;
    const int64_t key = vs < ve ? a.skeys[vs] : 0;
    const double cc[3] = {i2sdf::quadric_cell_centre(lo[0], (key >> (2 * VOXEL_BITS)) & mask, a.h),
                          i2sdf::quadric_cell_centre(lo[1], (key >> VOXEL_BITS) & mask, a.h),
                          i2sdf::quadric_cell_centre(lo[2], key & mask, a.h)};
    // the corner quadrics: lane l takes corners l, l + 64, ... of the run
    double q[QD_VALUES];
#pragma unroll
    for (int k = 0; k < QD_VALUES; ++k) q[k] = 0.0;
    if (!a.average) {
      int64_t cs = a.crun[2 * m], ce = a.crun[2 * m + 1];
      if (cs < 0) cs = 0;
      if (ce > 3 * a.F) ce = 3 * a.F;
      for (int64_t j = cs + lane; j < ce; j += 64) {
        const int64_t corner = a.cperm[j];
        if (corner < 0 || corner >= 3 * a.F) continue;
        int v[3];
        if (!face_ok(a.faces, corner / 3, (int32_t)a.V, v)) continue;
        double p[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int d = 0; d < 3; ++d) p[c][d] = (double)a.verts[3 * (int64_t)v[c] + d];
        double t[QD_VALUES];
        i2sdf::quadric_face(p[0], p[1], p[2], cc, t);
#pragma unroll
        for (int k = 0; k < QD_VALUES; ++k) q[k] += t[k];
      }
#pragma unroll
      for (int k = 0; k < QD_VALUES; ++k) q[k] = wave_sum(q[k]);
    }
    // the vertex sums: lanes 0..2 a coordinate each, lanes 3..5 a normal component each, ascending vertex index
    double s = 0.0;
    if (lane < 3 || (lane < 6 && a.normals)) {
      const float* src = lane < 3 ? a.verts + lane : a.normals + (lane - 3);
      for (int64_t j = vs; j < ve; ++j) {
        const int64_t v = a.vperm[j];
        if (v < 0 || v >= a.V) continue;
        s += (double)src[3 * v];
      }
    }
    const double sum[3] = {__shfl(s, 0, 64), __shfl(s, 1, 64), __shfl(s, 2, 64)};
    const double nsum[3] = {__shfl(s, 3, 64), __shfl(s, 4, 64), __shfl(s, 5, 64)};
    if (lane != 0 || vs >= ve) continue;
    const double cnt = (double)(ve - vs);
    const double mean[3] = {sum[0] / cnt, sum[1] / cnt, sum[2] / cnt};
    if (a.average) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.out_verts[3 * m + c] = (float)mean[c];
      a.fallback[m] = 0;
    } else {
      const double rel[3] = {mean[0] - cc[0], mean[1] - cc[1], mean[2] - cc[2]};
      double x[3];
      a.fallback[m] = i2sdf::quadric_solve(q, a.reg, rel, 0.5 * a.h, x) ? 1 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) a.out_verts[3 * m + c] = (float)(cc[c] + x[c]);
    }
    if (a.out_normals) {
      float nn[3];
      i2sdf::quadric_normal(nsum, nn);
#pragma unroll
      for (int c = 0; c < 3; ++c) a.out_normals[3 * m + c] = nn[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------- faces
__device__ __forceinline__ bool triple_less(int32_t a0, int32_t a1, int32_t a2, int32_t b0, int32_t b1, int32_t b2) {
  return a0 < b0 || (a0 == b0 && (a1 < b1 || (a1 == b1 && a2 < b2)));
}

__global__ __launch_bounds__(SM_THREADS) void sm_face_keys(const float* __restrict__ verts, int32_t n_verts, const int32_t* __restrict__ faces,
                                                           int64_t F, const int32_t* __restrict__ vmap, int32_t n_map, int32_t flags,
                                                           int32_t* __restrict__ out_faces, int64_t* __restrict__ key_hi,
                                                           int64_t* __restrict__ key_lo, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (f >= F) return;
  int v[3];
  int32_t t[3] = {-1, -1, -1};
  bool keep = face_ok(faces, f, n_verts, v);
  if (keep) {
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = vmap ? vmap[v[c]] : v[c];
    keep = t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[0] < n_map && t[1] < n_map && t[2] < n_map;
  }
  if (!keep) {
    atomicOr(status, I2SDF_SIMPLIFY_BAD_FACE);
    t[0] = t[1] = t[2] = -1;
  }
  if (keep && (flags & I2SDF_SIMPLIFY_DROP_REPEATED)) keep = t[0] != t[1] && t[1] != t[2] && t[2] != t[0];
  if (keep && (flags & I2SDF_SIMPLIFY_DROP_ZERO_AREA)) {
    double p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int d = 0; d < 3; ++d) p[c][d] = (double)verts[3 * (int64_t)v[c] + d];
    const double e0 = p[1][0] - p[0][0], e1 = p[1][1] - p[0][1], e2 = p[1][2] - p[0][2];
    const double g0 = p[2][0] - p[0][0], g1 = p[2][1] - p[0][1], g2 = p[2][2] - p[0][2];
    const double n0 = e1 * g2 - e2 * g1, n1 = e2 * g0 - e0 * g2, n2 = e0 * g1 - e1 * g0;      // tri_closest.h's tri_cross
    keep = !(n0 == 0.0 && n1 == 0.0 && n2 == 0.0);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out_faces[3 * f + c] = t[c];
  int64_t hi = DROPPED, lo = DROPPED;
  if (keep) {
    // the lexicographically smallest of the three rotations: one key per cyclic sequence, orientation kept
    int32_t b0 = t[0], b1 = t[1], b2 = t[2];
    if (triple_less(t[1], t[2], t[0], b0, b1, b2)) { b0 = t[1]; b1 = t[2]; b2 = t[0]; }
    if (triple_less(t[2], t[0], t[1], b0, b1, b2)) { b0 = t[2]; b1 = t[0]; b2 = t[1]; }
    hi = b0;
    lo = ((int64_t)b1 << 32) | (int64_t)b2;
  }
  key_hi[f] = hi;
  key_lo[f] = lo;
}

// keep[perm[i]]: is sorted entry i the first of its run of equal key pairs (and not a dropped one)?  first[i]: i at a head, else 0
__global__ __launch_bounds__(SM_THREADS) void sm_run_heads(const int64_t* __restrict__ shi, const int64_t* __restrict__ slo,
                                                           const int64_t* __restrict__ perm, int64_t n, uint8_t* __restrict__ keep,
                                                           int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool head = i == 0 || shi[i] != shi[i - 1] || slo[i] != slo[i - 1];
  if (first) first[i] = head ? (int32_t)i : 0;
  const int64_t src = perm[i];
  if (keep && src >= 0 && src < n) keep[src] = head && !(shi[i] == DROPPED && slo[i] == DROPPED);
}

__global__ __launch_bounds__(SM_THREADS) void sm_position_keys(const float* __restrict__ verts, int64_t V, int64_t* __restrict__ key_hi,
                                                               int64_t* __restrict__ key_lo) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= V) return;
  uint32_t b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    b[c] = __float_as_uint(verts[3 * i + c]);
    if (b[c] == 0x80000000u) b[c] = 0u;            // -0.0 is +0.0
  }
  key_hi[i] = (int64_t)b[0];
  key_lo[i] = (int64_t)(((uint64_t)b[1] << 32) | (uint64_t)b[2]);      // (may be negative: only equality and a total order are asked of it)
}

// ---------------------------------------------------------------------------------------------- topology
__global__ __launch_bounds__(SM_THREADS) void sm_edge_keys(const int32_t* __restrict__ faces, int64_t F, int32_t n_verts,
                                                           int64_t* __restrict__ keys, int32_t* vflag, unsigned long long* __restrict__ counts,
                                                           int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  int64_t n_rep = 0, n_ok = 0;
  if (f < F) {
    int v[3];
    const bool ok = face_ok(faces, f, n_verts, v);
    if (!ok) atomicOr(status, I2SDF_SIMPLIFY_BAD_FACE);
    const bool rep = ok && (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]);
    n_rep = rep;
    n_ok = ok && !rep;
    for (int c = 0; c < 3; ++c) {
      int64_t k = DROPPED;
      if (ok && !rep) {
        const int64_t a = v[c], b = v[c == 2 ? 0 : c + 1];
        k = a < b ? (a << 32) | (b << 1) : (b << 32) | (a << 1) | 1;      // bit 0: traversed from the larger index
        vflag[v[c]] = 1;                           // (every writer stores the same value)
      }
      keys[3 * f + c] = k;
    }
  }
  n_rep = wave_sum(n_rep);
  n_ok = wave_sum(n_ok);
  if ((threadIdx.x & 63) == 0) {
    if (n_rep) atomicAdd(counts + I2SDF_TOPO_REPEATED_FACES, (unsigned long long)n_rep);
    if (n_ok) atomicAdd(counts + I2SDF_TOPO_FACES, (unsigned long long)n_ok);
  }
}

__global__ __launch_bounds__(SM_THREADS) void sm_count_flags(const int32_t* __restrict__ vflag, int64_t V, unsigned long long* __restrict__ counts) {
  int64_t n = 0;
  for (int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * SM_THREADS) n += vflag[i] != 0;
  n = wave_sum(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(counts + I2SDF_TOPO_VERTICES, (unsigned long long)n);
}

// one thread per sorted half-edge; the head of a run of equal undirected edges classifies it (runs are as long as an edge has faces)
__global__ __launch_bounds__(SM_THREADS) void sm_edge_runs(const int64_t* __restrict__ sk, int64_t n, unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x;
  int64_t c[5] = {0, 0, 0, 0, 0};                  // edges, boundary, manifold, non-manifold, misoriented
  if (i < n && sk[i] != DROPPED && (i == 0 || (sk[i - 1] >> 1) != (sk[i] >> 1))) {
    const int64_t e = sk[i] >> 1;
    int64_t j = i + 1;
    while (j < n && (sk[j] >> 1) == e) ++j;
    const int64_t len = j - i;
    c[0] = 1;
    c[1] = len == 1;
    c[2] = len == 2;
    c[3] = len >= 3;
    c[4] = len == 2 && ((sk[i] ^ sk[i + 1]) & 1) == 0;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    c[k] = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(counts + k, (unsigned long long)c[k]);
  }
}

__global__ void sm_euler(int64_t* counts) {
  if (threadIdx.x || blockIdx.x) return;
  counts[I2SDF_TOPO_EULER] = counts[I2SDF_TOPO_VERTICES] - counts[I2SDF_TOPO_EDGES] + counts[I2SDF_TOPO_FACES];
}

}  // namespace

extern "C" int i2sdf_simplify_vertex_cells(const int64_t* sorted_keys, const int64_t* perm, const int32_t* head_scan, int64_t V, int64_t n_cells,
                                           int32_t* vertex_cell, int32_t* cell_start, void* stream) {
  if (!fits(V) || !fits(n_cells) || n_cells > V || !cell_start || !aligned(cell_start, 4)) return I2SDF_EINVAL;
  if (V > 0 && (!sorted_keys || !perm || !head_scan || !vertex_cell || !aligned(sorted_keys, 8) || !aligned(perm, 8) || !aligned(head_scan, 4) ||
                !aligned(vertex_cell, 4)))
    return I2SDF_EINVAL;
  sm_vertex_cells<<<blocks(V, SM_THREADS, INT_MAX), SM_THREADS, 0, (hipStream_t)stream>>>(sorted_keys, perm, head_scan, V, n_cells, vertex_cell,
                                                                                      cell_start);
  return i2sdf_hip_check(hipGetLastError(), "sm_vertex_cells");
}

extern "C" int i2sdf_simplify_corner_keys(const int32_t* faces, int64_t F, int64_t V, const int32_t* vertex_cell, int64_t n_cells,
                                          int32_t* corner_keys, int32_t* status, void* stream) {
  if (!fits(F) || !fits(V) || !fits(n_cells) || F > INT32_MAX / 3 || !status || !aligned(status, 4)) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  if (!faces || !corner_keys || (V > 0 && !vertex_cell) || !aligned(faces, 4) || !aligned(corner_keys, 4) || !aligned(vertex_cell, 4))
    return I2SDF_EINVAL;
  sm_corner_keys<<<blocks(F, SM_THREADS), SM_THREADS, 0, (hipStream_t)stream>>>(faces, F, (int32_t)V, vertex_cell, (int32_t)n_cells, corner_keys,
                                                                                status);
  return i2sdf_hip_check(hipGetLastError(), "sm_corner_keys");
}

extern "C" int i2sdf_simplify_corner_runs(const int32_t* sorted_corner_keys, int64_t F, int64_t n_cells, int32_t* corner_runs, void* stream) {
  if (!fits(F) || !fits(n_cells) || F > INT32_MAX / 3) return I2SDF_EINVAL;
  if (n_cells == 0) return I2SDF_OK;
  if (!corner_runs || !aligned(corner_runs, 4) || (F > 0 && (!sorted_corner_keys || !aligned(sorted_corner_keys, 4)))) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(corner_runs, 0, 8 * n_cells, st), "corner runs")) return rc;
  if (F == 0) return I2SDF_OK;
  sm_corner_runs<<<blocks(3 * F, SM_THREADS), SM_THREADS, 0, st>>>(sorted_corner_keys, 3 * F, (int32_t)n_cells, corner_runs);
  return i2sdf_hip_check(hipGetLastError(), "sm_corner_runs");
}

extern "C" int i2sdf_simplify_cells(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, const int32_t* bounds,
                                    double voxel_size, double reg, int32_t contraction, const int64_t* sorted_keys, const int64_t* perm,
                                    const int32_t* cell_start, const int64_t* corner_perm, const int32_t* corner_runs, int64_t n_cells,
                                    float* out_verts, float* out_normals, uint8_t* fallback, void* stream) {
  if (!fits(V) || !fits(F) || !fits(n_cells) || F > INT32_MAX / 3 || n_cells > V) return I2SDF_EINVAL;
  if (!(voxel_size > 0.0) || !isfinite(voxel_size) || !(reg > 0.0) || !isfinite(reg)) return I2SDF_EINVAL;
  if (contraction != I2SDF_SIMPLIFY_QUADRIC && contraction != I2SDF_SIMPLIFY_AVERAGE) return I2SDF_EINVAL;
  if (n_cells == 0) return I2SDF_OK;
  if (!verts || !bounds || !sorted_keys || !perm || !cell_start || !out_verts || !fallback || (normals && !out_normals)) return I2SDF_EINVAL;
  if (!aligned(verts, 4) || !aligned(normals, 4) || !aligned(bounds, 4) || !aligned(sorted_keys, 8) || !aligned(perm, 8) || !aligned(cell_start, 4) ||
      !aligned(out_verts, 4) || !aligned(out_normals, 4))
    return I2SDF_EINVAL;
  const bool quadric = contraction == I2SDF_SIMPLIFY_QUADRIC;
  if (quadric && (!corner_runs || !aligned(corner_runs, 4))) return I2SDF_EINVAL;
  if (quadric && F > 0 && (!faces || !corner_perm || !aligned(faces, 4) || !aligned(corner_perm, 8))) return I2SDF_EINVAL;
  CellArgs a;
  a.verts = verts; a.normals = normals; a.faces = faces; a.bounds = (const uint32_t*)bounds; a.skeys = sorted_keys; a.vperm = perm;
  a.cell_start = cell_start; a.cperm = corner_perm; a.crun = corner_runs; a.out_verts = out_verts; a.out_normals = normals ? out_normals : nullptr;
  a.fallback = fallback; a.h = voxel_size; a.reg = reg; a.V = V; a.F = F; a.M = n_cells; a.average = quadric ? 0 : 1;
  sm_cells<<<blocks(n_cells, SM_WAVES, SM_MAX_BLOCKS), SM_THREADS, 0, (hipStream_t)stream>>>(a);
  return i2sdf_hip_check(hipGetLastError(), "sm_cells");
}

extern "C" int i2sdf_simplify_face_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int32_t* vertex_map, int64_t n_map,
                                        int32_t flags, int32_t* out_faces, int64_t* key_hi, int64_t* key_lo, int32_t* status, void* stream) {
  if (!fits(V) || !fits(F) || !fits(n_map) || !status || !aligned(status, 4)) return I2SDF_EINVAL;
  if (flags & ~(I2SDF_SIMPLIFY_DROP_REPEATED | I2SDF_SIMPLIFY_DROP_ZERO_AREA)) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  if (!faces || !out_faces || !key_hi || !key_lo || !aligned(faces, 4) || !aligned(out_faces, 4) || !aligned(key_hi, 8) || !aligned(key_lo, 8) ||
      !aligned(vertex_map, 4))
    return I2SDF_EINVAL;
  if ((flags & I2SDF_SIMPLIFY_DROP_ZERO_AREA) && V > 0 && (!verts || !aligned(verts, 4))) return I2SDF_EINVAL;
  sm_face_keys<<<blocks(F, SM_THREADS), SM_THREADS, 0, (hipStream_t)stream>>>(verts, (int32_t)V, faces, F, vertex_map, (int32_t)n_map, flags,
                                                                              out_faces, key_hi, key_lo, status);
  return i2sdf_hip_check(hipGetLastError(), "sm_face_keys");
}

extern "C" int i2sdf_simplify_run_heads(const int64_t* sorted_hi, const int64_t* sorted_lo, const int64_t* perm, int64_t n, uint8_t* keep,
                                        int32_t* first, void* stream) {
  if (!fits(n)) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;                     // (an empty array has no address: nothing to check, nothing to do)
  if (!keep && !first) return I2SDF_EINVAL;
  if (!sorted_hi || !sorted_lo || !perm || !aligned(sorted_hi, 8) || !aligned(sorted_lo, 8) || !aligned(perm, 8) || !aligned(first, 4))
    return I2SDF_EINVAL;
  sm_run_heads<<<blocks(n, SM_THREADS), SM_THREADS, 0, (hipStream_t)stream>>>(sorted_hi, sorted_lo, perm, n, keep, first);
  return i2sdf_hip_check(hipGetLastError(), "sm_run_heads");
}

extern "C" int i2sdf_simplify_position_keys(const float* verts, int64_t V, int64_t* key_hi, int64_t* key_lo, void* stream) {
  if (!fits(V)) return I2SDF_EINVAL;
  if (V == 0) return I2SDF_OK;
  if (!verts || !key_hi || !key_lo || !aligned(verts, 4) || !aligned(key_hi, 8) || !aligned(key_lo, 8)) return I2SDF_EINVAL;
  sm_position_keys<<<blocks(V, SM_THREADS), SM_THREADS, 0, (hipStream_t)stream>>>(verts, V, key_hi, key_lo);
  return i2sdf_hip_check(hipGetLastError(), "sm_position_keys");
}

extern "C" int i2sdf_mesh_edge_stats_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, int32_t* vflag, int64_t* counts,
                                          int32_t* status, void* stream) {
  if (!fits(F) || !fits(V) || F > INT32_MAX / 3 || !counts || !status || !aligned(counts, 8) || !aligned(status, 4)) return I2SDF_EINVAL;
  if (F > 0 && (!faces || !keys || !aligned(faces, 4) || !aligned(keys, 8))) return I2SDF_EINVAL;
  if (V > 0 && (!vflag || !aligned(vflag, 4))) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(counts, 0, 8 * I2SDF_TOPO_COUNTS, st), "edge stats")) return rc;
  if (V > 0)
    if (int rc = i2sdf_hip_check(hipMemsetAsync(vflag, 0, 4 * V, st), "edge stats")) return rc;
  if (F == 0) return I2SDF_OK;
  sm_edge_keys<<<blocks(F, SM_THREADS), SM_THREADS, 0, st>>>(faces, F, (int32_t)V, keys, vflag, (unsigned long long*)counts, status);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "sm_edge_keys")) return rc;
  if (V == 0) return I2SDF_OK;
  sm_count_flags<<<blocks(V, SM_THREADS, 1024), SM_THREADS, 0, st>>>(vflag, V, (unsigned long long*)counts);
  return i2sdf_hip_check(hipGetLastError(), "sm_count_flags");
}

extern "C" int i2sdf_mesh_edge_stats(const int64_t* sorted_keys, int64_t F, int64_t* counts, void* stream) {
  if (!fits(F) || F > INT32_MAX / 3 || !counts || !aligned(counts, 8)) return I2SDF_EINVAL;
  if (F > 0 && (!sorted_keys || !aligned(sorted_keys, 8))) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F > 0) {
    sm_edge_runs<<<blocks(3 * F, SM_THREADS), SM_THREADS, 0, st>>>(sorted_keys, 3 * F, (unsigned long long*)counts);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "sm_edge_runs")) return rc;
  }
  sm_euler<<<1, 64, 0, st>>>(counts);
  return i2sdf_hip_check(hipGetLastError(), "sm_euler");
}
