// Mesh operations on the device, the middle of the reference's mesh export (utils/plots.py:280-297, model/eval/recon.py:61-71,
// where trimesh runs them on the host): face components, face / component areas, sub-mesh compaction, surface sampling.
//
//   components  edge keys (min(va,vb) << 32 | max(va,vb), one per face side) -> sorted by the caller -> one thread per sorted entry
//               unites the owners of equal neighbours in parent[] (lock-free: a root is hooked under a SMALLER root by an integer
//               compare-and-swap, so every tree's root is its smallest face and the final roots do not depend on the order of the
//               unions) -> flatten: labels[f] = root(f).  A retry follows only a compare-and-swap that lost to another thread's
//               progress; nobody waits for anybody.
//   areas       0.5 |(v1 - v0) x (v2 - v0)| in fp32; running sums in fp64 by a reduce-then-scan in a fixed order (no atomics).
//   largest     component areas = differences of the fp64 running sum over the faces sorted by label; the largest by integer
//               atomicMax of the (non-negative) double's bit pattern, ties to the smaller label by atomicMin: order-free results.
//   compaction  mark the vertices of kept faces, (scans by the caller), re-index faces and gather vertices / normals.
//   sampling    one thread per sample: binary search of the fp64 running sum, point from the two barycentric draws.
// Face indices are validated wherever they are used: a face with an index outside [0, n_verts) is never dereferenced; it sets
// the caller's status word instead (i2sdf_mesh_status turns that into I2SDF_EINVAL).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"

// every product and sum rounded on its own, like the numpy restatement of the tests (no fused multiply-adds)
#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;

constexpr int MO_THREADS = 256;

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ faces, int64_t f, int32_t n_verts, int v[3]) {
  v[0] = faces[3 * f]; v[1] = faces[3 * f + 1]; v[2] = faces[3 * f + 2];
  return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] < n_verts && v[1] < n_verts && v[2] < n_verts;
}

// ---------------------------------------------------------------------------------------------- components
__global__ __launch_bounds__(MO_THREADS) void mo_edge_keys(const int32_t* __restrict__ faces, int64_t F, int32_t n_verts,
                                                           int64_t* __restrict__ keys, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f >= F) return;
  int v[3];
  if (!face_ok(faces, f, n_verts, v)) {
    atomicOr(status, 1);
    for (int c = 0; c < 3; ++c) keys[3 * f + c] = -(3 * f + c) - 1;      // unique: a refused face is connected to nothing
    return;
  }
  for (int c = 0; c < 3; ++c) {
    const int64_t a = v[c], b = v[c == 2 ? 0 : c + 1];
    keys[3 * f + c] = a < b ? (a << 32) | b : (b << 32) | a;
  }
}

__global__ __launch_bounds__(MO_THREADS) void mo_init_parent(int32_t* __restrict__ parent, int64_t F) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f < F) parent[f] = (int32_t)f;
}

// root of x, halving the path on the way (a non-root never becomes a root again and only ever points to an ancestor, so a
// racing store of a grandparent is harmless)
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
  int32_t p = __hip_atomic_load(parent + x, RLX_AGENT);
  while (p != x) {
    const int32_t g = __hip_atomic_load(parent + p, RLX_AGENT);
    if (g != p) __hip_atomic_store(parent + x, g, RLX_AGENT);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
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

// sorted entry i and its left neighbour hold the same edge -> their faces are connected (a run of k entries makes k-1 unions)
__global__ __launch_bounds__(MO_THREADS) void mo_unite_runs(const int64_t* __restrict__ keys, const int64_t* __restrict__ perm, int64_t n,
                                                            int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x + 1;
  if (i >= n || keys[i] != keys[i - 1]) return;
  const int64_t pa = perm[i], pb = perm[i - 1];
  if (pa < 0 || pb < 0 || pa >= n || pb >= n) return;          // (not a permutation of the 3F entries: nothing to unite)
  unite(parent, (int32_t)(pa / 3), (int32_t)(pb / 3));
}

__global__ __launch_bounds__(MO_THREADS) void mo_flatten(int32_t* parent, int64_t F) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f >= F) return;
  int32_t x = (int32_t)f, p = __hip_atomic_load(parent + x, RLX_AGENT);
  while (p != x) { x = p; p = __hip_atomic_load(parent + x, RLX_AGENT); }
  if (x != (int32_t)f) __hip_atomic_store(parent + f, x, RLX_AGENT);     // (others may still walk through f: the root is an ancestor)
}

// ---------------------------------------------------------------------------------------------- areas
__global__ __launch_bounds__(MO_THREADS) void mo_face_areas(const float* __restrict__ verts, int32_t n_verts, const int32_t* __restrict__ faces,
                                                            int64_t F, float* __restrict__ area, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f >= F) return;
  int v[3];
  if (!face_ok(faces, f, n_verts, v)) { atomicOr(status, 1); area[f] = 0.0f; return; }
  float e1[3], e2[3];
  for (int c = 0; c < 3; ++c) {
    const float p0 = verts[3 * (int64_t)v[0] + c];
    e1[c] = verts[3 * (int64_t)v[1] + c] - p0;
    e2[c] = verts[3 * (int64_t)v[2] + c] - p0;
  }
  const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  area[f] = 0.5f * sqrtf(cx * cx + cy * cy + cz * cz);
}

// ---------------------------------------------------------------------------------------------- fp64 running sum
struct SrcF32 {                                    // level 0: x[order[i]] (order NULL: x[i]) widened to fp64
  const float* x; const int64_t* order; int64_t n_src;
  __device__ double operator()(int64_t i) const {
    const int64_t j = order ? order[i] : i;
    return j >= 0 && j < n_src ? (double)x[j] : 0.0;
  }
};

// levels of chunk sums above the n items (blockops.h); at least 16 bytes, so that a caller's allocation is never empty
bool scan_layout(int64_t n, ScanLevels& L) {
  if (!fits(n) || !scan_levels((n + SCAN_CHUNK - 1) / SCAN_CHUNK, sizeof(double), 0, L)) return false;
  if (L.bytes < 16) L.bytes = 16;
  return true;
}

// ---------------------------------------------------------------------------------------------- largest component
// i is the last face (in label order) of its component: area = cdf[i] - cdf[start - 1], start = first entry with this label
__device__ __forceinline__ bool segment_area(const int32_t* __restrict__ lab, const double* __restrict__ cdf, int64_t F, int64_t i, double& area) {
  if (i + 1 < F && lab[i + 1] == lab[i]) return false;
  const int32_t l = lab[i];
  int64_t lo = 0, hi = i;                          // first position whose label is >= l
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (lab[mid] < l) lo = mid + 1; else hi = mid;
  }
  area = lo > 0 ? cdf[i] - cdf[lo - 1] : cdf[i];
  if (!(area > 0.0)) area = 0.0;                   // (NaN areas and rounding below zero lose against everything)
  return true;
}

__global__ void mo_best_init(unsigned long long* best) {      // (area bits, label); an empty mesh keeps them
  best[0] = 0;
  best[1] = (unsigned long long)INT64_MAX;
}

__global__ __launch_bounds__(MO_THREADS) void mo_best_area(const int32_t* __restrict__ lab, const double* __restrict__ cdf, int64_t F,
                                                           unsigned long long* best) {
  const int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  double a;
  if (i >= F || !segment_area(lab, cdf, F, i, a)) return;
  atomicMax(best, (unsigned long long)__double_as_longlong(a));          // non-negative doubles order like their bit patterns
}

__global__ __launch_bounds__(MO_THREADS) void mo_best_label(const int32_t* __restrict__ lab, const double* __restrict__ cdf, int64_t F,
                                                            unsigned long long* best) {
  const int64_t i = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  double a;
  if (i >= F || !segment_area(lab, cdf, F, i, a)) return;
  if ((unsigned long long)__double_as_longlong(a) == best[0]) atomicMin(best + 1, (unsigned long long)lab[i]);
}

// ---------------------------------------------------------------------------------------------- compaction
__global__ __launch_bounds__(MO_THREADS) void mo_mark(const int32_t* __restrict__ faces, const uint8_t* __restrict__ mask, int64_t F,
                                                      int32_t n_verts, int32_t* __restrict__ fkeep, int32_t* vflag,
                                                      int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f >= F) return;
  int v[3];
  int keep = mask[f] != 0;
  if (keep && !face_ok(faces, f, n_verts, v)) { atomicOr(status, 1); keep = 0; }
  fkeep[f] = keep;
  if (keep)
    for (int c = 0; c < 3; ++c) vflag[v[c]] = 1;   // (every writer stores the same value)
}

__global__ __launch_bounds__(MO_THREADS) void mo_compact_faces(const int32_t* __restrict__ faces, const int32_t* __restrict__ fkeep,
                                                               const int32_t* __restrict__ fscan, const int32_t* __restrict__ vscan,
                                                               int64_t F, int32_t* __restrict__ out, int64_t cap_f) {
  const int64_t f = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (f >= F || !fkeep[f]) return;
  const int64_t o = (int64_t)fscan[f] - 1;         // inclusive scans: position + 1
  if (o < 0 || o >= cap_f) return;
  for (int c = 0; c < 3; ++c) out[3 * o + c] = vscan[faces[3 * f + c]] - 1;
}

__global__ __launch_bounds__(MO_THREADS) void mo_compact_verts(const float* __restrict__ verts, const float* __restrict__ normals,
                                                               const int32_t* __restrict__ vflag, const int32_t* __restrict__ vscan,
                                                               int64_t V, float* __restrict__ out_v, float* __restrict__ out_n, int64_t cap_v) {
  const int64_t v = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (v >= V || !vflag[v]) return;
  const int64_t o = (int64_t)vscan[v] - 1;
  if (o < 0 || o >= cap_v) return;
  for (int c = 0; c < 3; ++c) {
    out_v[3 * o + c] = verts[3 * v + c];
    if (normals) out_n[3 * o + c] = normals[3 * v + c];
  }
}

// ---------------------------------------------------------------------------------------------- sampling
__global__ __launch_bounds__(MO_THREADS) void mo_sample(const float* __restrict__ verts, int32_t n_verts, const int32_t* __restrict__ faces,
                                                        int64_t F, const double* __restrict__ cdf, const float* __restrict__ u_face,
                                                        const float* __restrict__ u_bary, int64_t count, float* __restrict__ points,
                                                        int32_t* __restrict__ face_index, int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * MO_THREADS + threadIdx.x;
  if (s >= count) return;
  const double pick = (double)u_face[s] * cdf[F - 1];
  int64_t lo = 0, hi = F;                          // np.searchsorted(cdf, pick, side='left'): first i with cdf[i] >= pick
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] < pick) lo = mid + 1; else hi = mid;
  }
  const int64_t f = lo < F ? lo : F - 1;
  face_index[s] = (int32_t)f;
  int v[3];
  if (!face_ok(faces, f, n_verts, v)) {
    atomicOr(status, 1);
    for (int c = 0; c < 3; ++c) points[3 * s + c] = 0.0f;
    return;
  }
  float a = u_bary[2 * s], b = u_bary[2 * s + 1];
  if (a + b > 1.0f) { a = fabsf(a - 1.0f); b = fabsf(b - 1.0f); }
  for (int c = 0; c < 3; ++c) {
    const float p0 = verts[3 * (int64_t)v[0] + c];
    const float e1 = verts[3 * (int64_t)v[1] + c] - p0, e2 = verts[3 * (int64_t)v[2] + c] - p0;
    points[3 * s + c] = p0 + a * e1 + b * e2;
  }
}

}  // namespace

extern "C" int64_t i2sdf_mesh_scan_workspace_bytes(int64_t n) {
  ScanLevels L;
  return scan_layout(n, L) ? L.bytes : 0;
}

extern "C" int i2sdf_mesh_status(const int32_t* status, void* stream) {
  if (!status) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  int32_t h = 0;
  if (int rc = i2sdf_hip_check(hipMemcpyAsync(&h, status, 4, hipMemcpyDeviceToHost, st), "mesh status")) return rc;
  if (int rc = i2sdf_hip_check(hipStreamSynchronize(st), "mesh status")) return rc;
  return h ? I2SDF_EINVAL : I2SDF_OK;
}

extern "C" int i2sdf_mesh_edge_keys(const int32_t* faces, int64_t F, int64_t n_verts, int64_t* keys, int32_t* status, void* stream) {
  if (!fits(F) || !fits(n_verts)) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  if (!faces || !keys || !status) return I2SDF_EINVAL;
  mo_edge_keys<<<blocks(F, MO_THREADS), MO_THREADS, 0, (hipStream_t)stream>>>(faces, F, (int32_t)n_verts, keys, status);
  return i2sdf_hip_check(hipGetLastError(), "mo_edge_keys");
}

extern "C" int i2sdf_mesh_face_components(const int64_t* sorted_keys, const int64_t* perm, int64_t F, int32_t* labels, void* stream) {
  if (!fits(F)) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  if (!sorted_keys || !perm || !labels) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  mo_init_parent<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(labels, F);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_init_parent")) return rc;
  mo_unite_runs<<<blocks(3 * F - 1, MO_THREADS), MO_THREADS, 0, st>>>(sorted_keys, perm, 3 * F, labels);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_unite_runs")) return rc;
  mo_flatten<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(labels, F);
  return i2sdf_hip_check(hipGetLastError(), "mo_flatten");
}

extern "C" int i2sdf_mesh_face_areas(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, float* area, int32_t* status,
                                     void* stream) {
  if (!fits(F) || !fits(n_verts)) return I2SDF_EINVAL;
  if (F == 0) return I2SDF_OK;
  if (!verts || !faces || !area || !status) return I2SDF_EINVAL;
  mo_face_areas<<<blocks(F, MO_THREADS), MO_THREADS, 0, (hipStream_t)stream>>>(verts, (int32_t)n_verts, faces, F, area, status);
  return i2sdf_hip_check(hipGetLastError(), "mo_face_areas");
}

extern "C" int i2sdf_mesh_cumsum_f64(const float* x, int64_t n_x, const int64_t* order, int64_t n, double* cdf, void* workspace, void* stream) {
  ScanLevels L;
  if (!fits(n_x) || !scan_layout(n, L) || (!order && n > n_x)) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  if (!x || !cdf || !workspace) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  double* sums = (double*)((char*)workspace + L.level_off[0]);
  const SrcF32 src{x, order, n_x};
  // chunk sums, their exclusive offsets (up the levels and down again), then the running sum of the items themselves
  scan_reduce_kernel<SrcF32, double><<<(unsigned)L.level_n[0], SCAN_THREADS, 0, st>>>(src, n, sums);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "scan_reduce_kernel")) return rc;
  if (int rc = scan_levels_exclusive<double>(workspace, L, nullptr, st)) return rc;
  scan_chunks_kernel<SrcF32, double, true><<<(unsigned)L.level_n[0], SCAN_THREADS, 0, st>>>(src, n, sums, cdf, nullptr);
  return i2sdf_hip_check(hipGetLastError(), "scan_chunks_kernel");
}

extern "C" int i2sdf_mesh_largest_label(const int32_t* sorted_labels, const double* cdf, int64_t F, int64_t* best, void* stream) {
  if (!fits(F) || !best) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  mo_best_init<<<1, 1, 0, st>>>((unsigned long long*)best);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_best_init")) return rc;
  if (F == 0) return I2SDF_OK;
  if (!sorted_labels || !cdf) return I2SDF_EINVAL;
  mo_best_area<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(sorted_labels, cdf, F, (unsigned long long*)best);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_best_area")) return rc;
  mo_best_label<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(sorted_labels, cdf, F, (unsigned long long*)best);
  return i2sdf_hip_check(hipGetLastError(), "mo_best_label");
}

extern "C" int i2sdf_mesh_compact_mark(const int32_t* faces, const uint8_t* mask, int64_t F, int64_t n_verts, int32_t* fkeep, int32_t* vflag,
                                       int32_t* status, void* stream) {
  if (!fits(F) || !fits(n_verts)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (n_verts > 0) {
    if (!vflag) return I2SDF_EINVAL;
    if (int rc = i2sdf_hip_check(hipMemsetAsync(vflag, 0, 4 * n_verts, st), "compact mark")) return rc;
  }
  if (F == 0) return I2SDF_OK;
  if (!faces || !mask || !fkeep || !status) return I2SDF_EINVAL;
  mo_mark<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(faces, mask, F, (int32_t)n_verts, fkeep, vflag, status);
  return i2sdf_hip_check(hipGetLastError(), "mo_mark");
}

extern "C" int i2sdf_mesh_compact_gather(const float* verts, const float* normals, int64_t n_verts, const int32_t* faces, int64_t F,
                                         const int32_t* fkeep, const int32_t* fscan, const int32_t* vflag, const int32_t* vscan,
                                         float* out_verts, float* out_normals, int32_t* out_faces, int64_t cap_v, int64_t cap_f, void* stream) {
  if (!fits(F) || !fits(n_verts) || cap_v < 0 || cap_f < 0) return I2SDF_EINVAL;
  if (normals && !out_normals && cap_v > 0) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (F > 0 && cap_f > 0) {
    if (!faces || !fkeep || !fscan || !vscan || !out_faces) return I2SDF_EINVAL;
    mo_compact_faces<<<blocks(F, MO_THREADS), MO_THREADS, 0, st>>>(faces, fkeep, fscan, vscan, F, out_faces, cap_f);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_compact_faces")) return rc;
  }
  if (n_verts > 0 && cap_v > 0) {
    if (!verts || !vflag || !vscan || !out_verts) return I2SDF_EINVAL;
    mo_compact_verts<<<blocks(n_verts, MO_THREADS), MO_THREADS, 0, st>>>(verts, normals, vflag, vscan, n_verts, out_verts, out_normals, cap_v);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "mo_compact_verts")) return rc;
  }
  return I2SDF_OK;
}

extern "C" int i2sdf_mesh_sample_surface(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, const double* cdf,
                                         const float* u_face, const float* u_bary, int64_t count, float* points, int32_t* face_index,
                                         int32_t* status, void* stream) {
  if (!fits(F) || !fits(n_verts) || !fits(count)) return I2SDF_EINVAL;
  if (count == 0) return I2SDF_OK;
  if (F == 0) return I2SDF_EINVAL;                 // nothing to draw from
  if (!verts || !faces || !cdf || !u_face || !u_bary || !points || !face_index || !status) return I2SDF_EINVAL;
  mo_sample<<<blocks(count, MO_THREADS), MO_THREADS, 0, (hipStream_t)stream>>>(verts, (int32_t)n_verts, faces, F, cdf, u_face, u_bary, count, points,
                                                                    face_index, status);
  return i2sdf_hip_check(hipGetLastError(), "mo_sample");
}
