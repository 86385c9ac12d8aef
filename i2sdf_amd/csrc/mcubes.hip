// Marching cubes on the device: the SDF zero-level surface of an (nx, ny, nz) fp32 volume (z fastest, i2sdf_sdf_grid's volume
// order) as (verts, faces, normals) -- what model/eval/recon.py:53-60,91-95 and utils/plots.py:197-206 get from
// skimage.measure.marching_cubes on the host.  Case tables: mcubes_tables.inc, derived by gen_mc_tables.py (conventions there).
//
// Three phases, all deterministic (integer sums, fixed order, no atomics, no inter-workgroup flags):
//   classify  one thread per lattice point: crossing edges it owns (its +x, +y, +z edges) and the triangle count of the cell
//             whose low corner it is; one (vertices, triangles) pair per 256-point block;
//   scan      exclusive offsets of the block pairs, reduce-then-scan over workgroups in separate launches (1024 pairs per
//             workgroup per level);
//   emit      (a) vertices: block offset + in-block scan = the point's first vertex; stored with the point's 3-bit edge mask
//             so that (b) faces can look up the vertex of any edge of their cell through its owning point.
// Vertex order: lattice-point linear index, then axis x < y < z.  Face order: cell linear index, then table slot.
// Memory-bound: threads of a wave read consecutive z, every value is re-read from L2 by the neighbouring cells.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"

// every product and sum rounded on its own, like the numpy restatement of the tests (no fused multiply-adds)
#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;

#include "mcubes_tables.inc"

constexpr int MC_THREADS = 256;                  // lattice points per classify / emit block

struct Vol {
  const float* v;
  int nx, ny, nz;
  int64_t sx, sy;                                // strides of x and y (z is 1)
  int64_t n;
  float level;
};

struct Geo { float sp[3]; float org[3]; };

__device__ __forceinline__ int64_t axis_stride(const Vol& V, int a) { return a == 0 ? V.sx : (a == 1 ? V.sy : 1); }

__device__ __forceinline__ void unflatten(const Vol& V, int64_t p, int& i, int& j, int& k) {
  k = (int)(p % V.nz);
  const int64_t q = p / V.nz;
  j = (int)(q % V.ny);
  i = (int)(q / V.ny);
}

// bit a set iff the +a edge of point (i, j, k) exists and its ends straddle the level (NaN is not above)
__device__ __forceinline__ int edge_mask(const Vol& V, int64_t p, int i, int j, int k) {
  const bool a0 = V.v[p] > V.level;
  int m = 0;
  if (i < V.nx - 1 && ((V.v[p + V.sx] > V.level) != a0)) m |= 1;
  if (j < V.ny - 1 && ((V.v[p + V.sy] > V.level) != a0)) m |= 2;
  if (k < V.nz - 1 && ((V.v[p + 1] > V.level) != a0)) m |= 4;
  return m;
}

__device__ __forceinline__ int64_t corner_offset(const Vol& V, int c) { return (c & 1) * V.sx + ((c >> 1) & 1) * V.sy + ((c >> 2) & 1); }

// case byte of the cell whose low corner is p, or -1 when p is on an upper border (no cell)
__device__ __forceinline__ int cell_case(const Vol& V, int64_t p, int i, int j, int k) {
  if (i >= V.nx - 1 || j >= V.ny - 1 || k >= V.nz - 1) return -1;
  int cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cs |= (V.v[p + corner_offset(V, c)] > V.level ? 1 : 0) << c;
  return cs;
}

__global__ __launch_bounds__(MC_THREADS) void mc_classify(Vol V, longlong2* __restrict__ blk) {
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  longlong2 c = make_longlong2(0, 0);             // (vertices, triangles) of this point
  if (p < V.n) {
    int i, j, k;
    unflatten(V, p, i, j, k);
    c.x = __popc(edge_mask(V, p, i, j, k));
    const int cs = cell_case(V, p, i, j, k);
    if (cs >= 0) c.y = kMcNumTri[cs];
  }
  longlong2 tot;
  (void)block_excl_scan<MC_THREADS>(c, tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// np.gradient(vol, *spacing) at one point: central differences over 2*spacing, one-sided on the border
__device__ __forceinline__ float grad_axis(const Vol& V, int64_t p, int idx, int n, int64_t s, float sp) {
  if (idx == 0) return (V.v[p + s] - V.v[p]) / sp;
  if (idx == n - 1) return (V.v[p] - V.v[p - s]) / sp;
  return (V.v[p + s] - V.v[p - s]) / (2.0f * sp);
}

__device__ __forceinline__ void gradient(const Vol& V, const Geo& G, int64_t p, int i, int j, int k, float g[3]) {
  g[0] = grad_axis(V, p, i, V.nx, V.sx, G.sp[0]);
  g[1] = grad_axis(V, p, j, V.ny, V.sy, G.sp[1]);
  g[2] = grad_axis(V, p, k, V.nz, 1, G.sp[2]);
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_verts(Vol V, Geo G, const longlong2* __restrict__ blk, int32_t* __restrict__ pofs,
                                                            uint8_t* __restrict__ pmask, float* __restrict__ verts,
                                                            float* __restrict__ normals, int64_t cap_v) {
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int i = 0, j = 0, k = 0, m = 0;
  if (p < V.n) {
    unflatten(V, p, i, j, k);
    m = edge_mask(V, p, i, j, k);
  }
  int tot;
  int64_t off = block_excl_scan<MC_THREADS>((int)__popc(m), tot) + blk[blockIdx.x].x;
  if (p >= V.n) return;
  pofs[p] = (int32_t)off;
  pmask[p] = (uint8_t)m;
  if (!m) return;
  const int idx[3] = {i, j, k};
  float g0[3];
  gradient(V, G, p, i, j, k, g0);
  const float v0 = V.v[p];
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1)) continue;
    if (off >= cap_v) return;
    const int64_t q = p + axis_stride(V, a);
    const float v1 = V.v[q];
    const float t = (V.level - v0) / (v1 - v0);
    float g1[3];
    gradient(V, G, q, i + (a == 0), j + (a == 1), k + (a == 2), g1);
    float nv[3];
    for (int c = 0; c < 3; ++c) {
      const float e = c == a ? 1.0f : 0.0f;
      verts[3 * off + c] = G.org[c] + ((float)idx[c] + t * e) * G.sp[c];
      nv[c] = (1.0f - t) * g0[c] + t * g1[c];
    }
    const float len = sqrtf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
    for (int c = 0; c < 3; ++c) normals[3 * off + c] = -(nv[c] / len);
    ++off;
  }
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_faces(Vol V, const longlong2* __restrict__ blk, const int32_t* __restrict__ pofs,
                                                            const uint8_t* __restrict__ pmask, int32_t* __restrict__ faces, int64_t cap_f) {
  const int64_t p = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  int cs = -1;
  if (p < V.n) {
    int i, j, k;
    unflatten(V, p, i, j, k);
    cs = cell_case(V, p, i, j, k);
  }
  const int nt = cs >= 0 ? kMcNumTri[cs] : 0;
  int tot;
  const int64_t off = block_excl_scan<MC_THREADS>(nt, tot) + blk[blockIdx.x].y;
  for (int s = 0; s < nt; ++s) {
    if (off + s >= cap_f) return;
    for (int c = 0; c < 3; ++c) {
      const int e = kMcTriTable[cs][3 * s + c];
      const int a = e >> 2;
      const int64_t owner = p + corner_offset(V, kMcEdgeLo[e]);
      faces[3 * (off + s) + c] = pofs[owner] + __popc(pmask[owner] & ((1 << a) - 1));
    }
  }
}

// workspace: [pofs int32 n][pmask uint8 n][scan levels of longlong2 pairs ...][total pair], 16-byte aligned pieces
struct Layout {
  int64_t n, nb0;
  int64_t off_pofs, off_mask, off_total, bytes;
  ScanLevels scan;                               // level 0: the nb0 block pairs
};

bool layout(int32_t nx, int32_t ny, int32_t nz, Layout& L) {
  if (nx < 2 || ny < 2 || nz < 2) return false;
  L.n = (int64_t)nx * ny * nz;
  L.nb0 = (L.n + MC_THREADS - 1) / MC_THREADS;
  if (L.nb0 > INT32_MAX) return false;
  int64_t o = 0;
  L.off_pofs = o; o = align16(o + 4 * L.n);
  L.off_mask = o; o = align16(o + L.n);
  if (!scan_levels(L.nb0, sizeof(longlong2), o, L.scan)) return false;
  L.off_total = L.scan.bytes;
  L.bytes = L.off_total + 16;
  return true;
}

}  // namespace

extern "C" int64_t i2sdf_marching_cubes_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  Layout L;
  return layout(nx, ny, nz, L) ? L.bytes : 0;
}

extern "C" int i2sdf_marching_cubes_count(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace,
                                          int64_t* counts_out, void* stream) {
  Layout L;
  if (!vol || !workspace || !layout(nx, ny, nz, L)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const Vol V{vol, nx, ny, nz, (int64_t)ny * nz, nz, L.n, level};
  longlong2* total = (longlong2*)(ws + L.off_total);
  mc_classify<<<(unsigned)L.nb0, MC_THREADS, 0, st>>>(V, (longlong2*)(ws + L.scan.level_off[0]));
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mc_classify")) return rc;
  if (int rc = scan_levels_exclusive(ws, L.scan, total, st)) return rc;
  if (counts_out) return i2sdf_hip_check(hipMemcpyAsync(counts_out, total, 16, hipMemcpyDeviceToDevice, st), "marching cubes counts");
  return I2SDF_OK;
}

extern "C" int i2sdf_marching_cubes_emit(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing,
                                         const float* origin, void* workspace, float* verts, float* normals, int32_t* faces,
                                         int64_t cap_v, int64_t cap_f, void* stream) {
  Layout L;
  if (!vol || !workspace || !spacing || !origin || cap_v < 0 || cap_f < 0 || !layout(nx, ny, nz, L)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int64_t tot[2];
  if (int rc = i2sdf_hip_check(hipMemcpyAsync(tot, ws + L.off_total, 16, hipMemcpyDeviceToHost, st), "marching cubes counts")) return rc;
  if (int rc = i2sdf_hip_check(hipStreamSynchronize(st), "marching cubes counts")) return rc;
  if (tot[0] > INT32_MAX || tot[1] > INT32_MAX) return I2SDF_EINVAL;         // int32 vertex indices
  if (tot[0] > cap_v || tot[1] > cap_f) return I2SDF_EWORKSPACE;
  if (tot[1] == 0) return I2SDF_OK;                                            // (every crossing edge lies in some cell)
  if (!verts || !normals || !faces) return I2SDF_EINVAL;
  const Vol V{vol, nx, ny, nz, (int64_t)ny * nz, nz, L.n, level};
  Geo G;
  for (int c = 0; c < 3; ++c) { G.sp[c] = spacing[c]; G.org[c] = origin[c]; }
  const longlong2* blk = (const longlong2*)(ws + L.scan.level_off[0]);
  int32_t* pofs = (int32_t*)(ws + L.off_pofs);
  uint8_t* pmask = (uint8_t*)(ws + L.off_mask);
  mc_emit_verts<<<(unsigned)L.nb0, MC_THREADS, 0, st>>>(V, G, blk, pofs, pmask, verts, normals, cap_v);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "mc_emit_verts")) return rc;
  mc_emit_faces<<<(unsigned)L.nb0, MC_THREADS, 0, st>>>(V, blk, pofs, pmask, faces, cap_f);
  return i2sdf_hip_check(hipGetLastError(), "mc_emit_faces");
}
