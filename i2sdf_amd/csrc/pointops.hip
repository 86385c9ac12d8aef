// Point-set operations on the device, the scoring step right after the reference's mesh export (utils/mesh_util.py:evaluate,
// called by model/eval/recon.py:111-129, where open3d and a scikit-learn k-d tree run them on the host): voxel down-sampling,
// exact nearest neighbours, thresholded means.
//
//   bounds      per-axis minimum / maximum of the finite coordinates: wave reduction, then one integer atomicMin / atomicMax per
//               wave on the order-preserving integer image of the float (order-free, so bitwise reproducible).
//   down-sample open3d's rule: lo = min - voxel / 2, index = floor((p - lo) / voxel) in fp64, packed 21 bits per axis into one
//               key -> sorted by the caller (stable) -> heads of the runs (scanned by the caller) -> one thread per run sums its
//               points in fp64 in original index order and divides (a store-and-sum: no float atomics).
//   grid        a uniform grid over the reference's bounding box whose cell is enlarged until the grid fits the caller's table;
//               cell keys -> sorted by the caller (stable) -> cell start / end tables and the reference points re-ordered by cell
//               as (x, y, z, original index).
//   query       one query per lane: shells of cells of growing Chebyshev radius r around the query's (clamped) cell; a point
//               in a cell that has not been visited after shell r lies at least r cells away, so the search ends as soon as the best
//               distance is inside that bound or the shells cover the whole grid.  A query that exhausts its ring budget is
//               appended to a list ...
//   fallback    ... that a second pass answers exactly with one wave per query over all reference points.
//   reduce      fp64 sum and count(d < threshold) of a distance array: a fixed chunk per workgroup, then one workgroup over the
//               partial sums in a fixed order.
// Distances are fp32 from fp32 differences, compared as squares; ties go to the smaller reference index everywhere.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"

// every product and sum rounded on its own, like the numpy restatement of the tests (no fused multiply-adds)
#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using i2sdf_blockops::block_sum;
using i2sdf_blockops::fits;

constexpr int PO_THREADS = 256;
constexpr int PO_MAX_BLOCKS = 2048;                // grid-stride beyond that
constexpr int RED_CHUNK = 1024;                    // distances per workgroup in the first reduce stage
constexpr int64_t GRID_MAX_CELLS = (int64_t)1 << 22;
constexpr int GRID_MAX_DIM = 1024;
constexpr int VOXEL_BITS = 21;
constexpr int STATUS_NONFINITE = 1, STATUS_OVERFLOW = 2;

struct GridDesc {                                  // written by po_grid_setup at the head of the grid workspace
  double lo[3];
  double cell;
  int32_t dims[3];
  int32_t n_cells;
  float cell_f;
  int32_t pad;
};
constexpr int64_t WS_DESC = 0, WS_BOUNDS = 64, WS_TABLES = 128;      // byte offsets into the grid workspace

inline int64_t grid_table_cells(int64_t R) {      // cells the caller's tables hold, a function of R alone
  int64_t c = 2 * R;
  if (c < 64) c = 64;
  return c > GRID_MAX_CELLS ? GRID_MAX_CELLS : c;
}

// order-preserving image of a float in the unsigned integers
__device__ __forceinline__ uint32_t f_enc(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f_dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// ---------------------------------------------------------------------------------------------- bounds
__global__ void po_bounds_init(uint32_t* bounds) {
  if (threadIdx.x < 8) bounds[threadIdx.x] = threadIdx.x < 4 ? 0xffffffffu : 0u;      // [0..2] minima, [4..6] maxima
}

__global__ __launch_bounds__(PO_THREADS) void po_bounds(const float* __restrict__ pts, int64_t n, uint32_t* bounds, int32_t* status) {
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PO_THREADS) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (!finite3(p[0], p[1], p[2])) { bad = true; continue; }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t e = f_enc(p[c]);
      mn[c] = e < mn[c] ? e : mn[c];
      mx[c] = e > mx[c] ? e : mx[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t a = __shfl_xor(mn[c], d, 64), b = __shfl_xor(mx[c], d, 64);
      mn[c] = a < mn[c] ? a : mn[c];
      mx[c] = b > mx[c] ? b : mx[c];
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      atomicMin(bounds + c, mn[c]);
      atomicMax(bounds + 4 + c, mx[c]);
    }
  if (bad) atomicOr(status, STATUS_NONFINITE);
}

// ---------------------------------------------------------------------------------------------- voxel down-sampling
__global__ __launch_bounds__(PO_THREADS) void po_voxel_keys(const float* __restrict__ pts, int64_t n, const uint32_t* __restrict__ bounds,
                                                            double voxel, int64_t* __restrict__ keys, int32_t* status) {
  const double lo[3] = {(double)f_dec(bounds[0]) - 0.5 * voxel, (double)f_dec(bounds[1]) - 0.5 * voxel,
                        (double)f_dec(bounds[2]) - 0.5 * voxel};
  const double limit = (double)(1 << VOXEL_BITS);
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PO_THREADS) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int64_t key = INT64_MAX;
    if (!finite3(p[0], p[1], p[2])) {
      atomicOr(status, STATUS_NONFINITE);
    } else {
      const double t[3] = {floor(((double)p[0] - lo[0]) / voxel), floor(((double)p[1] - lo[1]) / voxel),
                           floor(((double)p[2] - lo[2]) / voxel)};
      if (t[0] >= 0.0 && t[1] >= 0.0 && t[2] >= 0.0 && t[0] < limit && t[1] < limit && t[2] < limit)
        key = ((int64_t)t[0] << (2 * VOXEL_BITS)) | ((int64_t)t[1] << VOXEL_BITS) | (int64_t)t[2];
      else
        atomicOr(status, STATUS_OVERFLOW);
    }
    keys[i] = key;
  }
}

__global__ __launch_bounds__(PO_THREADS) void po_voxel_heads(const int64_t* __restrict__ skeys, int64_t n, int32_t* __restrict__ heads) {
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PO_THREADS)
    heads[i] = i == 0 || skeys[i] != skeys[i - 1];
}

// the head of every run of equal keys sums the run: fp64, left to right (= original index order after the caller's stable sort)
__global__ __launch_bounds__(PO_THREADS) void po_voxel_mean(const float* __restrict__ pts, int64_t n, const int64_t* __restrict__ skeys,
                                                            const int64_t* __restrict__ perm, const int32_t* __restrict__ head_scan,
                                                            float* __restrict__ out, int32_t* __restrict__ counts, int64_t cap_m) {
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PO_THREADS) {
    const int64_t key = skeys[i];
    if (i > 0 && skeys[i - 1] == key) continue;
    const int64_t m = (int64_t)head_scan[i] - 1;   // inclusive scan: position + 1
    if (m < 0 || m >= cap_m) continue;
    double s[3] = {0.0, 0.0, 0.0};
    int64_t j = i;
    for (; j < n && skeys[j] == key; ++j) {
      const int64_t src = perm[j];
      if (src < 0 || src >= n) continue;           // (not a permutation of the points: nothing to add)
      s[0] += (double)pts[3 * src];
      s[1] += (double)pts[3 * src + 1];
      s[2] += (double)pts[3 * src + 2];
    }
    const double cnt = (double)(j - i);
    out[3 * m] = (float)(s[0] / cnt);
    out[3 * m + 1] = (float)(s[1] / cnt);
    out[3 * m + 2] = (float)(s[2] / cnt);
    counts[m] = (int32_t)(j - i);
  }
}

// ---------------------------------------------------------------------------------------------- grid
// one thread: the cell edge and the grid's shape from the bounding box.  About `target` cells; every axis at most
// GRID_MAX_DIM cells; the cell grows until the grid fits `cap` cells, so no bounding box can enlarge the tables.
__global__ void po_grid_setup(const uint32_t* __restrict__ bounds, int64_t cap, GridDesc* g) {
  if (threadIdx.x || blockIdx.x) return;
  double lo[3], ext[3], maxext = 0.0, vol = 1.0;
  int k = 0;
  for (int c = 0; c < 3; ++c) {
    lo[c] = (double)f_dec(bounds[c]);
    ext[c] = (double)f_dec(bounds[4 + c]) - lo[c];
    if (!(ext[c] >= 0.0) || !isfinite(ext[c]) || !isfinite(lo[c])) { ext[c] = 0.0; lo[c] = 0.0; }      // (no finite point at all)
    if (ext[c] > 0.0) { vol *= ext[c]; ++k; }
    maxext = ext[c] > maxext ? ext[c] : maxext;
  }
  double cell = 1.0;
  int32_t dims[3] = {1, 1, 1};
  if (k > 0) {
    cell = pow(vol / (double)(cap / 2), 1.0 / (double)k);
    const double floor_cell = maxext / (double)(GRID_MAX_DIM - 1);
    if (!(cell >= floor_cell)) cell = floor_cell;
    for (int it = 0; it < 4096; ++it) {
      int64_t total = 1;
      for (int c = 0; c < 3; ++c) {
        double d = floor(ext[c] / cell) + 1.0;
        if (!(d <= (double)GRID_MAX_DIM)) d = (double)GRID_MAX_DIM;
        dims[c] = (int32_t)d;
        total *= dims[c];
      }
      if (total <= cap) break;
      cell *= 1.125;
    }
    if ((int64_t)dims[0] * dims[1] * dims[2] > cap) { dims[0] = dims[1] = dims[2] = 1; cell = 2.0 * maxext; }     // (cannot happen)
  }
  for (int c = 0; c < 3; ++c) { g->lo[c] = lo[c]; g->dims[c] = dims[c]; }
  g->cell = cell;
  g->n_cells = dims[0] * dims[1] * dims[2];
  g->cell_f = (float)cell;
  g->pad = 0;
}

// cell coordinate of p along one axis, clamped into the grid (a query outside the box gets the nearest border cell; NaN -> 0)
__device__ __forceinline__ int cell_coord(float p, double lo, double cell, int dim) {
  const double t = floor(((double)p - lo) / cell);
  return t >= 0.0 ? (t < (double)dim ? (int)t : dim - 1) : 0;
}

__global__ __launch_bounds__(PO_THREADS) void po_grid_keys(const float* __restrict__ ref, int64_t R, const GridDesc* __restrict__ g,
                                                           int64_t* __restrict__ keys) {
  const GridDesc d = *g;
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < R; i += (int64_t)gridDim.x * PO_THREADS) {
    const int cx = cell_coord(ref[3 * i], d.lo[0], d.cell, d.dims[0]), cy = cell_coord(ref[3 * i + 1], d.lo[1], d.cell, d.dims[1]),
              cz = cell_coord(ref[3 * i + 2], d.lo[2], d.cell, d.dims[2]);
    keys[i] = ((int64_t)cx * d.dims[1] + cy) * d.dims[2] + cz;
  }
}

// sorted entry i: re-ordered copy of its point with its original index; run borders fill the cell tables (zeroed before)
__global__ __launch_bounds__(PO_THREADS) void po_grid_build(const float* __restrict__ ref, int64_t R, const int64_t* __restrict__ skeys,
                                                            const int64_t* __restrict__ perm, int64_t cap, int32_t* __restrict__ cell_start,
                                                            int32_t* __restrict__ cell_end, float4* __restrict__ sref) {
  for (int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; i < R; i += (int64_t)gridDim.x * PO_THREADS) {
    const int64_t key = skeys[i];
    int64_t src = perm[i];
    const bool ok = src >= 0 && src < R;
    if (!ok) src = 0;
    sref[i] = make_float4(ref[3 * src], ref[3 * src + 1], ref[3 * src + 2], __int_as_float(ok ? (int32_t)src : INT_MAX));
    if (key < 0 || key >= cap) continue;           // (keys that po_grid_keys did not write: the cell stays empty)
    if (i == 0 || skeys[i - 1] != key) cell_start[key] = (int32_t)i;
    if (i == R - 1 || skeys[i + 1] != key) cell_end[key] = (int32_t)(i + 1);
  }
}

// ---------------------------------------------------------------------------------------------- nearest neighbour
__device__ __forceinline__ void scan_cell(const float4* __restrict__ sref, int32_t b, int32_t e, float qx, float qy, float qz, float& best,
                                          int32_t& bi) {
  for (int32_t i = b; i < e; ++i) {
    const float4 p = sref[i];
    const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const int32_t idx = __float_as_int(p.w);
    if (d2 < best || (d2 == best && idx < bi)) { best = d2; bi = idx; }
  }
}

__global__ __launch_bounds__(PO_THREADS) void po_nn_query(const float* __restrict__ query, int64_t Q, const float4* __restrict__ sref, int64_t R,
                                                          const GridDesc* __restrict__ g, const int32_t* __restrict__ cell_start,
                                                          const int32_t* __restrict__ cell_end, int32_t max_ring, float* __restrict__ dist,
                                                          int32_t* __restrict__ index, int32_t* __restrict__ fb_list, int32_t* status) {
  const GridDesc d = *g;
  const int nx = d.dims[0], ny = d.dims[1], nz = d.dims[2];
  for (int64_t q = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x; q < Q; q += (int64_t)gridDim.x * PO_THREADS) {
    const float qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    if (!finite3(qx, qy, qz)) {
      atomicOr(status, STATUS_NONFINITE);
      dist[q] = __uint_as_float(0x7fc00000u);
      index[q] = -1;
      continue;
    }
    const int cx = cell_coord(qx, d.lo[0], d.cell, nx), cy = cell_coord(qy, d.lo[1], d.cell, ny), cz = cell_coord(qz, d.lo[2], d.cell, nz);
    float best = INFINITY;
    int32_t bi = INT_MAX;
    bool done = false;
    for (int r = 0; r <= max_ring && !done; ++r) {
      const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
      const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
      const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
      for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) {
          const int64_t row = ((int64_t)x * ny + y) * nz;
          if (x - cx == r || cx - x == r || y - cy == r || cy - y == r) {      // a side wall of the shell: the whole z range
            for (int z = z0; z <= z1; ++z) scan_cell(sref, cell_start[row + z], cell_end[row + z], qx, qy, qz, best, bi);
          } else {                                                           // inside the walls: bottom and top only
            if (cz - r >= 0) scan_cell(sref, cell_start[row + cz - r], cell_end[row + cz - r], qx, qy, qz, best, bi);
            if (r > 0 && cz + r <= nz - 1) scan_cell(sref, cell_start[row + cz + r], cell_end[row + cz + r], qx, qy, qz, best, bi);
          }
        }
      // everything not visited yet is at least r cells away (cell coordinates are exact to ~1e-13 cells; the bound keeps 1e-4)
      const float lb = (float)r * d.cell_f * 0.9999f;
      const bool covered = x0 == 0 && y0 == 0 && z0 == 0 && x1 == nx - 1 && y1 == ny - 1 && z1 == nz - 1;
      done = covered || best <= lb * lb;
    }
    dist[q] = sqrtf(best);
    index[q] = bi == INT_MAX ? -1 : bi;
    if (!done) {
      const int32_t pos = atomicAdd(status + 1, 1);
      if (pos < Q) fb_list[pos] = (int32_t)q;
    }
  }
}

// one wave per listed query over all reference points in their original order
__global__ __launch_bounds__(PO_THREADS) void po_nn_fallback(const float* __restrict__ query, int64_t Q, const float* __restrict__ ref, int64_t R,
                                                             const int32_t* __restrict__ fb_list, const int32_t* __restrict__ status,
                                                             float* __restrict__ dist, int32_t* __restrict__ index) {
  const int lane = threadIdx.x & 63;
  const int64_t n_waves = (int64_t)gridDim.x * (PO_THREADS / 64);
  int64_t n_fb = status[1];
  if (n_fb > Q) n_fb = Q;
  for (int64_t w = (int64_t)blockIdx.x * (PO_THREADS / 64) + (threadIdx.x >> 6); w < n_fb; w += n_waves) {
    const int64_t q = fb_list[w];
    if (q < 0 || q >= Q) continue;
    const float qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    float best = INFINITY;
    int32_t bi = INT_MAX;
    for (int64_t j = lane; j < R; j += 64) {
      const float dx = qx - ref[3 * j], dy = qy - ref[3 * j + 1], dz = qz - ref[3 * j + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best) { best = d2; bi = (int32_t)j; }           // (j ascends: the first of equal distances stays)
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const float ob = __shfl_xor(best, s, 64);
      const int32_t oi = __shfl_xor(bi, s, 64);
      if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) {
      dist[q] = sqrtf(best);
      index[q] = bi == INT_MAX ? -1 : bi;
    }
  }
}

// ---------------------------------------------------------------------------------------------- thresholded reduce
__global__ __launch_bounds__(PO_THREADS) void po_reduce_chunks(const float* __restrict__ dist, int64_t n, double threshold,
                                                               double* __restrict__ part) {
  const int64_t base = (int64_t)blockIdx.x * RED_CHUNK;
  double s = 0.0, c = 0.0;
#pragma unroll
  for (int u = 0; u < RED_CHUNK / PO_THREADS; ++u) {
    const int64_t i = base + u * PO_THREADS + threadIdx.x;
    if (i < n) {
      const double v = (double)dist[i];
      s += v;
      c += v < threshold ? 1.0 : 0.0;
    }
  }
  s = block_sum<PO_THREADS>(s);
  c = block_sum<PO_THREADS>(c);                    // (whole numbers below 2^53: exact in any order)
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = c; }
}

__global__ __launch_bounds__(PO_THREADS) void po_reduce_final(const double* __restrict__ part, int64_t n_part, double* __restrict__ out) {
  double s = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n_part; i += PO_THREADS) { s += part[2 * i]; c += part[2 * i + 1]; }
  s = block_sum<PO_THREADS>(s);
  c = block_sum<PO_THREADS>(c);
  if (threadIdx.x == 0) { out[0] = s; out[1] = c; }
}

inline unsigned blocks(int64_t n) { return i2sdf_blockops::blocks(n, PO_THREADS, PO_MAX_BLOCKS); }      // every kernel here strides

}  // namespace

extern "C" int i2sdf_points_bounds(const float* points, int64_t n, int32_t* bounds, int32_t* status, void* stream) {
  if (!fits(n) || !bounds || !status) return I2SDF_EINVAL;
  if (n > 0 && !points) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  po_bounds_init<<<1, 64, 0, st>>>((uint32_t*)bounds);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "po_bounds_init")) return rc;
  if (n == 0) return I2SDF_OK;
  po_bounds<<<blocks(n), PO_THREADS, 0, st>>>(points, n, (uint32_t*)bounds, status);
  return i2sdf_hip_check(hipGetLastError(), "po_bounds");
}

extern "C" int i2sdf_points_voxel_keys(const float* points, int64_t n, const int32_t* bounds, double voxel_size, int64_t* keys,
                                       int32_t* status, void* stream) {
  if (!fits(n) || !(voxel_size > 0.0) || !isfinite(voxel_size)) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  if (!points || !bounds || !keys || !status) return I2SDF_EINVAL;
  po_voxel_keys<<<blocks(n), PO_THREADS, 0, (hipStream_t)stream>>>(points, n, (const uint32_t*)bounds, voxel_size, keys, status);
  return i2sdf_hip_check(hipGetLastError(), "po_voxel_keys");
}

extern "C" int i2sdf_points_voxel_heads(const int64_t* sorted_keys, int64_t n, int32_t* heads, void* stream) {
  if (!fits(n)) return I2SDF_EINVAL;
  if (n == 0) return I2SDF_OK;
  if (!sorted_keys || !heads) return I2SDF_EINVAL;
  po_voxel_heads<<<blocks(n), PO_THREADS, 0, (hipStream_t)stream>>>(sorted_keys, n, heads);
  return i2sdf_hip_check(hipGetLastError(), "po_voxel_heads");
}

extern "C" int i2sdf_points_voxel_mean(const float* points, int64_t n, const int64_t* sorted_keys, const int64_t* perm,
                                       const int32_t* head_scan, float* out_points, int32_t* out_counts, int64_t cap_m, void* stream) {
  if (!fits(n) || !fits(cap_m)) return I2SDF_EINVAL;
  if (n == 0 || cap_m == 0) return I2SDF_OK;
  if (!points || !sorted_keys || !perm || !head_scan || !out_points || !out_counts) return I2SDF_EINVAL;
  po_voxel_mean<<<blocks(n), PO_THREADS, 0, (hipStream_t)stream>>>(points, n, sorted_keys, perm, head_scan, out_points, out_counts, cap_m);
  return i2sdf_hip_check(hipGetLastError(), "po_voxel_mean");
}

extern "C" int64_t i2sdf_points_grid_workspace_bytes(int64_t n_ref) {
  if (n_ref <= 0 || !fits(n_ref)) return 0;
  return WS_TABLES + 2 * 4 * grid_table_cells(n_ref);
}

extern "C" int i2sdf_points_grid_keys(const float* ref, int64_t n_ref, void* workspace, int64_t* keys, int32_t* status, void* stream) {
  if (n_ref <= 0 || !fits(n_ref) || !ref || !workspace || !keys || !status) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  uint32_t* bounds = (uint32_t*)((char*)workspace + WS_BOUNDS);
  GridDesc* g = (GridDesc*)((char*)workspace + WS_DESC);
  if (int rc = i2sdf_points_bounds(ref, n_ref, (int32_t*)bounds, status, stream)) return rc;
  po_grid_setup<<<1, 64, 0, st>>>(bounds, grid_table_cells(n_ref), g);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "po_grid_setup")) return rc;
  po_grid_keys<<<blocks(n_ref), PO_THREADS, 0, st>>>(ref, n_ref, g, keys);
  return i2sdf_hip_check(hipGetLastError(), "po_grid_keys");
}

extern "C" int i2sdf_points_grid_build(const float* ref, int64_t n_ref, const int64_t* sorted_keys, const int64_t* perm, void* workspace,
                                       float* sorted_ref, void* stream) {
  if (n_ref <= 0 || !fits(n_ref) || !ref || !sorted_keys || !perm || !workspace || !sorted_ref) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t cap = grid_table_cells(n_ref);
  int32_t* cell_start = (int32_t*)((char*)workspace + WS_TABLES);
  if (int rc = i2sdf_hip_check(hipMemsetAsync(cell_start, 0, 2 * 4 * cap, st), "grid tables")) return rc;
  po_grid_build<<<blocks(n_ref), PO_THREADS, 0, st>>>(ref, n_ref, sorted_keys, perm, cap, cell_start, cell_start + cap, (float4*)sorted_ref);
  return i2sdf_hip_check(hipGetLastError(), "po_grid_build");
}

extern "C" int i2sdf_points_nn_query(const float* query, int64_t n_query, const float* sorted_ref, int64_t n_ref, const void* workspace,
                                     int32_t max_ring, float* dist, int32_t* index, int32_t* fallback_list, int32_t* status, void* stream) {
  if (!fits(n_query) || n_ref <= 0 || !fits(n_ref) || max_ring < 0 || max_ring > GRID_MAX_DIM) return I2SDF_EINVAL;
  if (n_query == 0) return I2SDF_OK;
  if (!query || !sorted_ref || !workspace || !dist || !index || !fallback_list || !status) return I2SDF_EINVAL;
  const int64_t cap = grid_table_cells(n_ref);
  const int32_t* cell_start = (const int32_t*)((const char*)workspace + WS_TABLES);
  po_nn_query<<<blocks(n_query), PO_THREADS, 0, (hipStream_t)stream>>>(query, n_query, (const float4*)sorted_ref, n_ref,
                                                                        (const GridDesc*)((const char*)workspace + WS_DESC), cell_start,
                                                                        cell_start + cap, max_ring, dist, index, fallback_list, status);
  return i2sdf_hip_check(hipGetLastError(), "po_nn_query");
}

extern "C" int i2sdf_points_nn_fallback(const float* query, int64_t n_query, const float* ref, int64_t n_ref, const int32_t* fallback_list,
                                        const int32_t* status, float* dist, int32_t* index, void* stream) {
  if (!fits(n_query) || n_ref <= 0 || !fits(n_ref)) return I2SDF_EINVAL;
  if (n_query == 0) return I2SDF_OK;
  if (!query || !ref || !fallback_list || !status || !dist || !index) return I2SDF_EINVAL;
  const int64_t want = (n_query + PO_THREADS / 64 - 1) / (PO_THREADS / 64);      // a wave per query, at most
  po_nn_fallback<<<(unsigned)(want < PO_MAX_BLOCKS ? want : PO_MAX_BLOCKS), PO_THREADS, 0, (hipStream_t)stream>>>(
      query, n_query, ref, n_ref, fallback_list, status, dist, index);
  return i2sdf_hip_check(hipGetLastError(), "po_nn_fallback");
}

extern "C" int64_t i2sdf_points_reduce_workspace_bytes(int64_t n) {
  if (n <= 0 || !fits(n)) return 0;
  return 16 * ((n + RED_CHUNK - 1) / RED_CHUNK);
}

extern "C" int i2sdf_points_threshold_reduce(const float* dist, int64_t n, double threshold, void* workspace, double* out, void* stream) {
  if (n <= 0 || !fits(n) || !dist || !workspace || !out || threshold != threshold) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_part = (n + RED_CHUNK - 1) / RED_CHUNK;
  po_reduce_chunks<<<(unsigned)n_part, PO_THREADS, 0, st>>>(dist, n, threshold, (double*)workspace);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "po_reduce_chunks")) return rc;
  po_reduce_final<<<1, PO_THREADS, 0, st>>>((const double*)workspace, n_part, out);
  return i2sdf_hip_check(hipGetLastError(), "po_reduce_final");
}
