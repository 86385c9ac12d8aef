// TSDF fusion of depth maps and the extraction of its zero-level mesh on the device -- what utils/mesh_util.py:refuse and
// :depth2mesh get from open3d's ScalableTSDFVolume (integrate + extract_triangle_mesh) on the host.  The rule is restated from
// open3d's sources (not checked against a build of it):
//   1. a depth >= depth_trunc (or not > 0) is no measurement;
//   2. space is cut into units of 16^3 voxels; unit index of a point = floor(p / unit_len) per axis, unit_len = 16 voxel_length
//      (the CALLER rounds that product to fp32 once); voxel (i, j, k) of unit U has its centre at U unit_len + (i + 1/2) voxel_length;
//   3. camera c touches every unit between those of p - sdf_trunc and p + sdf_trunc (per axis, inclusive) for every back-projected
//      pixel p with u % stride == 0, v % stride == 0 and a measurement;
//   4. camera c is integrated into exactly the units it touched, cameras in list order: a voxel centre goes to the camera frame; if
//      z > 0 its pixel is (int)(x fx / z + cx + 0.5), (int)(y fy / z + cy + 0.5); inside the image and with a measurement d there,
//      sdf = (d - z) m(u, v), m = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1); if sdf > -sdf_trunc: t = min(1, sdf / sdf_trunc),
//      tsdf <- (tsdf w + t) / (w + 1), w <- w + 1;
//   5. marching cubes over cells of 8 neighbouring voxel centres, across unit borders: a cell counts iff its 8 voxels exist with w > 0;
//      a corner is inside iff tsdf < 0 (case bit c set iff NOT tsdf < 0); one vertex per crossing lattice edge that a counted cell
//      uses, at the linear interpolation between the two centres; mcubes_tables.inc (right-hand face normal towards positive tsdf).
//      Vertex normals: the normalised interpolated central-difference gradient of tsdf, pointing towards POSITIVE tsdf (the side the
//      cameras were on, the side of the face normals); a difference uses the neighbours that exist with w > 0 (both: (f+ - f-) / 2,
//      one: the one-sided difference, none: 0); a zero gradient gives a zero normal.
//
// Arithmetic: fp32, every product and sum rounded on its own in the order written (tests/refuse_ref.py follows it):
//   back-projection  xc = (((float)u - cx) d) / fx, yc = (((float)v - cy) d) / fy, zc = d; p_k = ((m[4k] xc + m[4k+1] yc) + m[4k+2] zc) + m[4k+3]
//                    with m the camera-to-world rows; unit range floorf((p_k - sdf_trunc) / unit_len) .. floorf((p_k + sdf_trunc) / unit_len)
//   centre           x_k = (float)U_k unit_len + ((float)i_k + 0.5f) voxel_length
//   camera frame     q_k = ((w[4k] x + w[4k+1] y) + w[4k+2] z) + w[4k+3], w the world-to-camera rows
//   pixel            fu = (((q_x fx) / q_z) + cx) + 0.5f, u = (int)fu (towards zero), inside iff -1 < fu < W; v alike
//   update           ax = ((float)u - cx) / fx, ay alike, m = sqrtf((ax ax + ay ay) + 1), sdf = (d - q_z) m, t = fminf(1, sdf / sdf_trunc),
//                    tsdf = (tsdf w + t) / (w + 1)
//   vertex           t = (0 - f0) / (f1 - f0), position = centre of the edge's low voxel, + t voxel_length along the edge's axis
//
// Memory grows with the touched units: a dense int32 table of unit slots spans the bounding box of all touched units (at most 2^24
// cells); tsdf and weight are fp32 arrays of 4096 voxels per allocated unit, voxel (i << 8 | j << 4 | k), k fastest.
//   bounds     integer atomic min / max of the touched unit indices over all cameras
//   mark       union pass (slot == NULL): stamp[cell] <- 1 for every touched cell, all cameras in one launch.  The CALLER scans the
//              stamps into the slot table (slots ascend with the cell index, i.e. with (ix, iy, iz)) and clears them.
//              camera pass: an integer atomicMax stamps the cell with c + 1; the lane that stamps it first appends the cell's slot to
//              the camera's list (the list's order varies from run to run; nothing depends on it)
//   integrate  workgroups stride over (listed unit, 256-voxel slab); one lane per voxel, so each voxel has one writer per camera
//   cells / count / emit   classify, scan (block sums by the caller) and emit as mcubes.hip does, over the allocated units; neighbours
//              across a unit border are found through the slot table.  Vertex order: unit slot, voxel, axis; faces: unit slot, voxel,
//              table slot.
// Everything is bitwise reproducible from run to run: values that several lanes write go through integer atomics or are the same
// constant from every writer (the union pass's stamps); every voxel and every output element has one writer per launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/i2sdf.h"
#include "blockops.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using i2sdf_blockops::block_excl_scan;

#include "mcubes_tables.inc"

constexpr int TS_THREADS = 256;
constexpr int TS_SLABS = 16;                      // 256-voxel slabs per unit
constexpr int TS_GRID_MAX = 1 << 16;              // workgroups of a striding launch
constexpr float TS_UNIT_LIMIT = 1048576.0f;       // |unit index| beyond 2^20 is refused (flag)

struct Pin {
  float fx, fy, cx, cy;
  int H, W;
  float vl, unit_len, trunc, dtrunc;
  int stride;
};

struct Grid {
  int umin[3], dims[3];
  int64_t cells, n_units;                        // (n_units: slots above it in the table are not followed)
};

__device__ __forceinline__ float measurement(float d, float dtrunc) { return (d > 0.0f && d < dtrunc) ? d : 0.0f; }

// unit range touched by the sampled pixel `idx` of camera cam; false: no measurement (or an index out of range: flag)
__device__ bool pixel_units(const Pin& P, const float* __restrict__ depths, const float* __restrict__ c2w, int cam, int64_t idx,
                            int lo[3], int hi[3], int32_t* flag) {
  const int Ws = (P.W + P.stride - 1) / P.stride;
  const int u = (int)(idx % Ws) * P.stride, v = (int)(idx / Ws) * P.stride;
  const float d = measurement(depths[((int64_t)cam * P.H + v) * P.W + u], P.dtrunc);
  if (!(d > 0.0f)) return false;
  const float xc = (((float)u - P.cx) * d) / P.fx, yc = (((float)v - P.cy) * d) / P.fy;
  const float* m = c2w + 12 * (int64_t)cam;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float p = ((m[4 * k] * xc + m[4 * k + 1] * yc) + m[4 * k + 2] * d) + m[4 * k + 3];
    const float a = floorf((p - P.trunc) / P.unit_len), b = floorf((p + P.trunc) / P.unit_len);
    if (!(fabsf(a) <= TS_UNIT_LIMIT && fabsf(b) <= TS_UNIT_LIMIT)) {
      *flag = 1;
      return false;
    }
    lo[k] = (int)a;
    hi[k] = (int)b;
  }
  return true;
}

// bounds int32[8]: min unit (3), max unit (3), flag, unused -- initialised by the caller to (INT32_MAX x 3, INT32_MIN x 3, 0, 0)
__global__ __launch_bounds__(TS_THREADS) void ts_bounds(Pin P, const float* __restrict__ depths, const float* __restrict__ c2w, int64_t n_s,
                                                        int32_t* __restrict__ bounds) {
  const int64_t idx = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  int lo[3], hi[3];
  if (idx >= n_s || !pixel_units(P, depths, c2w, blockIdx.y, idx, lo, hi, bounds + 6)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (lo[k] < bounds[k]) atomicMin(&bounds[k], lo[k]);          // (the plain read only saves atomics: the values move one way)
    if (hi[k] > bounds[3 + k]) atomicMax(&bounds[3 + k], hi[k]);
  }
}

// slot == NULL: union pass over cameras cam0 + blockIdx.y.  Otherwise the pass of camera cam0 alone.
__global__ __launch_bounds__(TS_THREADS) void ts_mark(Pin P, Grid G, const float* __restrict__ depths, const float* __restrict__ c2w, int cam0,
                                                      int64_t n_s, const int32_t* __restrict__ slot, int32_t* __restrict__ stamp,
                                                      int32_t* __restrict__ list, int32_t* __restrict__ list_count, int64_t n_units,
                                                      int32_t* __restrict__ flag) {
  const int64_t idx = (int64_t)blockIdx.x * TS_THREADS + threadIdx.x;
  const int cam = cam0 + blockIdx.y;
  int lo[3], hi[3];
  if (idx >= n_s || !pixel_units(P, depths, c2w, cam, idx, lo, hi, flag)) return;
  for (int x = lo[0]; x <= hi[0]; ++x)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int z = lo[2]; z <= hi[2]; ++z) {
        const int64_t cx = (int64_t)x - G.umin[0], cy = (int64_t)y - G.umin[1], cz = (int64_t)z - G.umin[2];
        if (cx < 0 || cy < 0 || cz < 0 || cx >= G.dims[0] || cy >= G.dims[1] || cz >= G.dims[2]) {   // (a grid that is not these depths')
          *flag = 1;
          continue;
        }
        const int64_t cell = (cx * G.dims[1] + cy) * G.dims[2] + cz;
        if (!slot) {
          // (plain stores from many lanes race here, but every one of them stores the same 1 into a cell that starts at 0, so the
          // result does not depend on who wins; the read before it only saves stores)
          if (stamp[cell] == 0) stamp[cell] = 1;
          continue;
        }
        const int s = slot[cell];
        if (s < 0 || s >= n_units) {
          *flag = 1;
          continue;
        }
        if (stamp[cell] == cam + 1) continue;                     // (already listed for this camera; only saves the atomic below, which decides)
        if (atomicMax(&stamp[cell], cam + 1) < cam + 1) {
          const int at = atomicAdd(list_count, 1);
          if (at < n_units) list[at] = s;
        }
      }
}

__device__ __forceinline__ void cell_coords(const Grid& G, int64_t cell, int c[3]) {
  c[2] = (int)(cell % G.dims[2]);
  const int64_t q = cell / G.dims[2];
  c[1] = (int)(q % G.dims[1]);
  c[0] = (int)(q / G.dims[1]);
}

__device__ __forceinline__ void voxel_centre(const Pin& P, const Grid& G, const int c[3], int lin, float x[3]) {
  const int ijk[3] = {lin >> 8, (lin >> 4) & 15, lin & 15};
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = (float)(G.umin[k] + c[k]) * P.unit_len + ((float)ijk[k] + 0.5f) * P.vl;
}

__global__ __launch_bounds__(TS_THREADS) void ts_integrate(Pin P, Grid G, const float* __restrict__ depth, const float* __restrict__ w2c,
                                                           const int32_t* __restrict__ unit_cell, const int32_t* __restrict__ list,
                                                           const int32_t* __restrict__ list_count, int64_t n_units, float* __restrict__ tsdf,
                                                           float* __restrict__ weight) {
  int64_t n = *list_count;
  if (n > n_units) n = n_units;
  for (int64_t it = blockIdx.x; it < n * TS_SLABS; it += gridDim.x) {
    const int s = list[it / TS_SLABS];
    if (s < 0 || s >= n_units) continue;
    const int lin = (int)(it % TS_SLABS) * TS_THREADS + threadIdx.x;
    int c[3];
    cell_coords(G, unit_cell[s], c);
    float x[3], q[3];
    voxel_centre(P, G, c, lin, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((w2c[4 * k] * x[0] + w2c[4 * k + 1] * x[1]) + w2c[4 * k + 2] * x[2]) + w2c[4 * k + 3];
    if (!(q[2] > 0.0f)) continue;
    const float fu = (((q[0] * P.fx) / q[2]) + P.cx) + 0.5f, fv = (((q[1] * P.fy) / q[2]) + P.cy) + 0.5f;
    if (!(fu > -1.0f && fu < (float)P.W && fv > -1.0f && fv < (float)P.H)) continue;
    const int u = (int)fu, v = (int)fv;
    const float d = measurement(depth[(int64_t)v * P.W + u], P.dtrunc);
    if (!(d > 0.0f)) continue;
    const float ax = ((float)u - P.cx) / P.fx, ay = ((float)v - P.cy) / P.fy;
    const float m = sqrtf((ax * ax + ay * ay) + 1.0f);
    const float sdf = (d - q[2]) * m;
    if (!(sdf > -P.trunc)) continue;
    const float t = fminf(1.0f, sdf / P.trunc);
    const int64_t at = (int64_t)s * 4096 + lin;
    const float w = weight[at];
    tsdf[at] = (tsdf[at] * w + t) / (w + 1.0f);
    weight[at] = w + 1.0f;
  }
}

// voxel (unit cell coordinates c, in-unit i j k) + (di, dj, dk), each offset in [-1, 2]: its index in the voxel arrays, or -1
__device__ __forceinline__ int64_t neighbour(const Grid& G, const int32_t* __restrict__ slot, const int c[3], int lin, int di, int dj, int dk) {
  int ijk[3] = {(lin >> 8) + di, ((lin >> 4) & 15) + dj, (lin & 15) + dk};
  int cc[3] = {c[0], c[1], c[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (ijk[k] < 0) { ijk[k] += 16; --cc[k]; }
    else if (ijk[k] >= 16) { ijk[k] -= 16; ++cc[k]; }
    if (cc[k] < 0 || cc[k] >= G.dims[k]) return -1;
  }
  const int s = slot[((int64_t)cc[0] * G.dims[1] + cc[1]) * G.dims[2] + cc[2]];
  return s < 0 || s >= G.n_units ? -1 : (int64_t)s * 4096 + (ijk[0] << 8 | ijk[1] << 4 | ijk[2]);
}

// cellcase[voxel] = case byte of the cell whose low corner the voxel is, -1 when the cell does not count
__global__ __launch_bounds__(TS_THREADS) void ts_cells(Grid G, const int32_t* __restrict__ slot, const int32_t* __restrict__ unit_cell,
                                                       const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                       int16_t* __restrict__ cellcase) {
  const int s = blockIdx.x / TS_SLABS, lin = (blockIdx.x % TS_SLABS) * TS_THREADS + threadIdx.x;
  int c[3];
  cell_coords(G, unit_cell[s], c);
  int cs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t q = neighbour(G, slot, c, lin, k & 1, (k >> 1) & 1, (k >> 2) & 1);
    if (q < 0 || !(weight[q] > 0.0f)) { cs = -1; break; }
    cs |= (tsdf[q] < 0.0f ? 0 : 1) << k;
  }
  cellcase[(int64_t)s * 4096 + lin] = (int16_t)cs;
}

// bit a set iff the +a edge of the voxel crosses the level and a counted cell uses it
__device__ int edge_mask(const Grid& G, const int32_t* __restrict__ slot, const int c[3], int lin, int64_t self, const float* __restrict__ tsdf,
                         const int16_t* __restrict__ cellcase) {
  int m = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, d = (a + 2) % 3;
    bool used = false;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      int off[3] = {0, 0, 0};
      off[b] = -(o & 1);
      off[d] = -(o >> 1);
      const int64_t q = o == 0 ? self : neighbour(G, slot, c, lin, off[0], off[1], off[2]);
      if (q >= 0 && cellcase[q] >= 0) used = true;
    }
    if (!used) continue;                        // (a counted cell: both ends of the edge exist with w > 0)
    const int64_t q = neighbour(G, slot, c, lin, a == 0, a == 1, a == 2);
    if (q >= 0 && ((tsdf[q] < 0.0f) != (tsdf[self] < 0.0f))) m |= 1 << a;
  }
  return m;
}

__global__ __launch_bounds__(TS_THREADS) void ts_count(Grid G, const int32_t* __restrict__ slot, const int32_t* __restrict__ unit_cell,
                                                       const float* __restrict__ tsdf, const int16_t* __restrict__ cellcase,
                                                       uint8_t* __restrict__ emask, int64_t* __restrict__ blk) {
  const int s = blockIdx.x / TS_SLABS, lin = (blockIdx.x % TS_SLABS) * TS_THREADS + threadIdx.x;
  const int64_t self = (int64_t)s * 4096 + lin;
  int c[3];
  cell_coords(G, unit_cell[s], c);
  const int m = edge_mask(G, slot, c, lin, self, tsdf, cellcase);
  emask[self] = (uint8_t)m;
  const int cs = cellcase[self];
  int tv, tt;
  (void)block_excl_scan<TS_THREADS>((int)__popc(m), tv);
  (void)block_excl_scan<TS_THREADS>(cs >= 0 ? kMcNumTri[cs] : 0, tt);
  if (threadIdx.x == 0) { blk[2 * (int64_t)blockIdx.x] = tv; blk[2 * (int64_t)blockIdx.x + 1] = tt; }
}

// central difference of tsdf along every axis at voxel `self` (see the head of the file)
__device__ void gradient(const Grid& G, const int32_t* __restrict__ slot, const int c[3], int lin, int64_t self, const float* __restrict__ tsdf,
                         const float* __restrict__ weight, float g[3]) {
  const float f0 = tsdf[self];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int64_t p = neighbour(G, slot, c, lin, a == 0, a == 1, a == 2), n = neighbour(G, slot, c, lin, -(a == 0), -(a == 1), -(a == 2));
    const bool hp = p >= 0 && weight[p] > 0.0f, hn = n >= 0 && weight[n] > 0.0f;
    g[a] = hp && hn ? (tsdf[p] - tsdf[n]) / 2.0f : (hp ? tsdf[p] - f0 : (hn ? f0 - tsdf[n] : 0.0f));
  }
}

__global__ __launch_bounds__(TS_THREADS) void ts_emit_verts(Pin P, Grid G, const int32_t* __restrict__ slot, const int32_t* __restrict__ unit_cell,
                                                            const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                            const uint8_t* __restrict__ emask, const int64_t* __restrict__ blk_excl,
                                                            int32_t* __restrict__ pofs, float* __restrict__ verts, float* __restrict__ normals,
                                                            int64_t cap_v) {
  const int s = blockIdx.x / TS_SLABS, lin = (blockIdx.x % TS_SLABS) * TS_THREADS + threadIdx.x;
  const int64_t self = (int64_t)s * 4096 + lin;
  const int m = emask[self];
  int tot;
  int64_t off = block_excl_scan<TS_THREADS>((int)__popc(m), tot) + blk_excl[2 * (int64_t)blockIdx.x];
  pofs[self] = (int32_t)off;
  if (!m) return;
  int c[3];
  cell_coords(G, unit_cell[s], c);
  float x[3], g0[3];
  voxel_centre(P, G, c, lin, x);
  gradient(G, slot, c, lin, self, tsdf, weight, g0);
  const float f0 = tsdf[self];
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1)) continue;
    if (off >= cap_v) return;
    const int64_t q = neighbour(G, slot, c, lin, a == 0, a == 1, a == 2);     // (exists: the mask says so)
    const float t = (0.0f - f0) / (tsdf[q] - f0);
    // the neighbour's own unit coordinates and in-unit index, for its gradient
    int ijk[3] = {lin >> 8, (lin >> 4) & 15, lin & 15}, cc[3] = {c[0], c[1], c[2]};
    if (++ijk[a] == 16) { ijk[a] = 0; ++cc[a]; }
    float g1[3], nv[3];
    gradient(G, slot, cc, ijk[0] << 8 | ijk[1] << 4 | ijk[2], q, tsdf, weight, g1);
    for (int k = 0; k < 3; ++k) {
      verts[3 * off + k] = k == a ? x[k] + t * P.vl : x[k];
      nv[k] = (1.0f - t) * g0[k] + t * g1[k];
    }
    const float len = sqrtf((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2]);
    for (int k = 0; k < 3; ++k) normals[3 * off + k] = len > 0.0f ? nv[k] / len : 0.0f;
    ++off;
  }
}

__global__ __launch_bounds__(TS_THREADS) void ts_emit_faces(Grid G, const int32_t* __restrict__ slot, const int32_t* __restrict__ unit_cell,
                                                            const int16_t* __restrict__ cellcase, const uint8_t* __restrict__ emask,
                                                            const int64_t* __restrict__ blk_excl, const int32_t* __restrict__ pofs,
                                                            int32_t* __restrict__ faces, int64_t cap_f) {
  const int s = blockIdx.x / TS_SLABS, lin = (blockIdx.x % TS_SLABS) * TS_THREADS + threadIdx.x;
  const int64_t self = (int64_t)s * 4096 + lin;
  const int cs = cellcase[self];
  const int nt = cs >= 0 ? kMcNumTri[cs] : 0;
  int tot;
  const int64_t off = block_excl_scan<TS_THREADS>(nt, tot) + blk_excl[2 * (int64_t)blockIdx.x + 1];
  if (!nt) return;
  int c[3];
  cell_coords(G, unit_cell[s], c);
  for (int r = 0; r < nt; ++r) {
    if (off + r >= cap_f) return;
    for (int k = 0; k < 3; ++k) {
      const int e = kMcTriTable[cs][3 * r + k];
      const int a = e >> 2, lo = kMcEdgeLo[e];
      const int64_t owner = neighbour(G, slot, c, lin, lo & 1, (lo >> 1) & 1, (lo >> 2) & 1);   // (exists: the cell counts)
      faces[3 * (off + r) + k] = pofs[owner] + __popc(emask[owner] & ((1 << a) - 1));
    }
  }
}

bool pin(const float* K4, int32_t H, int32_t W, float vl, float unit_len, float trunc, float dtrunc, int32_t stride, Pin& P) {
  if (!K4 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX || stride < 1) return false;
  if (!(K4[0] > 0.0f && K4[1] > 0.0f && K4[0] < INFINITY && K4[1] < INFINITY && fabsf(K4[2]) < INFINITY && fabsf(K4[3]) < INFINITY)) return false;
  if (!(vl > 0.0f && vl < INFINITY && unit_len > 0.0f && unit_len < INFINITY && trunc > 0.0f && trunc < INFINITY && dtrunc > 0.0f)) return false;
  P = Pin{K4[0], K4[1], K4[2], K4[3], H, W, vl, unit_len, trunc, dtrunc, stride};
  return true;
}

int64_t grid_cells(const int32_t* grid6) {
  if (!grid6) return 0;
  int64_t n = 1;
  for (int k = 0; k < 3; ++k) {
    const int64_t d = grid6[3 + k];
    if (d < 1 || d > I2SDF_TSDF_MAX_CELLS || llabs((int64_t)grid6[k]) > (1 << 21)) return 0;
    n *= d;
    if (n > I2SDF_TSDF_MAX_CELLS) return 0;
  }
  return n;
}

bool grid(const int32_t* grid6, int64_t n_units, Grid& G) {
  G.cells = grid_cells(grid6);
  G.n_units = n_units;
  if (!G.cells) return false;
  for (int k = 0; k < 3; ++k) { G.umin[k] = grid6[k]; G.dims[k] = grid6[3 + k]; }
  return true;
}

int64_t sampled(const Pin& P) { return (int64_t)((P.W + P.stride - 1) / P.stride) * ((P.H + P.stride - 1) / P.stride); }

bool units_ok(int64_t n_units) { return n_units >= 1 && n_units <= I2SDF_TSDF_MAX_CELLS; }

}  // namespace

extern "C" int64_t i2sdf_tsdf_table_cells(const int32_t* grid6) { return grid_cells(grid6); }

extern "C" int64_t i2sdf_tsdf_extract_workspace_bytes(int64_t n_units) {
  // per voxel: cellcase int16, emask uint8 (padded to 4 bytes together), pofs int32
  return units_ok(n_units) ? n_units * 4096 * 8 : 0;
}

extern "C" int i2sdf_tsdf_bounds(const float* depths, int32_t n_cam, int32_t H, int32_t W, const float* c2w, const float* K4, float voxel_length,
                                 float unit_length, float sdf_trunc, float depth_trunc, int32_t stride, int32_t* bounds, void* stream) {
  Pin P;
  if (n_cam < 0 || n_cam > 65535 || !pin(K4, H, W, voxel_length, unit_length, sdf_trunc, depth_trunc, stride, P)) return I2SDF_EINVAL;
  if (n_cam == 0) return I2SDF_OK;
  if (!depths || !c2w || !bounds) return I2SDF_EINVAL;
  const int64_t n_s = sampled(P);
  ts_bounds<<<dim3((unsigned)((n_s + TS_THREADS - 1) / TS_THREADS), (unsigned)n_cam), TS_THREADS, 0, (hipStream_t)stream>>>(P, depths, c2w, n_s, bounds);
  return i2sdf_hip_check(hipGetLastError(), "ts_bounds");
}

extern "C" int i2sdf_tsdf_mark(const float* depths, int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float* c2w, const float* K4,
                               float voxel_length, float unit_length, float sdf_trunc, float depth_trunc, int32_t stride, const int32_t* grid6,
                               const int32_t* slot, int64_t n_units, int32_t* stamp, int32_t* list, int32_t* list_count, int32_t* flag,
                               void* stream) {
  Pin P;
  Grid G;
  if (n_cam < 0 || n_cam > 65535 || !pin(K4, H, W, voxel_length, unit_length, sdf_trunc, depth_trunc, stride, P) || !grid(grid6, n_units, G)) return I2SDF_EINVAL;
  if (n_cam == 0) return I2SDF_OK;
  if (!depths || !c2w || !stamp || !flag) return I2SDF_EINVAL;
  if (slot && (cam < 0 || cam >= n_cam || !list || !list_count || !units_ok(n_units))) return I2SDF_EINVAL;
  const int64_t n_s = sampled(P);
  const dim3 g((unsigned)((n_s + TS_THREADS - 1) / TS_THREADS), slot ? 1u : (unsigned)n_cam);
  ts_mark<<<g, TS_THREADS, 0, (hipStream_t)stream>>>(P, G, depths, c2w, slot ? cam : 0, n_s, slot, stamp, list, list_count, n_units, flag);
  return i2sdf_hip_check(hipGetLastError(), "ts_mark");
}

extern "C" int i2sdf_tsdf_integrate(const float* depths, int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float* w2c, const float* K4,
                                    float voxel_length, float unit_length, float sdf_trunc, float depth_trunc, const int32_t* grid6,
                                    const int32_t* unit_cell, int64_t n_units, const int32_t* list, const int32_t* list_count, float* tsdf,
                                    float* weight, void* stream) {
  Pin P;
  Grid G;
  if (n_cam < 1 || n_cam > 65535 || cam < 0 || cam >= n_cam || !pin(K4, H, W, voxel_length, unit_length, sdf_trunc, depth_trunc, 1, P) ||
      !grid(grid6, n_units, G) || !units_ok(n_units))
    return I2SDF_EINVAL;
  if (!depths || !w2c || !unit_cell || !list || !list_count || !tsdf || !weight) return I2SDF_EINVAL;
  const int64_t want = n_units * TS_SLABS;
  ts_integrate<<<(unsigned)(want < TS_GRID_MAX ? want : TS_GRID_MAX), TS_THREADS, 0, (hipStream_t)stream>>>(
      P, G, depths + (int64_t)cam * H * W, w2c + 12 * (int64_t)cam, unit_cell, list, list_count, n_units, tsdf, weight);
  return i2sdf_hip_check(hipGetLastError(), "ts_integrate");
}

extern "C" int i2sdf_tsdf_count(const int32_t* grid6, const int32_t* slot, const int32_t* unit_cell, int64_t n_units, const float* tsdf,
                                const float* weight, void* workspace, int64_t* blocks, void* stream) {
  Grid G;
  if (!grid(grid6, n_units, G) || !units_ok(n_units) || !slot || !unit_cell || !tsdf || !weight || !workspace || !blocks) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = n_units * 4096;
  int16_t* cellcase = (int16_t*)workspace;
  uint8_t* emask = (uint8_t*)workspace + 2 * nv;
  const unsigned nb = (unsigned)(n_units * TS_SLABS);
  ts_cells<<<nb, TS_THREADS, 0, st>>>(G, slot, unit_cell, tsdf, weight, cellcase);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "ts_cells")) return rc;
  ts_count<<<nb, TS_THREADS, 0, st>>>(G, slot, unit_cell, tsdf, cellcase, emask, blocks);
  return i2sdf_hip_check(hipGetLastError(), "ts_count");
}

extern "C" int i2sdf_tsdf_emit(const int32_t* grid6, float voxel_length, float unit_length, const int32_t* slot, const int32_t* unit_cell,
                               int64_t n_units, const float* tsdf, const float* weight, void* workspace, const int64_t* blocks_excl, float* verts,
                               float* normals, int32_t* faces, int64_t cap_v, int64_t cap_f, void* stream) {
  Grid G;
  if (!grid(grid6, n_units, G) || !units_ok(n_units) || !slot || !unit_cell || !tsdf || !weight || !workspace || !blocks_excl) return I2SDF_EINVAL;
  if (!(voxel_length > 0.0f && voxel_length < INFINITY && unit_length > 0.0f && unit_length < INFINITY) || cap_v < 0 || cap_f < 0 ||
      cap_v > INT32_MAX || cap_f > INT32_MAX)
    return I2SDF_EINVAL;
  if (cap_v == 0 || cap_f == 0) return I2SDF_OK;
  if (!verts || !normals || !faces) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nv = n_units * 4096;
  const int16_t* cellcase = (const int16_t*)workspace;
  const uint8_t* emask = (const uint8_t*)workspace + 2 * nv;
  int32_t* pofs = (int32_t*)((char*)workspace + 4 * nv);
  Pin P{};
  P.vl = voxel_length;
  P.unit_len = unit_length;
  const unsigned nb = (unsigned)(n_units * TS_SLABS);
  ts_emit_verts<<<nb, TS_THREADS, 0, st>>>(P, G, slot, unit_cell, tsdf, weight, emask, blocks_excl, pofs, verts, normals, cap_v);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "ts_emit_verts")) return rc;
  ts_emit_faces<<<nb, TS_THREADS, 0, st>>>(G, slot, unit_cell, cellcase, emask, blocks_excl, pofs, faces, cap_f);
  return i2sdf_hip_check(hipGetLastError(), "ts_emit_faces");
}
