// Density clustering (DBSCAN) of a point cloud on the device -- the `use_dbscan` seeding of I2SDFNetwork.init_emission_groups
// (model/network/__init__.py:50-65, where sklearn.cluster.DBSCAN labels 10 000 sampled points on the host).  include/i2sdf.h,
// section "Density clustering", states the law; this file computes it on the whole cloud without (n, n) or neighbour-list storage.
//
//   cells     bounds of the finite points (i2sdf_points_bounds) -> cell edge c = (eps / 2)(1 + 2^-20), cell coordinate
//             floor((p - lo) / c) in fp64, 21 bits per axis in one int64 key -> sorted by the caller (stable) -> run heads, an exclusive
//             scan of them (blockops.h) -> the unique keys and the start of every occupied cell.  The cells are SPARSE: there is no dense
//             table; a neighbour cell is found by binary search in the unique keys.
//   waves     one wave owns one occupied cell in every kernel below.  Its lanes look the 125 cells around it up once (lane l: offsets l
//             and l + 64), keep the answers in registers and hand them round by shuffles; then the lanes sweep a neighbour cell's points
//             together, 64 at a time, and the votes end the sweep as early as the law allows.
//   core      a cell with min_samples points or more: all of them are core, no distance is formed (two points of one cell are always
//             within eps).  Otherwise each point counts its neighbours and stops at min_samples.  The cell's core points are hooked to
//             the smallest of them (plain stores: no union runs in that launch).
//   unions    for a pair of neighbouring cells with core points whose roots differ when looked at: ONE core pair within eps is searched,
//             the search ends at the first hit, and lane 0 calls unite() (unionfind.h).  Two launches: the 26 adjacent cells first, the
//             98 cells of the second shell after them, when most roots already agree.
//   labels    a flag at every root, an exclusive scan, n_clusters = the total; a core point takes rank[root]; a non-core point the
//             smallest rank among the neighbour cells holding a core point within eps (all core points of a cell share a root, so one hit
//             settles a cell).
// No kernel waits for another workgroup: no spin lock, no grid barrier, no polled flag.  A retry follows only a lost compare-and-swap.
// Everything is stream ordered; the host reads nothing.  Every output is an order-free function of the input.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"
#include "blockops.h"
#include "unionfind.h"

// every difference, product and sum rounded on its own, like the numpy restatement of the tests (no fused multiply-adds)
#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

using namespace i2sdf_blockops;
using i2sdf_unionfind::find_root;
using i2sdf_unionfind::unite;

constexpr int DB_THREADS = 256, DB_WAVES = DB_THREADS / 64;
constexpr int DB_MAX_BLOCKS = 2048;                // grid-stride beyond that
constexpr int CELL_BITS = 21;
constexpr int STATUS_NONFINITE = 1, STATUS_CELLS = 2;
constexpr int64_t NO_KEY = INT64_MAX;              // a point without a cell (non-finite, or beyond the 2^21 cells); sorts last
constexpr int N_SLOTS = 125, OWN_SLOT = 62;        // the 5 x 5 x 5 cells around a cell; slot = ((dx + 2) 5 + dy + 2) 5 + dz + 2

struct Header {                                    // head of the workspace
  uint32_t bounds[8];                              // i2sdf_points_bounds: [0..2] minima, [4..6] maxima (order-preserving images)
  int32_t flags;                                   // STATUS_* of i2sdf_dbscan_cell_keys
  int32_t n_cells, n_valid;                        // occupied cells; sorted entries that have a cell (they come first)
  int32_t pad;
};
constexpr int64_t WS_HEADER = 256;

struct Layout {                                    // byte offsets into the workspace
  ScanLevels L;                                    // int32 scan levels: run heads, later root flags
  int64_t spts, ukey, cstart, croot, parent, score, bytes;
};

inline bool layout(int64_t n, Layout& w) {
  if (!scan_levels(n, 4, WS_HEADER, w.L)) return false;
  int64_t o = align16(w.L.bytes);
  w.spts = o;   o += 16 * n;                       // float4 per sorted entry: x, y, z, original index (-1: no point)
  w.ukey = o;   o = align16(o + 8 * n);            // int64 per occupied cell
  w.cstart = o; o = align16(o + 4 * (n + 1));      // int32: first sorted entry of a cell; [n_cells] = n_valid
  w.croot = o;  o = align16(o + 4 * n);            // int32 per cell: its smallest core point, -1 without one
  w.parent = o; o = align16(o + 4 * n);            // int32 per point (original index): union-find
  w.score = o;  o = align16(o + n);                // uint8 per sorted entry: core flag
  w.bytes = o;
  return true;
}

__device__ __forceinline__ float f_dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the test of the law: fp64 differences of the fp32 coordinates, squares added x, y, z; inclusive.  (A NaN coordinate fails it.)
__device__ __forceinline__ bool within(const float4 a, const float4 b, double eps2) {
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  const double d2 = dx * dx + dy * dy + dz * dz;
  return d2 <= eps2;
}

__device__ __forceinline__ int32_t cells_of(const Header* h) { return (h->flags & STATUS_CELLS) ? 0 : h->n_cells; }

// ---------------------------------------------------------------------------------------------- cell keys
__global__ __launch_bounds__(DB_THREADS) void db_keys_kernel(const float* __restrict__ pts, int64_t n, Header* h, double cell,
                                                             int64_t* __restrict__ keys) {
  const double lo[3] = {(double)f_dec(h->bounds[0]), (double)f_dec(h->bounds[1]), (double)f_dec(h->bounds[2])};
  const double limit = (double)(1 << CELL_BITS);
  int flags = 0;
  for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DB_THREADS) {
    const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int64_t key = NO_KEY;
    if (!finite3(p[0], p[1], p[2])) {
      flags |= STATUS_NONFINITE;
    } else {
      const double t[3] = {floor(((double)p[0] - lo[0]) / cell), floor(((double)p[1] - lo[1]) / cell), floor(((double)p[2] - lo[2]) / cell)};
      if (t[0] >= 0.0 && t[1] >= 0.0 && t[2] >= 0.0 && t[0] < limit && t[1] < limit && t[2] < limit)
        key = ((int64_t)t[0] << (2 * CELL_BITS)) | ((int64_t)t[1] << CELL_BITS) | (int64_t)t[2];
      else
        flags |= STATUS_CELLS;
    }
    keys[i] = key;
  }
  if (flags) atomicOr(&h->flags, flags);
}

__global__ void db_status_kernel(const Header* h, int32_t* status, int32_t* n_clusters) {
  if (threadIdx.x || blockIdx.x) return;
  *status = h->flags;
  if (n_clusters && (h->flags & STATUS_CELLS)) *n_clusters = 0;
}

// ---------------------------------------------------------------------------------------------- sorted entries -> cells
// sorted entry i: its point with its original index, its run-head flag; original index i: the start values of everything per point
__global__ __launch_bounds__(DB_THREADS) void db_gather_kernel(const float* __restrict__ pts, int64_t n, const int64_t* __restrict__ skeys,
                                                               const int64_t* __restrict__ perm, Header* h, float4* __restrict__ spts,
                                                               int32_t* __restrict__ heads, int32_t* __restrict__ croot,
                                                               int32_t* __restrict__ parent, uint8_t* __restrict__ score,
                                                               int64_t* __restrict__ labels, uint8_t* __restrict__ core) {
  const float nan = __uint_as_float(0x7fc00000u);
  for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DB_THREADS) {
    const int64_t key = skeys[i], src = perm[i];
    const bool ok = key != NO_KEY && src >= 0 && src < n;      // (not a permutation of the points: the entry holds no point)
    spts[i] = ok ? make_float4(pts[3 * src], pts[3 * src + 1], pts[3 * src + 2], __int_as_float((int32_t)src))
                 : make_float4(nan, nan, nan, __int_as_float(-1));
    heads[i] = key != NO_KEY && (i == 0 || skeys[i - 1] != key);
    if (key != NO_KEY && (i == n - 1 || skeys[i + 1] == NO_KEY)) h->n_valid = (int32_t)(i + 1);
    croot[i] = -1;
    parent[i] = (int32_t)i;
    score[i] = 0;
    labels[i] = -1;
    core[i] = 0;
  }
}

__global__ __launch_bounds__(DB_THREADS) void db_cells_kernel(const int64_t* __restrict__ skeys, int64_t n, const int32_t* __restrict__ head_scan,
                                                              const Header* h, int64_t* __restrict__ ukey, int32_t* __restrict__ cstart) {
  const int64_t m = h->n_cells;                    // <= n: at most one head per entry
  for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DB_THREADS) {
    const int64_t key = skeys[i];
    if (key == NO_KEY || (i > 0 && skeys[i - 1] == key)) continue;
    const int64_t c = head_scan[i];                // exclusive scan of the heads: the cell's number
    if (c < 0 || c >= n) continue;
    ukey[c] = key;
    cstart[c] = (int32_t)i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && m >= 0 && m <= n) {
    const int32_t v = h->n_valid;
    cstart[m] = v < 0 ? 0 : (v > n ? (int32_t)n : v);
  }
}

// ---------------------------------------------------------------------------------------------- the cells around a cell
__device__ __forceinline__ int32_t find_cell(const int64_t* __restrict__ ukey, int32_t m, int64_t key) {
  int32_t lo = 0, hi = m;
  for (int it = 0; it < 32 && lo < hi; ++it) {     // (m < 2^31: 31 halvings at most)
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (ukey[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo < m && ukey[lo] == key ? lo : -1;
}

// the occupied cell at offset `slot` from the cell of `key` whose Chebyshev distance lies in ring_lo .. ring_hi, or -1
__device__ __forceinline__ int32_t neighbour_cell(const int64_t* __restrict__ ukey, int32_t m, int64_t key, int slot, int ring_lo, int ring_hi) {
  if (slot >= N_SLOTS) return -1;
  const int dx = slot / 25 - 2, dy = (slot / 5) % 5 - 2, dz = slot % 5 - 2;
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
  const int ring = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
  if (ring < ring_lo || ring > ring_hi) return -1;
  const int64_t mask = ((int64_t)1 << CELL_BITS) - 1;
  const int64_t x = (key >> (2 * CELL_BITS)) + dx, y = ((key >> CELL_BITS) & mask) + dy, z = (key & mask) + dz;
  if (x < 0 || y < 0 || z < 0 || x > mask || y > mask || z > mask) return -1;
  return find_cell(ukey, m, (x << (2 * CELL_BITS)) | (y << CELL_BITS) | z);
}

// first / end sorted entry of cell c, clamped so that a malformed table is never read out of range
__device__ __forceinline__ void cell_range(const int32_t* __restrict__ cstart, int32_t c, int64_t n, int64_t& s, int64_t& e) {
  s = cstart[c];
  e = cstart[c + 1];
  if (s < 0) s = 0;
  if (e > n) e = n;
}

// The neighbour cells of a wave live in two registers per lane (slots lane and lane + 64).  FOR_NEIGHBOURS walks the occupied ones in
// slot order: `b` is the cell, `sl` the lane holding it, `hi` whether it is the lane's second register.
#define FOR_NEIGHBOURS(n0, n1)                                                                          \
  for (int hi = 0; hi < 2; ++hi)                                                                        \
    for (uint64_t todo = __ballot((hi ? n1 : n0) >= 0); todo; todo &= todo - 1)                         \
      if (const int sl = __ffsll((unsigned long long)todo) - 1; true)                                   \
        if (const int32_t b = __shfl(hi ? n1 : n0, sl, 64); true)

// ---------------------------------------------------------------------------------------------- core flags
__global__ __launch_bounds__(DB_THREADS) void db_core_kernel(const float4* __restrict__ spts, int64_t n, const Header* h,
                                                             const int64_t* __restrict__ ukey, const int32_t* __restrict__ cstart,
                                                             double eps2, int32_t min_samples, uint8_t* score, int32_t* __restrict__ croot,
                                                             int32_t* parent, uint8_t* __restrict__ core) {
  const int lane = threadIdx.x & 63;
  const int32_t m = cells_of(h);
  const int64_t n_waves = (int64_t)gridDim.x * DB_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); c < m; c += n_waves) {
    int64_t s, e;
    cell_range(cstart, (int32_t)c, n, s, e);
    int32_t mine = INT_MAX;                        // smallest core index this lane has seen
    if (e - s >= min_samples) {                    // a dense cell: every point is core (two points of one cell are within eps)
      for (int64_t i = s + lane; i < e; i += 64) {
        const int32_t w = __float_as_int(spts[i].w);
        if (w < 0) continue;
        score[i] = 1;
        core[w] = 1;
        mine = w < mine ? w : mine;
      }
    } else {
      const int32_t n0 = neighbour_cell(ukey, m, ukey[c], lane, 0, 2), n1 = neighbour_cell(ukey, m, ukey[c], lane + 64, 0, 2);
      for (int64_t i = s; i < e; ++i) {            // (fewer than min_samples points; the lanes share each point's count)
        const float4 p = spts[i];
        const int32_t w = __float_as_int(p.w);
        if (w < 0) continue;
        int32_t count = 0;
        FOR_NEIGHBOURS(n0, n1) {
          if (count >= min_samples) break;
          int64_t bs, be;
          cell_range(cstart, b, n, bs, be);
          for (int64_t j0 = bs; j0 < be && count < min_samples; j0 += 64) {
            const int64_t j = j0 + lane;
            const bool hit = j < be && within(p, spts[j], eps2);
            count += __popcll(__ballot(hit));
          }
        }
        if (count >= min_samples && lane == (int)((i - s) & 63)) {      // (the lane that reads score[i] back below)
          score[i] = 1;
          core[w] = 1;
          mine = w < mine ? w : mine;
        }
      }
    }
    const int32_t first = wave_min(mine);
    if (first == INT_MAX) continue;                // no core point here
    if (lane == 0) croot[c] = first;
    for (int64_t i = s + lane; i < e; i += 64) {
      const int32_t w = __float_as_int(spts[i].w);
      if (w > first && score[i]) parent[w] = first;      // (w < n by db_gather_kernel; first < w: the invariant of unionfind.h)
    }
  }
}

// ---------------------------------------------------------------------------------------------- unions across cells
__global__ __launch_bounds__(DB_THREADS) void db_pairs_kernel(const float4* __restrict__ spts, int64_t n, const Header* h,
                                                              const int64_t* __restrict__ ukey, const int32_t* __restrict__ cstart,
                                                              const uint8_t* __restrict__ score, const int32_t* __restrict__ croot,
                                                              double eps2, int ring_lo, int ring_hi, int32_t* parent) {
  const int lane = threadIdx.x & 63;
  const int32_t m = cells_of(h);
  const int64_t n_waves = (int64_t)gridDim.x * DB_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); c < m; c += n_waves) {
    const int32_t ra = croot[c];
    if (ra < 0) continue;
    int32_t n0 = neighbour_cell(ukey, m, ukey[c], lane, ring_lo, ring_hi), n1 = neighbour_cell(ukey, m, ukey[c], lane + 64, ring_lo, ring_hi);
    if (n0 >= 0 && (n0 <= c || croot[n0] < 0)) n0 = -1;       // every unordered pair once, from its lower cell; core points on both sides
    if (n1 >= 0 && (n1 <= c || croot[n1] < 0)) n1 = -1;
    int64_t s, e;
    cell_range(cstart, (int32_t)c, n, s, e);
    FOR_NEIGHBOURS(n0, n1) {
      const int32_t rb = croot[b];
      int differ = 0;
      if (lane == 0) differ = find_root(parent, ra) != find_root(parent, rb);
      if (!__shfl(differ, 0, 64)) continue;        // already one component when looked at
      int64_t bs, be;
      cell_range(cstart, b, n, bs, be);
      bool found = false;
      for (int64_t i = s; i < e && !found; ++i) {
        if (!score[i]) continue;
        const float4 p = spts[i];
        for (int64_t j0 = bs; j0 < be; j0 += 64) {
          const int64_t j = j0 + lane;
          const bool hit = j < be && score[j] && within(p, spts[j], eps2);
          if (__any(hit)) { found = true; break; }
        }
      }
      if (found && lane == 0) unite(parent, ra, rb);
    }
  }
}

// ---------------------------------------------------------------------------------------------- labels
__global__ __launch_bounds__(DB_THREADS) void db_roots_kernel(const uint8_t* __restrict__ core, int64_t n, int32_t* parent,
                                                              int32_t* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * DB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DB_THREADS) {
    int32_t f = 0;
    if (core[i]) {
      const int32_t r = find_root(parent, (int32_t)i);
      f = r == (int32_t)i;
      if (!f) __hip_atomic_store(parent + i, r, I2SDF_UF_RLX);      // (others may still walk through i: the root is an ancestor)
    }
    flags[i] = f;
  }
}

__global__ __launch_bounds__(DB_THREADS) void db_labels_kernel(const float4* __restrict__ spts, int64_t n, const Header* h,
                                                               const int64_t* __restrict__ ukey, const int32_t* __restrict__ cstart,
                                                               const uint8_t* __restrict__ score, const int32_t* __restrict__ croot,
                                                               int32_t* parent, const int32_t* __restrict__ rank, double eps2,
                                                               int32_t min_samples, int64_t* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int32_t m = cells_of(h);
  const int64_t n_waves = (int64_t)gridDim.x * DB_WAVES;
  for (int64_t c = (int64_t)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); c < m; c += n_waves) {
    int64_t s, e;
    cell_range(cstart, (int32_t)c, n, s, e);
    const int32_t rc = croot[c];
    if (rc >= 0) {                                 // the cell's core points share one root (no union runs any more)
      const int32_t own = rank[find_root(parent, rc)];
      for (int64_t i = s + lane; i < e; i += 64) {
        const int32_t w = __float_as_int(spts[i].w);
        if (w >= 0 && score[i]) labels[w] = own;
      }
    }
    if (e - s >= min_samples) continue;            // a dense cell has core points only
    int32_t n0 = neighbour_cell(ukey, m, ukey[c], lane, 0, 2), n1 = neighbour_cell(ukey, m, ukey[c], lane + 64, 0, 2);
    int32_t r0 = INT_MAX, r1 = INT_MAX;            // the cluster of each neighbour cell's core points
    if (n0 >= 0) { const int32_t r = croot[n0]; if (r < 0) n0 = -1; else r0 = rank[find_root(parent, r)]; }
    if (n1 >= 0) { const int32_t r = croot[n1]; if (r < 0) n1 = -1; else r1 = rank[find_root(parent, r)]; }
    for (int64_t i = s; i < e; ++i) {
      const float4 p = spts[i];
      const int32_t w = __float_as_int(p.w);
      if (w < 0 || score[i]) continue;
      int32_t best = INT_MAX;
      FOR_NEIGHBOURS(n0, n1) {
        const int32_t rb = __shfl(hi ? r1 : r0, sl, 64);
        if (rb >= best) continue;                  // this cell cannot lower the label
        int64_t bs, be;
        cell_range(cstart, b, n, bs, be);
        for (int64_t j0 = bs; j0 < be; j0 += 64) {
          const int64_t j = j0 + lane;
          const bool hit = j < be && score[j] && within(p, spts[j], eps2);
          if (__any(hit)) { best = rb; break; }
        }
      }
      if (best != INT_MAX && lane == 0) labels[w] = best;
    }
  }
}

inline unsigned blocks(int64_t n) { return i2sdf_blockops::blocks(n, DB_THREADS, DB_MAX_BLOCKS); }       // one thread per point, striding
inline unsigned cell_blocks(int64_t n) { return i2sdf_blockops::blocks(n, DB_WAVES, 2 * DB_MAX_BLOCKS); }   // one wave per cell, striding

inline bool aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
inline bool size_ok(int64_t n) { return n >= 1 && fits(n); }
inline bool eps_ok(double eps) { return isfinite(eps) && eps > 0.0 && isfinite(eps * eps) && eps * eps > 0.0; }

}  // namespace

extern "C" int64_t i2sdf_dbscan_workspace_bytes(int64_t n) {
  Layout w;
  if (!size_ok(n) || !layout(n, w)) return 0;
  return w.bytes;
}

extern "C" int i2sdf_dbscan_cell_keys(const float* points, int64_t n, double eps, void* workspace, int64_t* keys, int32_t* status,
                                      void* stream) {
  Layout w;
  if (!size_ok(n) || !eps_ok(eps) || !layout(n, w)) return I2SDF_EINVAL;
  if (!aligned(points, 4) || !aligned(workspace, 16) || !aligned(keys, 8) || !aligned(status, 4)) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  Header* h = (Header*)workspace;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(h, 0, WS_HEADER, st), "dbscan header")) return rc;
  if (int rc = i2sdf_points_bounds(points, n, (int32_t*)h->bounds, &h->flags, stream)) return rc;
  const double cell = (0.5 * eps) * (1.0 + 1.0 / 1048576.0);
  db_keys_kernel<<<blocks(n), DB_THREADS, 0, st>>>(points, n, h, cell, keys);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_keys_kernel")) return rc;
  db_status_kernel<<<1, 64, 0, st>>>(h, status, nullptr);
  return i2sdf_hip_check(hipGetLastError(), "db_status_kernel");
}

extern "C" int i2sdf_dbscan_label(const float* points, int64_t n, double eps, int32_t min_samples, const int64_t* sorted_keys,
                                  const int64_t* perm, void* workspace, int64_t* labels, uint8_t* core, int32_t* n_clusters, int32_t* status,
                                  void* stream) {
  Layout w;
  if (!size_ok(n) || !eps_ok(eps) || min_samples < 1 || !layout(n, w)) return I2SDF_EINVAL;
  if (!aligned(points, 4) || !aligned(sorted_keys, 8) || !aligned(perm, 8) || !aligned(workspace, 16) || !aligned(labels, 8) || !core ||
      !aligned(n_clusters, 4) || !aligned(status, 4))
    return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Header* h = (Header*)ws;
  int32_t* scan0 = (int32_t*)(ws + w.L.level_off[0]);
  float4* spts = (float4*)(ws + w.spts);
  int64_t* ukey = (int64_t*)(ws + w.ukey);
  int32_t *cstart = (int32_t*)(ws + w.cstart), *croot = (int32_t*)(ws + w.croot), *parent = (int32_t*)(ws + w.parent);
  uint8_t* score = (uint8_t*)(ws + w.score);
  const double eps2 = eps * eps;

  if (int rc = i2sdf_hip_check(hipMemsetAsync(&h->n_cells, 0, 8, st), "dbscan counts")) return rc;      // n_cells, n_valid
  db_gather_kernel<<<blocks(n), DB_THREADS, 0, st>>>(points, n, sorted_keys, perm, h, spts, scan0, croot, parent, score, labels, core);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_gather_kernel")) return rc;
  if (int rc = scan_levels_exclusive<int32_t>(ws, w.L, &h->n_cells, st)) return rc;
  db_cells_kernel<<<blocks(n), DB_THREADS, 0, st>>>(sorted_keys, n, scan0, h, ukey, cstart);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_cells_kernel")) return rc;
  db_core_kernel<<<cell_blocks(n), DB_THREADS, 0, st>>>(spts, n, h, ukey, cstart, eps2, min_samples, score, croot, parent, core);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_core_kernel")) return rc;
  for (int ring = 1; ring <= 2; ++ring) {
    db_pairs_kernel<<<cell_blocks(n), DB_THREADS, 0, st>>>(spts, n, h, ukey, cstart, score, croot, eps2, ring, ring, parent);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "db_pairs_kernel")) return rc;
  }
  db_roots_kernel<<<blocks(n), DB_THREADS, 0, st>>>(core, n, parent, scan0);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_roots_kernel")) return rc;
  if (int rc = scan_levels_exclusive<int32_t>(ws, w.L, n_clusters, st)) return rc;
  db_labels_kernel<<<cell_blocks(n), DB_THREADS, 0, st>>>(spts, n, h, ukey, cstart, score, croot, parent, scan0, eps2, min_samples, labels);
  if (int rc = i2sdf_hip_check(hipGetLastError(), "db_labels_kernel")) return rc;
  db_status_kernel<<<1, 64, 0, st>>>(h, status, n_clusters);
  return i2sdf_hip_check(hipGetLastError(), "db_status_kernel");
}
