// Host-side plan of i2sdf_weight_grads (wgrad.hip): which GEMM tasks a training step has, and in which launches they run.  No device code,
// no HIP call: wgrad.hip enqueues what wgrad_passes() returns, tests/wgrad_probe.cpp prints it.  Internal linkage (the kernels take WgLaunch / WnTab).
#pragma once
#include <algorithm>
#include <vector>
#include "mlp_common.h"

namespace {

constexpr int WG_CH = I2SDF_WG_CH;   // points per split-M chunk (plan.h; plan.cpp: PART_ALIGN -- point ranges are cut at chunk boundaries)
constexpr int MAX_TASKS = 30;
// dynamic LDS of the 4-wave kernels (the layouts: wgrad.hip, at wgrad_narrow_body and wgrad3p_body)
constexpr int WGW_SLOT = (16 * 16 + 4) * 64;               // floats of one wave's partial 128x128 tile (+ 4 bias sums) in LDS
constexpr int WGN_LDS_BYTES = 2 * WGW_SLOT * 4;            // two such slots (wgrad_wide_body) > three narrow partials (3 * (8 * 16 + 4) * 64 * 4)
constexpr int W3P_PL = 4 * 4 * 3 * 256;                    // floats per plane stage: 4 quarters x 4 tiles x 3 planes x 1 KB (48 KB)
constexpr int W3P_SLOTS = 2;
constexpr int W3P_LDS_BYTES = W3P_SLOTS * W3P_PL * 4;      // 96 KB of the CU's 160 KB

// A / B point at column a_c0 / b_c0 of the operand's first row in the POINT-MAJOR sense; a_blk / b_blk = leading points of the
// operand tensor stored in the blocked layout (mlp_common.h; only 256-wide tensors, accessed as 128-column tiles, are ever blocked)
// a_p24 / b_p24: the operand's blocked points are packed 24-bit records (x3.h P24: abars, gus, gas under I2SDF_OPT_SAVES24; only 256-wide tensors,
// read by the split-arithmetic kernels)
struct WgJob { const float* A; const float* B; int32_t lda, ldb, a_w, b_w; int64_t m_count; int64_t a_blk, b_blk; int32_t a_c0, b_c0; int32_t a_p24, b_p24; };
// The operand shape of a task decides which body runs it (narrow operands run 4x / 2x fewer MFMAs per point pair)
enum WgVariant : int32_t {
  WG_TILE = 0,          // 128 x 128 tile, neither operand narrow: wgrad_kernel, in split arithmetic wgrad_wide_body
  WG_NARROW_A = 1,      // A at most 32 columns (the output rows)
  WG_NARROW_B32 = 2,    // B at most 32 columns (PE(view) columns)
  WG_NARROW_B64 = 3,    // B at most 64 columns (PE(x) columns)
  WG_BLOCK = 4          // a whole 256 x 256 block in split arithmetic: wgrad3p_body
};
struct WgTask {
  WgJob j[2];
  int32_t njobs, relu_b, has_bias, rows_store, cols_store, ldo;
  int32_t variant, pad;      // WgVariant
  int64_t out_off, bias_off;
};
struct WgLaunch { WgTask t[MAX_TASKS]; int32_t n; int32_t chunk0; int64_t chunk_stride; float* partials; };     // chunk0: first chunk of this launch (point ranges)

inline int32_t wg_variant(const WgTask& x) {
  const WgJob& j = x.j[0];
  return j.a_w == 256 ? WG_BLOCK : j.a_w <= 32 ? WG_NARROW_A : j.b_w <= 32 ? WG_NARROW_B32 : j.b_w <= 64 ? WG_NARROW_B64 : WG_TILE;
}

// where layer l's bias sums sit in a chunk's partials: behind its [wg_rows x wg_cols] block
inline int64_t bias_off(const i2sdf::NetPlan& np, int l) { return np.wgrad_off[l] + (int64_t)np.wg_rows[l] * np.wg_cols[l]; }

struct Src { const float* p; int ld; int w; int64_t blk = 0; int p24 = 0; };     // a [Mp][ld] matrix, the width used from it, blocked-prefix points, those as packed 24-bit records

struct TaskList {
  std::vector<WgTask> tasks;
  bool quads = false;        // emit one 256x256 task (bf16x3 kernel) where both operands are 256 wide
  // Emit the tiles of layer l's weight block.  rows: segments of A (one per source, stacked in block rows at row0[i]);
  // cols: segments of B.  job 0 = (A0[i], B0[k]) over mA0[i] points, job 1 = (A1[i], B1[k]) over m1 points (optional).
  void add_block(const i2sdf::NetPlan& np, int l, const std::vector<Src>& A0, const std::vector<Src>& A1, const std::vector<int>& row0,
                 const std::vector<int64_t>& mA0, const std::vector<Src>& B0, const std::vector<Src>& B1, int64_t m1, bool relu_b) {
    const int ldo = np.wg_cols[l];
    int col0 = 0;
    for (size_t k = 0; k < B0.size(); ++k) {
      // the [aw x bw] tile at (r0, c0) of segment pair (i, k); the first tile of a block row also sums A's columns (the bias gradient)
      auto add = [&](size_t i, int r0, int c0, int aw, int bw) {
        WgTask t{};
        t.j[0] = WgJob{A0[i].p + r0, B0[k].p + c0, A0[i].ld, B0[k].ld, aw, bw, mA0[i], A0[i].blk, B0[k].blk, r0, c0, A0[i].p24, B0[k].p24};
        t.njobs = 1;
        if (!A1.empty() && A1[i].p != nullptr && !B1.empty()) {
          t.j[1] = WgJob{A1[i].p + r0, B1[k].p + c0, A1[i].ld, B1[k].ld, aw, bw, m1, A1[i].blk, B1[k].blk, r0, c0, A1[i].p24, B1[k].p24};
          t.njobs = 2;
        }
        t.relu_b = relu_b ? 1 : 0;
        t.has_bias = (k == 0 && c0 == 0) ? 1 : 0;
        t.rows_store = aw; t.cols_store = bw; t.ldo = ldo;
        t.out_off = np.wgrad_off[l] + (int64_t)(row0[i] + r0) * ldo + col0 + c0;
        t.bias_off = bias_off(np, l) + row0[i] + r0;
        t.variant = wg_variant(t);
        tasks.push_back(t);
      };
      auto quad = [&](size_t i) { return quads && B0[k].w == 256 && A0[i].w == 256; };
      for (size_t i = 0; i < A0.size(); ++i)
        if (quad(i)) add(i, 0, 0, 256, 256);
      for (int ct = 0; ct * 128 < B0[k].w; ++ct)
        for (size_t i = 0; i < A0.size(); ++i) {
          if (quad(i)) continue;
          for (int rt = 0; rt * 128 < A0[i].w; ++rt) add(i, rt * 128, ct * 128, std::min(128, A0[i].w - rt * 128), std::min(128, B0[k].w - ct * 128));
        }
      col0 += B0[k].w;
    }
  }
};

inline bool wgrad_has_rgb(const i2sdf_train_buffers* tb) { return tb->M_main > 0 && tb->gar; }
inline bool wgrad_has_light(const i2sdf_plan* p, const i2sdf_train_buffers* tb) { return p->light.d.n_lin > 0 && tb->M_main > 0 && tb->gal0; }

// every GEMM task of a step, net by net and layer by layer
inline std::vector<WgTask> wgrad_tasks(const i2sdf_plan* p, const i2sdf_train_buffers* tb) {
  const int64_t Mp = tb->Mp, Ms = tb->M_sdf, Mm = tb->M_main;
  TaskList tl;
  tl.quads = p->wgrad_bf16x3 != 0;
  {  // ---- SDF net
    const i2sdf::NetPlan& np = p->sdf;
    const i2sdf_mlp_desc& d = np.d;
    const int L = d.n_lin, H = d.hidden, F = p->F, PEC8 = i2sdf::cdiv(d.in0, 8) * 8;
    const int64_t ls = Mp * H;
    const int64_t bs = (H == 256) ? i2sdf::sdf_blocked_points(p, Ms, Mp) : 0;      // leading points of hs / abars / gus / gas in the blocked layout
    const int s24 = (H == 256 && i2sdf::sdf_saves24(p) && bs == Mp) ? 1 : 0;       // abars / gus / gas as packed 24-bit records (hs stays fp32)
    for (int l = 0; l < L - 1; ++l) {
      std::vector<Src> B0, B1;
      if (l == 0) { B0 = {{tb->pe, PEC8, PEC8}}; B1 = {{tb->gpbar, PEC8, PEC8}}; }
      else {
        B0 = {{tb->hs + (l - 1) * ls, H, H, bs}}; B1 = {{tb->gus + l * ls, H, H, bs, s24}};
        if (l == d.skip_layer) { B0.push_back({tb->pe, PEC8, PEC8}); B1.push_back({tb->gpbar, PEC8, PEC8}); }
      }
      tl.add_block(np, l, {{tb->gas + l * ls, H, H, bs, s24}}, {{tb->abars + l * ls, H, H, bs, s24}}, {0}, {Ms}, B0, B1, Ms, false);
    }
    std::vector<Src> A0 = {{tb->ga_last4, 4, 4}}, A1 = {{tb->ones4, 4, 4}};
    std::vector<int> row0 = {0};
    std::vector<int64_t> mA0 = {Ms};
    if (F > 0 && Mm > 0 && tb->fbar) { A0.push_back({tb->fbar, F, F}); A1.push_back({nullptr, 0, 0}); row0.push_back(32); mA0.push_back(Mm); }
    tl.add_block(np, L - 1, A0, A1, row0, mA0, {{tb->hs + (L - 2) * ls, H, H, bs}}, {{tb->gus + (L - 1) * ls, H, H, bs}}, Ms,
                 false);       // (gus[L-1] stays fp32: x3.h X3Sweep2Src)
  }
  if (wgrad_has_rgb(tb)) {  // ---- radiance net
    const i2sdf::NetPlan& np = p->rgb;
    const i2sdf_mlp_desc& d = np.d;
    const int L = d.n_lin, H = d.hidden, F = p->F, PV8 = i2sdf::side_chunks(d) * 8;
    const int64_t ls = Mp * H;
    const int64_t br = (H == 256) ? i2sdf::rgb_blocked_points(p, Mm, Mp) : 0;     // leading points of rs / gar in the blocked layout
    for (int l = 0; l < L; ++l) {
      std::vector<Src> B0;
      if (l == 0) B0 = {{tb->pev, PV8, PV8}, {tb->feat, F, F}};
      else B0 = {{tb->rs + (l - 1) * ls, H, H, br}};
      std::vector<Src> A0;
      if (l < L - 1) A0 = {{tb->gar + l * ls, H, H, br}};
      else A0 = {{tb->ga_last_rgb, 4, 4}};
      tl.add_block(np, l, A0, {}, {0}, {Mm}, B0, {}, 0, false);
    }
  }
  if (wgrad_has_light(p, tb)) {  // ---- light head: l=0: A = G(a_0), B = relu(feature) ; l=1: A = G(a_1), B = softplus acts
    const i2sdf::NetPlan& np = p->light;
    const int H = np.d.hidden, F = p->F;
    tl.add_block(np, 0, {{tb->gal0, H, H}}, {}, {0}, {Mm}, {{tb->feat, F, F}}, {}, 0, true);
    tl.add_block(np, 1, {{tb->gal_last, 4, 4}}, {}, {0}, {Mm}, {{tb->hl, H, H}}, {}, 0, false);
  }
  return tl.tasks;
}

// ---- the launches: a pass is one kernel over a list of tasks, cut into WgLaunch batches of at most MAX_TASKS; grid = (chunks, tasks) ----
//   WGK_ALL*    wgrad_all_kernel<NPL>: blocks and narrow tasks of a point range as ONE grid; NPL = 2 under I2SDF_OPT_WGRAD_BF16X2, else 3
//   WGK_BLOCKS* wgrad3p_kernel<NPL>: the 256 x 256 blocks
//   WGK_TILES   wgrad_kernel<0, 0>: one wave per 128 x 128 tile, fp32-input MFMA (the plans without split arithmetic)
//   WGK_NARROW* wgrad_narrow_kernel<NPL>: every narrow tile in one launch of 4-wave workgroups.  bf16 split with THREE planes whenever the
//               256x256 blocks run in split arithmetic (then also the 128 x 128 tiles), else fp32-input MFMA.  Also under I2SDF_OPT_WGRAD_BF16X2:
//               bound by its operand reads (4.0-4.7 TB/s, matrix pipe 8-16 % busy), the third plane costs 20 us per launch and keeps
//               these few blocks fp32-equivalent
enum WgKernel { WGK_ALL2, WGK_ALL3, WGK_BLOCKS2, WGK_BLOCKS3, WGK_TILES, WGK_NARROW3, WGK_NARROW0, WGK_COUNT };
struct WgPass {
  WgKernel kern;
  int threads, lds_bytes;
  bool side;                          // without point ranges: on the forked side stream, beside the passes on the caller's
  std::vector<WgLaunch> batches;      // chunk0 and the grid's x are set when a batch is enqueued for a chunk range
};

inline void add_pass(std::vector<WgPass>& out, WgKernel kern, bool side, const std::vector<WgTask>& sel, int64_t chunk_stride, float* partials) {
  if (sel.empty()) return;
  WgPass ps{kern, kern == WGK_TILES ? 64 : 256, 0, side, {}};
  if (kern == WGK_NARROW0 || kern == WGK_NARROW3) ps.lds_bytes = WGN_LDS_BYTES;
  else if (kern == WGK_BLOCKS2 || kern == WGK_BLOCKS3) ps.lds_bytes = W3P_LDS_BYTES;
  else if (kern != WGK_TILES) ps.lds_bytes = std::max(W3P_LDS_BYTES, WGN_LDS_BYTES);
  for (size_t off = 0; off < sel.size(); off += MAX_TASKS) {
    WgLaunch L{};
    L.n = (int32_t)std::min<size_t>(MAX_TASKS, sel.size() - off);
    std::copy_n(sel.begin() + off, L.n, L.t);
    L.chunk_stride = chunk_stride; L.partials = partials;
    ps.batches.push_back(L);
  }
  out.push_back(std::move(ps));
}

// Workgroups are dispatched task by task, so every list is ordered LONGEST FIRST.  The tasks of one variant, two-job tasks in front:
inline std::vector<WgTask> wg_by_jobs(const std::vector<WgTask>& tasks, int32_t variant) {
  std::vector<WgTask> sel;
  for (int nj = 2; nj >= 1; --nj)
    for (const WgTask& x : tasks) if (x.variant == variant && x.njobs == nj) sel.push_back(x);
  return sel;
}
// all narrow tiles in one launch: most MFMAs per point pair first; in split arithmetic the 128 x 128 tiles of blocks that are not
// 256 x 256 (the light-mask head) join in front
inline std::vector<WgTask> wg_narrow_order(const std::vector<WgTask>& tasks, bool with_tiles) {
  std::vector<WgTask> sel;
  if (with_tiles)
    for (const WgTask& x : tasks) if (x.variant == WG_TILE) sel.push_back(x);
  for (int32_t var : {WG_NARROW_B64, WG_NARROW_A, WG_NARROW_B32}) {
    const std::vector<WgTask> v = wg_by_jobs(tasks, var);
    sel.insert(sel.end(), v.begin(), v.end());
  }
  return sel;
}

// The passes of a step.  `ranged`: they run once per point range, all on the range's stream; in split arithmetic the narrow tasks and the
// 256 x 256 blocks are then ONE grid -- the two-job blocks, the one-job blocks, then the short narrow tasks, which fill the last round:
// i2sdf_weight_grads 0.95-0.96 -> 0.91-0.92 ms against narrow-first, and against two launches per range the 250 narrow workgroups no longer
// run alone in front of a kernel boundary (profiles/r6_launch_chain_ab.txt) -- whenever they fit one WgLaunch.  Otherwise, and without
// ranges, the narrow launch (there: on the side stream) is followed by the block launch (the other order: +0.02 ms, measured).
inline std::vector<WgPass> wgrad_passes(const i2sdf_plan* p, const i2sdf_train_buffers* tb, float* partials, bool ranged) {
  const std::vector<WgTask> tasks = wgrad_tasks(p, tb);
  const bool x3 = p->wgrad_bf16x3 != 0, two = p->wgrad_bf16x2 != 0;
  const std::vector<WgTask> narrow = wg_narrow_order(tasks, x3), blocks = wg_by_jobs(tasks, WG_BLOCK);
  std::vector<WgPass> out;
  if (ranged && x3 && !blocks.empty() && narrow.size() + blocks.size() <= (size_t)MAX_TASKS) {
    std::vector<WgTask> all = blocks;
    all.insert(all.end(), narrow.begin(), narrow.end());
    add_pass(out, two ? WGK_ALL2 : WGK_ALL3, false, all, p->wgrad_floats, partials);
  } else {
    add_pass(out, x3 ? WGK_NARROW3 : WGK_NARROW0, !ranged, narrow, p->wgrad_floats, partials);
    add_pass(out, two ? WGK_BLOCKS2 : WGK_BLOCKS3, false, blocks, p->wgrad_floats, partials);
  }
  if (!x3) add_pass(out, WGK_TILES, false, wg_by_jobs(tasks, WG_TILE), p->wgrad_floats, partials);
  return out;
}

// ---- split-M reduction + weight-norm backward: one row of the table per layer (wn_backward_kernel) -----------------
struct WnLayer {
  int64_t off_v, off_g, off_bias, blk_off, bias_blk_off;
  int32_t rows, cols, row0, ldo, rsplit, rbase, split, base1, valid0;
  float mult;
};
struct WnTab { WnLayer l[3 * I2SDF_MAX_LAYERS]; int32_t n; int32_t n_rows; };

inline void fill_wn(WnTab& tab, const i2sdf::NetPlan& np, int kind, int& row0) {
  const i2sdf_mlp_desc& d = np.d;
  const bool enc = d.multires > 0 || i2sdf::rgb_idr(d);        // a PE / side block in front of the hidden or feature columns (plan.h: side_dim)
  const int PED = i2sdf::side_dim(d), PEC8 = enc ? i2sdf::side_chunks(d) * 8 : 0;
  for (int l = 0; l < d.n_lin; ++l) {
    WnLayer& y = tab.l[tab.n++];
    y.off_v = d.off_v[l]; y.off_g = d.off_g[l]; y.off_bias = d.off_bias[l];
    y.rows = d.out_dim[l]; y.cols = d.in_dim[l]; y.row0 = row0; row0 += y.rows;
    y.ldo = np.wg_cols[l];
    y.blk_off = np.wgrad_off[l];
    y.bias_blk_off = bias_off(np, l);
    y.rsplit = 1 << 30; y.rbase = 0; y.split = 0; y.base1 = 0; y.valid0 = y.cols; y.mult = 1.0f;
    const bool last = l == d.n_lin - 1;
    if (kind == 0) {
      if (l == d.skip_layer) { y.valid0 = y.cols - PED; y.split = d.hidden; y.base1 = y.cols - PED; y.mult = 0.70710678118654752440f; }
      if (last) { y.rsplit = 1; y.rbase = 32; }
    } else if (kind == 1) {
      if (l == 0) { y.valid0 = PED; y.split = PEC8; y.base1 = PED; }
    }
  }
}
inline WnTab wgrad_wn_tab(const i2sdf_plan* p, const i2sdf_train_buffers* tb) {
  WnTab tab{};
  int row0 = 0;
  fill_wn(tab, p->sdf, 0, row0);
  if (wgrad_has_rgb(tb)) fill_wn(tab, p->rgb, 1, row0);
  if (wgrad_has_light(p, tb)) fill_wn(tab, p->light, 2, row0);
  tab.n_rows = row0;
  return tab;
}

}  // namespace
