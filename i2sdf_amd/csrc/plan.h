// Host-side plan: where every packed weight stream lives and how it is produced from the flat parameter
// buffer.  The kernels walk the streams linearly; the order of ops inside a stream is fixed by the
// kernel's own static structure (see mlp_fwd.hip), and build_sdf / build_rgb / build_light (plan.cpp) emit the same order.
// plan.cpp is the only place that knows the layout: while it emits a stream it records the positions a launch takes as
// marks, and a launch site turns two marks into (pointer, stage count) with i2sdf::span().
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/i2sdf.h"
#include "x3h.h"

namespace i2sdf {

enum SegType : int32_t { SEG_ZERO = 0, SEG_BIAS = 1, SEG_WFWD = 2, SEG_WBWD = 3, SEG_ROWVEC = 4, SEG_SCALAR = 5,
                         SEG_WFWD3 = 6 /* bf16x3 split planes, K-outer order (x3.h) */,
                         SEG_WBWD3 = 7 /* transposed weights, bf16x3 split planes, K-outer order */,
                         // the 16-point-wave family (x3h.h): 16-row tiles, 32-wide k-chunks
                         SEG_BIAS_H = 8, SEG_WFWD3H = 9, SEG_WBWD3H = 10, SEG_ROWVEC_H = 11,
                         SEG_WFWD2H = 12 /* as SEG_WFWD3H with the two leading split planes only (the sampler's bf16x2 passes) */ };

// Column map from a padded register-space index to a source column of weight_v:
//   kp <  split : kp < valid0 ? base0 + kp : none
//   kp >= split : (kp-split) < valid1 ? base1 + (kp-split) : none
struct ColMap { int32_t split, base0, valid0, base1, valid1; };

struct Seg {
  int64_t chunk0;        // first chunk of the segment inside the pack buffer
  int32_t nchunks;       // chunks covered (including its zero padding)
  int32_t type;
  int64_t off_v, off_bias;
  int32_t scale_off;     // index of row 0 of this layer in the row-scale array
  int32_t rows, cols;    // logical shape of weight_v
  int32_t row_off;       // first logical row this segment covers (e.g. 1 for the feature rows)
  int32_t nrows;         // rows covered from row_off (rows beyond are zero)
  int32_t NT, KC;        // tile geometry: WFWD chunk (nt,kc); WBWD chunk (kt,nc) with NT=#kt, KC=#nc
  int32_t used;          // chunks that carry data (rest is zero padding)
  ColMap cm;
  float mult;
};

// Positions inside a net's streams (chunk index in the pack buffer), recorded by plan.cpp while it emits them.  A stream the net's
// shape has no kernels for is empty: all its marks coincide.
enum Mark : int {
  FWD, FWD_HIDDEN_END, FWD_SDF_END, FWD_END,      // fp32 forward: hidden layers | output row vector(s) | feature rows (sdf net)
  REV, REV_CHAIN, REV_W0, REV_END,                // fp32 reverse, sdf net: [w_sdf][W_feat^T] | [w_sdf][W_{L-2}^T .. W_1^T] | [W_0^T]
  FWD3, FWD3_HIDDEN_END, FWD3_END,                // bf16x3 forward, 32-point waves (x3.h): hidden layers | sdf row
  REV3, REV3_CHAIN, REV3_W0, REV3_END,            // bf16x3 reverse, as REV (the skip layer's transposed op is two ops: hidden part, PE part)
  FWD3H, FWD3H_SDF_END, FWD3H_END,                // bf16x3 forward, 16-point waves (x3h.h): hidden layers, output row vector(s) | feature rows
  REV3H, REV3H_END,                               // bf16x3 reverse, 16-point waves (radiance net)
  FWD2H, FWD2H_END,                               // sdf net, hidden layers + sdf row with TWO split planes (I2SDF_OPT_SAMPLER_BF16X2)
  N_MARKS
};
// What a launch walks: from one mark to another, in LDS stages of `stage_chunks` chunks (SC: 32-point waves, SCH: 16-point waves).
struct SpanId { Mark from, to; int stage_chunks; };
constexpr SpanId SPAN_FWD_HIDDEN{FWD, FWD_HIDDEN_END, SC};        // backward sweep 1
constexpr SpanId SPAN_FWD_SDF{FWD, FWD_SDF_END, SC};              // sdf-only forward
constexpr SpanId SPAN_FWD{FWD, FWD_END, SC};
constexpr SpanId SPAN_REV_SWEEP2{REV, REV_W0, SC};                // backward sweep 2 stops in front of W_0^T: the points carry no gradient
constexpr SpanId SPAN_REV_CHAIN{REV_CHAIN, REV_END, SC};          // the d sdf/dx chain starts at the second w_sdf
constexpr SpanId SPAN_REV{REV, REV_END, SC};                      // radiance net, light head: the whole stream
constexpr SpanId SPAN_FWD3_HIDDEN{FWD3, FWD3_HIDDEN_END, SC};
constexpr SpanId SPAN_FWD3{FWD3, FWD3_END, SC};
constexpr SpanId SPAN_REV3_SWEEP2{REV3, REV3_W0, SC};
constexpr SpanId SPAN_REV3_CHAIN{REV3_CHAIN, REV3_END, SC};
constexpr SpanId SPAN_FWD3H_SDF{FWD3H, FWD3H_SDF_END, SCH};
constexpr SpanId SPAN_FWD3H{FWD3H, FWD3H_END, SCH};
constexpr SpanId SPAN_REV3H{REV3H, REV3H_END, SCH};
constexpr SpanId SPAN_FWD2H{FWD2H, FWD2H_END, SCH};

// Radiance net: the columns of layer 0 in front of the feature columns are the per-point "side row" -- 'nerf': PE(view); 'idr':
// [x | PE(view) | normal] (include/i2sdf.h: I2SDF_RGB_MODE_*), one contiguous block of lin0.weight_v in either mode
// side_dim: THE width of a net's encoded input in front of the hidden / feature columns of its layer 0 -- PE(x) of the SDF net, the side row
// of the radiance net, d_in of a net without encoding (plan.cpp, wgrad.hip and the launch sites all take it from here)
// reserved = mode | act << 8 | embed << 24 (include/i2sdf.h): the mode in bits 0..7, the output activation I2SDF_RGB_ACT_* in bits 8..15, the view
// embedder I2SDF_RGB_EMBED_* in bits 24..27 (multires then carries the SH degree / the Fourier channel count)
inline int rgb_mode(const i2sdf_mlp_desc& d) { return d.reserved & 0xff; }
inline int rgb_act(const i2sdf_mlp_desc& d) { return (d.reserved >> 8) & 0xff; }
inline int rgb_embed(const i2sdf_mlp_desc& d) { return (d.reserved >> 24) & 0xf; }
inline bool rgb_idr(const i2sdf_mlp_desc& d) { return rgb_mode(d) == I2SDF_RGB_MODE_IDR; }
// width e of the embedded view direction E(v) of a radiance net with an SH / Fourier embedder
inline int embed_dim(const i2sdf_mlp_desc& d) { return rgb_embed(d) == I2SDF_RGB_EMBED_SH ? d.multires * d.multires : 2 * d.multires + 3; }
inline int side_dim(const i2sdf_mlp_desc& d) {
  if (rgb_embed(d) != I2SDF_RGB_EMBED_POSITIONAL) return embed_dim(d) + (rgb_idr(d) ? 6 : 0);      // [E(v)] / [x | E(v) | normal]
  const int raw = rgb_idr(d) ? 3 : d.d_in;          // 'idr': only the view direction (3 of the 9 raw inputs) is encoded
  return (d.multires > 0 ? raw + 2 * raw * d.multires : raw) + (rgb_idr(d) ? 6 : 0);
}
// 8-column chunks the side row occupies in the padded spaces (fp32 streams, saved row, weight-gradient block).  An SH / Fourier row keeps
// the positional row's 32 ('nerf') / 40 ('idr') columns whatever its own width: one kernel instantiation and one set of shapes for all of them
inline int side_chunks(const i2sdf_mlp_desc& d) {
  if (rgb_embed(d) != I2SDF_RGB_EMBED_POSITIONAL) return rgb_idr(d) ? 5 : 4;
  return (side_dim(d) + 7) / 8;
}

struct NetPlan {
  i2sdf_mlp_desc d;
  int32_t scale_off[I2SDF_MAX_LAYERS];
  int64_t mark[N_MARKS] = {};
  int64_t wgrad_off[I2SDF_MAX_LAYERS];         // offset (floats) of layer l's [rowsP x colsP] block in the wgrad buffer
  int32_t wg_rows[I2SDF_MAX_LAYERS], wg_cols[I2SDF_MAX_LAYERS];   // padded shape of that block
};

}  // namespace i2sdf

struct i2sdf_plan {
  i2sdf_net_desc desc;
  i2sdf::NetPlan sdf, rgb, light;
  std::vector<i2sdf::Seg> segs;
  i2sdf::Seg* d_segs = nullptr;      // device copy
  int32_t n_segs = 0;
  int32_t n_scale = 0;               // total rows over all layers of all nets
  int64_t scale_floats = 0;          // region [0, scale_floats) of the pack buffer holds g/||v||
  int64_t total_chunks = 0;          // chunks after the scale region (+1 stage of slack for the DMA look-ahead)
  int64_t wgrad_floats = 0;
  int32_t H = 0, F = 0;              // sdf hidden width / feature size
  int32_t n_cu = 256;                // compute units of the device the plan was created on (hipDeviceProp; 256 on MI355X)
  int32_t rgb_bf16x3 = 0;            // I2SDF_OPT_RGB_BF16X3: radiance forward / backward (full workgroups) in bf16x3 split arithmetic
  int32_t sdf_bwd_bf16x3 = 0;        // I2SDF_OPT_SDF_BWD_BF16X3: SDF backward sweeps (full workgroups) in bf16x3 split arithmetic
  int32_t train_fwd_bf16x3 = 0;      // I2SDF_OPT_TRAIN_FWD_BF16X3: SDF forward + d sdf/dx kernel in bf16x3 split arithmetic
  int32_t wgrad_bf16x3 = 0;          // I2SDF_OPT_WGRAD_BF16X3: full 256x256 weight-gradient blocks in bf16x3 split arithmetic
  int32_t sdf_fwd_bf16x3 = 0;        // i2sdf_plan_set_option(I2SDF_OPT_SDF_FWD_BF16X3): sdf-only forward in bf16x3 split arithmetic
  int32_t sampler_bf16x2 = 0;        // I2SDF_OPT_SAMPLER_BF16X2: the sampler's sdf-only passes with two split planes / three products
  i2sdf_exchange exchange{nullptr, nullptr};   // i2sdf_plan_set_exchange: small data-parallel exchanges (copied)
  int32_t dp_flags = 0;              // I2SDF_DP_GLOBAL_SAMPLER
  int32_t wgrad_bf16x2 = 0;          // I2SDF_OPT_WGRAD_BF16X2: 256x256 weight-gradient blocks with two split planes / three products
  int32_t blocked_saves = 0;         // I2SDF_OPT_BLOCKED_SAVES: saved tensors of the bf16x3 full workgroups in the blocked layout (mlp_common.h)
  int32_t saves24 = 0;               // I2SDF_OPT_SAVES24: abars / gus / gas as packed 24-bit records (mlp_common.h: sdf_saves24 says when it takes effect)
  int32_t tail_overlap = 0;          // I2SDF_OPT_TAIL_OVERLAP: split-K tail workgroups on a side stream, concurrent with the full ones
  // side stream + fork/join events of the tail overlap, created on first use (entry points take a const plan)
  mutable hipStream_t side = nullptr;
  mutable hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // I2SDF_OPT_PARTS (see PartRun below): number of point ranges the per-point entry points are cut into (0 / 1 = off)
  int32_t parts = 0;
  mutable hipStream_t part_st[I2SDF_MAX_PARTS - 1] = {nullptr, nullptr, nullptr};
  mutable hipEvent_t part_ev[I2SDF_MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};   // [0] fork event, [q] join event of part q
  mutable int32_t chain_active = 0;          // between i2sdf_chain_begin and i2sdf_chain_end
  // i2sdf_plan_set_view_embed: B of a Fourier view embedder, row r at view_B[12 r ..] (zero beyond the channel count), passed to the
  // radiance forward kernels by value (mlp_args.h: RgbEmbedFwdArgs)
  float view_B[3 * I2SDF_RGB_EMBED_MAX_CHANNELS] = {};
  int32_t view_B_set = 0;
  mutable int64_t chain_M = 0;               // the point count the active chain's ranges were cut from
};

// An entry point's refusal with a reason: the text goes where i2sdf_last_hip_error() finds it; returns I2SDF_EINVAL (plan.cpp)
int i2sdf_refuse(const char* why);
// hipSuccess -> I2SDF_OK; anything else -> I2SDF_EHIP, with `what` and the error's text where i2sdf_last_hip_error() finds them (plan.cpp)
int i2sdf_hip_check(hipError_t e, const char* what);

// ---- spans of the weight streams ----------------------------------------------------------------------------------
// What a kernel takes: where its weight stream starts and how many LDS stages it walks.  n_stages == 0: the span was refused -- empty
// (the net's shape has no such stream) or not a whole number of stages (a layout mistake in plan.cpp).  The entry point then returns
// I2SDF_EINVAL instead of launching a kernel whose DMA look-ahead would run past, or stop short of, the ops it consumes.
namespace i2sdf {
struct Span { const float* w = nullptr; int n_stages = 0; };
inline int64_t span_chunks(const NetPlan& np, SpanId id) { return np.mark[id.to] - np.mark[id.from]; }
inline Span span(const i2sdf_plan* p, const float* packed, const NetPlan& np, SpanId id) {
  const int64_t n = span_chunks(np, id);
  if (n <= 0 || n % id.stage_chunks) return Span{};
  return Span{packed + p->scale_floats + np.mark[id.from] * CHUNK_FLOATS, (int)(n / id.stage_chunks)};
}
}  // namespace i2sdf

// ---- point ranges ("parts") ---------------------------------------------------------------------------------------
// A launch over M points of 128-point workgroups on 256 CUs runs ceil(M/128/256) rounds, the last one partly empty, and the
// next kernel of the chain (forward -> d sdf/dx -> radiance -> ... ) cannot start before it has drained.  With I2SDF_OPT_PARTS
// = n the point batch is cut into n ranges at multiples of the weight-gradient chunk (1024 points); range q runs its whole
// chain of kernels on its own stream (range 0 on the caller's, the others on streams owned by the plan), so the ranges drift
// apart and the partly empty last round of one kernel is filled by workgroups of another range's next kernel.  No split-K tail
// workgroups in this mode: every point goes through the bf16x3 kernels, every saved tensor is blocked throughout.
//   parts_begin : fills `pr` with the ranges of a batch of M points and the stream of each.  Outside a chain it forks the side
//                 streams from `st` (they see everything enqueued on `st` so far); inside a chain (i2sdf_chain_begin) the streams
//                 are already forked and stay un-joined between entry points.
//   parts_end   : outside a chain joins the side streams back into `st` (the entry point returns stream-ordered on `st`).
struct PartRun {
  int n = 1;
  hipStream_t st[I2SDF_MAX_PARTS];
  int64_t lo[I2SDF_MAX_PARTS], hi[I2SDF_MAX_PARTS];     // point range of part q (lo a multiple of 1024; hi capped by M)
  bool own = false;                                      // this call forked, this call joins
};
bool i2sdf_parts_begin(const i2sdf_plan* p, hipStream_t st, int64_t M, PartRun* pr);
void i2sdf_parts_end(const i2sdf_plan* p, hipStream_t st, PartRun* pr);
void i2sdf_parts_join_all(const i2sdf_plan* p, hipStream_t st);        // `st` waits for every side stream (also inside a chain)
void i2sdf_parts_fence(const i2sdf_plan* p, hipStream_t st);           // every side stream waits for what is enqueued on `st`
// points per split-M chunk of the weight-gradient GEMMs == alignment of the point ranges (a chunk never straddles two ranges)
#ifndef I2SDF_WG_CH
#define I2SDF_WG_CH 2048      // (round 4: 2048 instead of 1024 halves the per-chunk partial sums -- wn_backward reads 220 instead of 440 MB -- step -0.04 ms)
#endif
inline bool i2sdf_parts_on(const i2sdf_plan* p) { return p->parts >= 2; }
// An entry point that does NOT cut its batch into ranges (its kernel family is not on the ranged path, e.g. rgb_bf16x3 off while the SDF
// flags are on) called inside a chain: the side streams still hold un-joined work of the previous entry point, and the next one will run
// on them again.  The guard joins every range into `st` before the entry point's launches and fences the side streams behind them.
struct ChainGuard {
  const i2sdf_plan* p; hipStream_t st; bool on;
  ChainGuard(const i2sdf_plan* p_, hipStream_t st_, bool ranged) : p(p_), st(st_), on(!ranged && p_->chain_active != 0) {
    if (on) i2sdf_parts_join_all(p, st);
  }
  ~ChainGuard() { if (on) i2sdf_parts_fence(p, st); }
};

// Fork: returns the stream the split-K tail of an entry point should be launched on -- the plan's side stream, ordered after
// everything already enqueued on `st`, or `st` itself when the overlap is off.  Join: `st` waits for the side stream.
// Launch order at the call sites: fork, tail (few long workgroups), full workgroups on `st`, join.
hipStream_t i2sdf_tail_fork(const i2sdf_plan* p, hipStream_t st);
void i2sdf_tail_join(const i2sdf_plan* p, hipStream_t st, hipStream_t side);

// Split of a launch over M points into full rounds of 128-point workgroups (one per CU) and a short tail that is run by
// the split-K kernels (ksplit.h): returns the number of points of the bulk part (0 = no split).
inline int64_t split_bulk_points(int64_t M, int n_cu) {
  const int64_t n_wg = (M + i2sdf::PTS_PER_WG - 1) / i2sdf::PTS_PER_WG;
  const int64_t full = (n_wg / n_cu) * n_cu, rem = n_wg - full;
  if (full == 0 || rem == 0 || rem * 4 > n_cu) return 0;      // nothing to gain, or the tail would not fit one round
  // the bulk is also where the blocked layout of the saved tensors ends, and the weight-gradient kernels pick an operand's layout once
  // per split-M chunk: a chunk must not straddle that boundary (n_cu * 128 is a multiple of the 2048-point chunk only when n_cu % 16 == 0
  // -- true for the 256 CUs of an MI355X, not for every partition of it).  No split then: every point goes through the full
  // workgroups, every saved tensor is blocked throughout.
  if ((full * i2sdf::PTS_PER_WG) % I2SDF_WG_CH != 0) return 0;
  return full * i2sdf::PTS_PER_WG;
}

// The three shapes of a per-point entry point's launches, with
//   full(stream, first_workgroup, n_workgroups, M_visible) : 128-point workgroups; points >= M_visible are masked
//   tail(stream, first_point)                              : the split-K kernel over the points from first_point on
// ranged    : one `full` per non-empty point range on the range's stream (the caller says whether its kernel family is on the ranged path);
// bulk+tail : when `may_split` (the entry point's own condition) and split_bulk_points() finds a partial last round.  TAIL_FORKED: tail first on
//             the side stream of i2sdf_tail_fork, full workgroups on `st`, join (the SDF entry points).  TAIL_BEHIND: full workgroups, then the
//             tail behind them on `st` (the radiance entry points: that tail is 32 short workgroups, the fork/join costs more than the
//             overlap gains -- measured);
// whole     : one `full` over the batch.
enum TailOrder { TAIL_FORKED, TAIL_BEHIND };
template <class Full, class Tail>
inline void i2sdf_dispatch_points(const i2sdf_plan* p, hipStream_t st, int64_t M, bool ranged, bool may_split, TailOrder order, Full full, Tail tail) {
  constexpr int64_t WG = i2sdf::PTS_PER_WG;
  if (ranged) {
    PartRun pr;
    i2sdf_parts_begin(p, st, M, &pr);
    for (int q = 0; q < pr.n; ++q)
      if (pr.hi[q] > pr.lo[q]) full(pr.st[q], (int)(pr.lo[q] / WG), (unsigned)((pr.hi[q] - pr.lo[q] + WG - 1) / WG), M);
    i2sdf_parts_end(p, st, &pr);
    return;
  }
  const int64_t bulk = may_split ? split_bulk_points(M, p->n_cu) : 0;
  if (bulk == 0) {
    full(st, 0, (unsigned)((M + WG - 1) / WG), M);
  } else if (order == TAIL_FORKED) {
    hipStream_t ts = i2sdf_tail_fork(p, st);
    tail(ts, bulk);
    full(st, 0, (unsigned)(bulk / WG), bulk);
    i2sdf_tail_join(p, st, ts);
  } else {
    full(st, 0, (unsigned)(bulk / WG), bulk);
    tail(st, bulk);
  }
}
