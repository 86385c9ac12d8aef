// Plan construction (host) + the C-ABI entry points that do not launch MLP kernels.
#include <hip/hip_runtime.h>
#include <string.h>
#include <initializer_list>
#include <string>
#include "plan.h"
#include <stdlib.h>

using namespace i2sdf;

static thread_local std::string g_hip_err;

int i2sdf_hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return I2SDF_OK;
  g_hip_err = std::string(what) + ": " + hipGetErrorString(e);
  return I2SDF_EHIP;
}

int i2sdf_refuse(const char* why) {
  g_hip_err = why;
  return I2SDF_EINVAL;
}

extern "C" int i2sdf_version(void) { return I2SDF_VERSION; }
extern "C" const char* i2sdf_last_hip_error(void) { return g_hip_err.c_str(); }
extern "C" const char* i2sdf_strerror(int code) {
  switch (code) {
    case I2SDF_OK: return "ok";
    case I2SDF_EINVAL: return "invalid argument or unsupported network shape";
    case I2SDF_EHIP: return "HIP runtime error";
    case I2SDF_ESPHERE: return "ray misses the scene bounding sphere";
    case I2SDF_EWORKSPACE: return "workspace too small";
    case I2SDF_ECOMM: return "RCCL error";
    default: return "unknown error";
  }
}

namespace {

constexpr int32_t HUGE_SPLIT = 1 << 30;
constexpr float RS2 = 0.70710678118654752440f;      // 1/sqrt(2) of the skip concatenation

struct Builder {
  std::vector<Seg>& segs;
  int64_t chunk;     // running chunk cursor
  void add(Seg s) { s.chunk0 = chunk; chunk += s.nchunks; segs.push_back(s); }
  void pad_to_stage() {
    int64_t r = chunk % SC;
    if (r) { Seg z{}; z.type = SEG_ZERO; z.nchunks = (int32_t)(SC - r); add(z); }
  }
};

Seg base_seg(const NetPlan& np, int l, int type) {
  Seg s{};
  s.type = type;
  s.off_v = np.d.off_v[l]; s.off_bias = np.d.off_bias[l];
  s.scale_off = np.scale_off[l];
  s.rows = np.d.out_dim[l]; s.cols = np.d.in_dim[l];
  s.row_off = 0; s.nrows = s.rows;
  s.mult = 1.0f;
  s.cm = ColMap{HUGE_SPLIT, 0, s.cols, 0, 0};
  return s;
}

int pe_dim(const i2sdf_mlp_desc& d) { return side_dim(d); }      // (plan.h: one definition for every caller)
int pe_chunks(const i2sdf_mlp_desc& d) { return side_chunks(d); }

ColMap cols(int n) { return ColMap{HUGE_SPLIT, 0, n, 0, 0}; }      // the first n columns, no split

// A kernel family's forward ops as data: the segment types its kernels read, its tile geometry, its split planes.
struct Family {
  int32_t bias_type, w_type, rowvec_type;
  int tile_rows;        // rows of an output tile
  int k_width;          // columns of a k-chunk of a dense op
  int rv_width;         // columns of a chunk of a row-vector op
  int bias_chunks;      // bias chunks per output tile
  int planes;           // chunks per (tile, k-chunk): 1 = fp32, 3 / 2 = bf16 split planes, K-outer order
  bool fold_skip;       // the 1/sqrt(2) of the skip concatenation is folded into that layer's weights (fp32: the kernel applies it)
};
constexpr Family FP32{SEG_BIAS, SEG_WFWD, SEG_ROWVEC, 32, 8, 8, 4, 1, false};
constexpr Family X3{SEG_BIAS, SEG_WFWD3, SEG_ROWVEC, 32, 16, 8, 4, 3, true};             // x3.h: 32-point waves
constexpr Family X3H{SEG_BIAS_H, SEG_WFWD3H, SEG_ROWVEC_H, 16, 32, 16, 1, 3, true};      // x3h.h: 16-point waves
constexpr Family X2H{SEG_BIAS_H, SEG_WFWD2H, SEG_ROWVEC_H, 16, 32, 16, 1, 2, true};      // the same with the two leading planes only (dense_x3h<..., PL = 2>)

// dense forward op: [NT * bias_chunks bias chunks][NT * KC * planes weight chunks] padded to stages
void emit_dense(Builder& b, const NetPlan& np, int l, const Family& f, int NT, int KC, ColMap cm, float mult, int row_off, int nrows) {
  Seg sb = base_seg(np, l, f.bias_type);
  sb.NT = NT; sb.KC = f.bias_chunks; sb.nchunks = sb.used = NT * f.bias_chunks; sb.row_off = row_off; sb.nrows = nrows;
  b.add(sb);
  Seg sw = base_seg(np, l, f.w_type);
  sw.NT = NT; sw.KC = KC; sw.used = NT * KC * f.planes; sw.cm = cm; sw.mult = mult; sw.row_off = row_off; sw.nrows = nrows;
  sw.nchunks = (f.w_type == SEG_WFWD ? op_chunks(NT, KC) : f.w_type == SEG_WFWD3 ? x3_op_chunks(NT, KC) : x3h_op_chunks(NT, KC, f.planes)) - sb.nchunks;
  b.add(sw);
}
// transposed op (no bias) of type SEG_WBWD / SEG_WBWD3 / SEG_WBWD3H: KT tiles over the layer's input space, reduction over its output rows in KC chunks
void emit_dense_bwd(Builder& b, const NetPlan& np, int l, int type, int KT, int KC, ColMap cm, int row_off, int nrows, float mult = 1.0f) {
  Seg sw = base_seg(np, l, type);
  sw.NT = KT; sw.KC = KC; sw.used = KT * KC * (type == SEG_WBWD ? 1 : 3); sw.cm = cm; sw.mult = mult; sw.row_off = row_off; sw.nrows = nrows;
  sw.nchunks = type == SEG_WBWD ? bwd_op_chunks(KT, KC) : type == SEG_WBWD3 ? x3_bwd_chunks(KT, KC) : x3h_bwd_chunks(KT, KC);
  b.add(sw);
}
// the first nrows rows of layer l as row vectors over the net's hidden width, then one scalar chunk
void emit_rowvec(Builder& b, const NetPlan& np, int l, const Family& f, int nrows) {
  const int KC = np.d.hidden / f.rv_width;
  Seg sw = base_seg(np, l, f.rowvec_type);
  sw.NT = nrows; sw.KC = KC; sw.used = nrows * KC; sw.nchunks = nrows * KC; sw.cm = cols(np.d.hidden); sw.nrows = nrows;
  b.add(sw);
  Seg sc = base_seg(np, l, SEG_SCALAR);
  sc.nchunks = (f.rowvec_type == SEG_ROWVEC ? rowvec_chunks(KC, nrows) : rowvec_h_chunks(KC, nrows)) - nrows * KC; sc.used = 1; sc.nrows = nrows;
  b.add(sc);
}
// the hidden layers of the SDF net, bottom-up: layer 0 reduces over PE(x), the skip layer over [h | PE(x)] (both parts padded to k-chunks)
void emit_sdf_hidden(Builder& b, const NetPlan& np, const Family& f) {
  const i2sdf_mlp_desc& d = np.d;
  const int H = d.hidden, PED = pe_dim(d), PEK = cdiv(PED, f.k_width);
  for (int l = 0; l < d.n_lin - 1; ++l) {
    ColMap cm = cols(d.in_dim[l]);
    int KC = (l == 0) ? PEK : H / f.k_width;
    float mult = 1.0f;
    if (l == d.skip_layer) {
      cm = ColMap{H, 0, d.in_dim[l] - PED, d.in_dim[l] - PED, PED}; KC += PEK;
      if (f.fold_skip) mult = RS2;
    }
    emit_dense(b, np, l, f, H / f.tile_rows, KC, cm, mult, 0, d.out_dim[l]);
  }
}

int check_mlp(const i2sdf_mlp_desc& d) {
  if (d.n_lin < 2 || d.n_lin > I2SDF_MAX_LAYERS) return I2SDF_EINVAL;
  if (d.hidden % 32 || d.hidden < 32 || d.hidden > 256) return I2SDF_EINVAL;
  return I2SDF_OK;
}

// records the builder's cursor under every mark of `ms` (a stream the shape has no kernels for keeps all its marks on one position)
void mark_here(NetPlan& np, const Builder& b, std::initializer_list<Mark> ms) {
  for (Mark k : ms) np.mark[k] = b.chunk;
}

// ---- SDF net (ImplicitNetwork with positional encoding) -------------------------------------
int build_sdf(i2sdf_plan* p, Builder& b) {
  NetPlan& np = p->sdf;
  const i2sdf_mlp_desc& d = np.d;
  const int L = d.n_lin, H = d.hidden, PEC = pe_chunks(d), PED = pe_dim(d);
  const int F = d.d_out - 1;
  if (check_mlp(d)) return I2SDF_EINVAL;
  if (d.multires <= 0 || d.d_in != 3 || d.in0 != PED) return I2SDF_EINVAL;
  if (F < 0 || F % 32 || F > 256) return I2SDF_EINVAL;
  if (d.skip_layer == 0 || d.skip_layer >= L - 1) return I2SDF_EINVAL;
  for (int l = 0; l < L - 1; ++l) {
    const int want_out = (l + 1 == d.skip_layer) ? H - PED : H;
    const int want_in = (l == 0) ? PED : H;
    if (d.out_dim[l] != want_out || d.in_dim[l] != want_in) return I2SDF_EINVAL;
  }
  if (d.in_dim[L - 1] != H) return I2SDF_EINVAL;
  p->H = H; p->F = F;
  const bool even_tiles = (H / 32) % 2 == 0, wide = H == 256 && F == 256;      // shapes the bf16x3 kernels of x3.h / x3h.h are built for
  const int PT = cdiv(PEC * 8, 32);                                            // 32-row tiles of the padded PE space
  // forward stream: hidden layers, sdf row, feature rows
  mark_here(np, b, {FWD});
  emit_sdf_hidden(b, np, FP32);
  mark_here(np, b, {FWD_HIDDEN_END});
  emit_rowvec(b, np, L - 1, FP32, 1);
  mark_here(np, b, {FWD_SDF_END});
  if (F > 0) emit_dense(b, np, L - 1, FP32, F / 32, H / 8, cols(H), 1.0f, 1, F);
  mark_here(np, b, {FWD_END});
  // reverse (transposed) stream: [w_sdf][Wfeat^T][w_sdf][W_{L-2}^T] ... [W_0^T]
  //   backward sweep 2 starts at REV (needs w_sdf before the feature op so that the op's epilogue can use it), skips the
  //   second copy and stops in front of W_0^T; the d sdf/dx chain starts at REV_CHAIN.
  mark_here(np, b, {REV});
  emit_rowvec(b, np, L - 1, FP32, 1);
  if (F > 0) emit_dense_bwd(b, np, L - 1, SEG_WBWD, H / 32, F / 8, cols(H), 1, F);
  mark_here(np, b, {REV_CHAIN});
  emit_rowvec(b, np, L - 1, FP32, 1);
  for (int l = L - 2; l >= 0; --l) {
    ColMap cm = cols(d.in_dim[l]);
    int KT = (l == 0) ? PT : H / 32;
    if (l == d.skip_layer) { cm = ColMap{H, 0, d.in_dim[l] - PED, d.in_dim[l] - PED, PED}; KT += PT; }
    if (l == 0) mark_here(np, b, {REV_W0});
    emit_dense_bwd(b, np, l, SEG_WBWD, KT, H / 8, cm, 0, d.out_dim[l]);
  }
  mark_here(np, b, {REV_END});
  // bf16x3 forward stream (backward sweep 1; sdf-only queries of 64-wide nets): hidden layers K-outer, then the fp32 sdf row
  mark_here(np, b, {FWD3, FWD3_HIDDEN_END, FWD3_END});
  if (even_tiles) {
    emit_sdf_hidden(b, np, X3);
    mark_here(np, b, {FWD3_HIDDEN_END});
    emit_rowvec(b, np, L - 1, X3, 1);
    mark_here(np, b, {FWD3_END});
  }
  // bf16x3 reverse stream, laid out as the fp32 one; skip factor folded into the weights
  mark_here(np, b, {REV3, REV3_CHAIN, REV3_W0, REV3_END});
  if (even_tiles) {
    emit_rowvec(b, np, L - 1, X3, 1);
    if (F > 0 && F % 16 == 0) emit_dense_bwd(b, np, L - 1, SEG_WBWD3, H / 32, F / 16, cols(H), 1, F);
    mark_here(np, b, {REV3_CHAIN});
    emit_rowvec(b, np, L - 1, X3, 1);
    for (int l = L - 2; l >= 0; --l) {
      if (l == 0) mark_here(np, b, {REV3_W0});
      // the skip layer's transposed op is emitted as two ops over the same reduction: hidden part, then PE part
      if (l == d.skip_layer) {
        emit_dense_bwd(b, np, l, SEG_WBWD3, H / 32, H / 16, cols(d.in_dim[l] - PED), 0, d.out_dim[l], RS2);
        emit_dense_bwd(b, np, l, SEG_WBWD3, PT, H / 16, ColMap{HUGE_SPLIT, d.in_dim[l] - PED, PED, 0, 0}, 0, d.out_dim[l], RS2);
      } else {
        emit_dense_bwd(b, np, l, SEG_WBWD3, (l == 0) ? PT : H / 32, H / 16, cols(d.in_dim[l]), 0, d.out_dim[l]);
      }
    }
    mark_here(np, b, {REV3_END});
  }
  // the forward stream for the 16-point-wave kernels (x3h.h): same ops in the same order, with the feature rows.  (No reverse stream of this
  // family for the SDF net: its d sdf/dx chain and sweeps run on 32-point waves.)
  mark_here(np, b, {FWD3H, FWD3H_SDF_END, FWD3H_END});
  if (wide) {
    emit_sdf_hidden(b, np, X3H);
    emit_rowvec(b, np, L - 1, X3H, 1);
    mark_here(np, b, {FWD3H_SDF_END});
    emit_dense(b, np, L - 1, X3H, F / 16, H / 32, cols(H), 1.0f, 1, F);          // feature rows
    mark_here(np, b, {FWD3H_END});
  }
  // the sampler's passes with two split planes (I2SDF_OPT_SAMPLER_BF16X2): hidden layers + the fp32 sdf row, 2/3 of the bytes and stages
  mark_here(np, b, {FWD2H, FWD2H_END});
  if (wide) {
    emit_sdf_hidden(b, np, X2H);
    emit_rowvec(b, np, L - 1, X2H, 1);
    mark_here(np, b, {FWD2H_END});
  }
  return I2SDF_OK;
}

// ---- radiance net: input [side row | feature]; side row = PE(view) ('nerf') or [x | PE(view) | normal] ('idr'; plan.h: side_dim) ----
int build_rgb(i2sdf_plan* p, Builder& b) {
  NetPlan& np = p->rgb;
  const i2sdf_mlp_desc& d = np.d;
  const bool idr = rgb_idr(d);
  const int L = d.n_lin, H = d.hidden, PED = pe_dim(d), PEC = pe_chunks(d), F = p->F;
  if (check_mlp(d)) return I2SDF_EINVAL;
  if ((rgb_mode(d) != I2SDF_RGB_MODE_NERF && !idr) || (idr && d.d_in != 9)) return I2SDF_EINVAL;
  if (rgb_act(d) > I2SDF_RGB_ACT_SOFTPLUS || (d.reserved & 0xf0ff0000) || rgb_embed(d) > I2SDF_RGB_EMBED_FOURIER) return I2SDF_EINVAL;      // (i2sdf_plan_create says why)
  // the reverse product of layer 0: the feature rows of W_0^T; 'idr' adds one more tile behind them that holds the three normal rows
  const ColMap rev0 = idr ? ColMap{F, PED, F, PED - 3, 3} : ColMap{HUGE_SPLIT, PED, F, 0, 0};
  if (d.skip_layer >= 0 || d.d_out != 3 || (d.multires <= 0 && !idr) || d.in0 != PED + F || F <= 0) return I2SDF_EINVAL;
  for (int l = 0; l < L - 1; ++l)
    if (d.out_dim[l] != H || d.in_dim[l] != (l == 0 ? PED + F : H)) return I2SDF_EINVAL;
  const bool wide = H == 256 && F == 256 && L >= 3;      // (the radiance net's bf16x3 kernels all run on 16-point waves)
  mark_here(np, b, {FWD});
  emit_dense(b, np, 0, FP32, H / 32, PEC + F / 8, ColMap{PEC * 8, 0, PED, PED, F}, 1.0f, 0, H);
  for (int l = 1; l < L - 1; ++l) emit_dense(b, np, l, FP32, H / 32, H / 8, cols(H), 1.0f, 0, H);
  emit_rowvec(b, np, L - 1, FP32, 3);
  mark_here(np, b, {FWD_END, REV});
  emit_rowvec(b, np, L - 1, FP32, 3);
  for (int l = L - 2; l >= 1; --l) emit_dense_bwd(b, np, l, SEG_WBWD, H / 32, H / 8, cols(H), 0, H);
  emit_dense_bwd(b, np, 0, SEG_WBWD, F / 32 + (idr ? 1 : 0), H / 8, rev0, 0, H);   // feature columns only ('idr': + the normal columns)
  mark_here(np, b, {REV_END});
  // bf16x3 streams, 16-point-wave family (x3h.h): layer 0 reduces over [PE(view) padded to 32-chunks | feature]
  mark_here(np, b, {FWD3H, FWD3H_END, REV3H, REV3H_END});
  if (wide) {
    const int PV32 = cdiv(PEC * 8, 32);
    emit_dense(b, np, 0, X3H, H / 16, PV32 + F / 32, ColMap{PV32 * 32, 0, PED, PED, F}, 1.0f, 0, H);
    for (int l = 1; l < L - 1; ++l) emit_dense(b, np, l, X3H, H / 16, H / 32, cols(H), 1.0f, 0, H);
    emit_rowvec(b, np, L - 1, X3H, 3);
    mark_here(np, b, {FWD3H_END, REV3H});
    emit_rowvec(b, np, L - 1, X3H, 3);
    for (int l = L - 2; l >= 1; --l) emit_dense_bwd(b, np, l, SEG_WBWD3H, H / 16, H / 32, cols(H), 0, H);
    emit_dense_bwd(b, np, 0, SEG_WBWD3H, F / 16 + (idr ? 2 : 0), H / 32, rev0, 0, H);      // (tiles come in pairs)
    mark_here(np, b, {REV3H_END});
  }
  return I2SDF_OK;
}

// ---- light-mask head: relu(feature) -> [hidden] softplus100 -> 1, sigmoid -----------------------
int build_light(i2sdf_plan* p, Builder& b) {
  NetPlan& np = p->light;
  const i2sdf_mlp_desc& d = np.d;
  if (d.n_lin == 0) return I2SDF_OK;
  const int H = d.hidden, F = p->F;
  if (d.n_lin != 2 || H % 32 || H > 256 || d.d_out != 1 || d.in0 != F || d.multires != 0) return I2SDF_EINVAL;
  if (d.out_dim[0] != H || d.in_dim[0] != F || d.in_dim[1] != H) return I2SDF_EINVAL;
  mark_here(np, b, {FWD});
  emit_dense(b, np, 0, FP32, H / 32, F / 8, cols(F), 1.0f, 0, H);
  emit_rowvec(b, np, 1, FP32, 1);
  mark_here(np, b, {FWD_END, REV});
  emit_rowvec(b, np, 1, FP32, 1);
  mark_here(np, b, {REV_END});
  // the forward on 16-point waves (mlp_x3h.hip: light_fwd3h_kernel), shapes of the shipped config only
  mark_here(np, b, {FWD3H, FWD3H_END});
  if (H == 128 && F == 256) {
    emit_dense(b, np, 0, X3H, H / 16, F / 32, cols(F), 1.0f, 0, H);
    emit_rowvec(b, np, 1, X3H, 1);
    mark_here(np, b, {FWD3H_END});
  }
  return I2SDF_OK;
}

// kind: 0 = sdf net, 1 = radiance net, 2 = light head
void assign_scales_and_wgrad(i2sdf_plan* p, NetPlan& np, int kind) {
  const i2sdf_mlp_desc& d = np.d;
  const int side = pe_dim(d), PEC8 = pe_chunks(d) * 8;
  for (int l = 0; l < d.n_lin; ++l) {
    np.scale_off[l] = p->n_scale;
    p->n_scale += d.out_dim[l];
    // effective-weight gradient block [rowsP][colsP] in the layer's padded input space, followed by the bias-grad row
    const bool last = (l == d.n_lin - 1);
    int rowsP = d.hidden, colsP = d.hidden;
    if (kind == 0) {
      if (l == 0) colsP = PEC8;
      else if (l == d.skip_layer) colsP = d.hidden + PEC8;
      if (last) rowsP = 32 + (d.d_out - 1);
    } else if (kind == 1) {
      if (l == 0) colsP = PEC8 + (d.in0 - side);
      if (last) rowsP = 32;
    } else {
      if (l == 0) colsP = d.in0;
      if (last) rowsP = 32;
    }
    np.wg_rows[l] = rowsP; np.wg_cols[l] = colsP;
    np.wgrad_off[l] = p->wgrad_floats;
    p->wgrad_floats += (int64_t)rowsP * colsP + rowsP;
  }
}

}  // namespace

extern "C" int i2sdf_plan_create(const i2sdf_net_desc* desc, i2sdf_plan** out) {
  if (!desc || !out) return I2SDF_EINVAL;
  {  // shapes the kernels are instantiated for: refuse anything else here, with the reason (i2sdf_last_hip_error), not at the first launch
    // (bits 16..23 of rgb.reserved first: the message of the output activation's check covers them)
    if (rgb_act(desc->rgb) > I2SDF_RGB_ACT_SOFTPLUS || (desc->rgb.reserved & 0x00ff0000)) {
      g_hip_err = "i2sdf_plan_create: rgb.reserved " + std::to_string(desc->rgb.reserved) + ": output activation " + std::to_string(rgb_act(desc->rgb)) +
                  " of the radiance net is not one of I2SDF_RGB_ACT_SIGMOID (0), I2SDF_RGB_ACT_RELU (1), I2SDF_RGB_ACT_SOFTPLUS (2) in bits 8..15"
                  " (bits 16..23 must be zero)";
      return I2SDF_EINVAL;
    }
    const int emb = rgb_embed(desc->rgb), n_emb = desc->rgb.multires;
    if (emb > I2SDF_RGB_EMBED_FOURIER || (desc->rgb.reserved & 0xf0000000)) {
      g_hip_err = "i2sdf_plan_create: rgb.reserved " + std::to_string(desc->rgb.reserved) + ": view embedder " + std::to_string(emb) +
                  " of the radiance net is not one of I2SDF_RGB_EMBED_POSITIONAL (0), I2SDF_RGB_EMBED_SH (1), I2SDF_RGB_EMBED_FOURIER (2) in bits 24..27"
                  " (bits 28..31 must be zero)";
      return I2SDF_EINVAL;
    }
    if (emb == I2SDF_RGB_EMBED_SH && (n_emb < 1 || n_emb > 5)) {
      g_hip_err = "i2sdf_plan_create: spherical-harmonics view embedder of degree " + std::to_string(n_emb) +
                  " (rgb.multires): the reference's SHEncoder and the kernels have degrees 1..5";
      return I2SDF_EINVAL;
    }
    if (emb == I2SDF_RGB_EMBED_FOURIER && (n_emb < 1 || n_emb > I2SDF_RGB_EMBED_MAX_CHANNELS)) {
      g_hip_err = "i2sdf_plan_create: Fourier view embedder with " + std::to_string(n_emb) + " channels (rgb.multires): 1..12 fit the 27 view "
                  "columns of the radiance net's side row (width 2 c + 3); more need wider rows";
      return I2SDF_EINVAL;
    }
    const int H = desc->sdf.hidden, Hr = desc->rgb.hidden;
    int F = 0;
    if (desc->rgb.n_lin > 0) {
      if (emb != I2SDF_RGB_EMBED_POSITIONAL) {
        // the feature size cannot be derived from in0 here (that would accept any in0): the SDF net's output says it
        F = desc->sdf.d_out - 1;
        if (desc->rgb.in0 != side_dim(desc->rgb) + F) {
          g_hip_err = "i2sdf_plan_create: rgb.in0 " + std::to_string(desc->rgb.in0) + " disagrees with the view embedder: " +
                      (emb == I2SDF_RGB_EMBED_SH ? "spherical harmonics of degree " : "Fourier features with channels ") + std::to_string(n_emb) +
                      " are " + std::to_string(embed_dim(desc->rgb)) + " wide, the side row " + std::to_string(side_dim(desc->rgb)) +
                      ", so lin0 has " + std::to_string(side_dim(desc->rgb) + F) + " columns with feature size " + std::to_string(F);
          return I2SDF_EINVAL;
        }
      } else {
        F = desc->rgb.in0 - (rgb_idr(desc->rgb) ? side_dim(desc->rgb) : (desc->rgb.multires > 0 ? 3 + 6 * desc->rgb.multires : 3));
      }
    }
    const bool ok = (H == 256 && Hr == 256 && F == 256) || (H == 64 && Hr == 64 && F == 64);
    if (!ok || desc->sdf.multires != 6 || (emb == I2SDF_RGB_EMBED_POSITIONAL && desc->rgb.multires != 4 && desc->rgb.multires != 0)) {
      g_hip_err = "i2sdf_plan_create: SDF width " + std::to_string(H) + " / radiance width " + std::to_string(Hr) + " / feature size " + std::to_string(F) +
                  " / multires " + std::to_string(desc->sdf.multires) + "," + std::to_string(desc->rgb.multires) +
                  ": the MLP kernels are instantiated for 256/256/256 and 64/64/64 with multires 6 (points) and 4 (view directions) only";
      return I2SDF_EINVAL;
    }
    if (rgb_idr(desc->rgb) && desc->rgb.d_in != 9) {
      g_hip_err = "i2sdf_plan_create: the radiance net's 'idr' mode needs d_in 9 (points, view directions, normals)";
      return I2SDF_EINVAL;
    }
    for (const i2sdf_mlp_desc* d : {&desc->sdf, &desc->rgb})
      if (d->n_lin < 2 || d->n_lin > I2SDF_MAX_LAYERS) {
        g_hip_err = std::string("i2sdf_plan_create: ") + (d == &desc->sdf ? "sdf" : "rgb") + ".n_lin " + std::to_string(d->n_lin) +
                    ": a net has 2.." + std::to_string(I2SDF_MAX_LAYERS) + " linear layers (I2SDF_MAX_LAYERS; 1.." +
                    std::to_string(I2SDF_MAX_LAYERS - 1) + " hidden layers and the output layer)";
        return I2SDF_EINVAL;
      }
    if (desc->sdf.skip_layer == 0 || desc->sdf.skip_layer >= desc->sdf.n_lin - 1) {
      g_hip_err = "i2sdf_plan_create: sdf.skip_layer " + std::to_string(desc->sdf.skip_layer) + " with n_lin " + std::to_string(desc->sdf.n_lin) +
                  ": the SDF kernels concatenate PE(x) in front of a hidden layer behind the first one, layers 1.." +
                  std::to_string(desc->sdf.n_lin - 2) + " here (-1: no skip); layer 0 reads PE(x) already and the output layer is evaluated as row vectors";
      return I2SDF_EINVAL;
    }
    const i2sdf_mlp_desc& dl = desc->light;
    if (dl.n_lin != 0 && !(dl.n_lin == 2 && ((dl.hidden == 128 && F == 256) || (dl.hidden == 32 && F == 64)))) {
      g_hip_err = "i2sdf_plan_create: light.n_lin " + std::to_string(dl.n_lin) + " / light.hidden " + std::to_string(dl.hidden) + " at feature size " +
                  std::to_string(F) + ": the light head's kernels are instantiated for one hidden layer of 128 at feature size 256 and of 32 at "
                  "feature size 64 only";
      return I2SDF_EINVAL;
    }
  }
  i2sdf_plan* p = new i2sdf_plan();
  p->desc = *desc;
  p->sdf.d = desc->sdf; p->rgb.d = desc->rgb; p->light.d = desc->light;
  assign_scales_and_wgrad(p, p->sdf, 0);
  assign_scales_and_wgrad(p, p->rgb, 1);
  if (desc->light.n_lin) assign_scales_and_wgrad(p, p->light, 2);
  p->scale_floats = round_up(p->n_scale, CHUNK_FLOATS);
  Builder b{p->segs, 0};
  const char* net = "SDF net";
  int rc = build_sdf(p, b);
  if (!rc) { net = "radiance net"; rc = build_rgb(p, b); }
  if (!rc) { net = "light head"; rc = build_light(p, b); }
  if (rc) {
    g_hip_err = std::string("i2sdf_plan_create: the descriptor of the ") + net + " is inconsistent: its layers' out_dim / in_dim, in0, d_in, d_out or "
                "multires do not follow from n_lin, hidden, skip_layer and the feature size";
    delete p;
    return rc;
  }
  { Seg z{}; z.type = SEG_ZERO; z.nchunks = SC > SCH ? SC : SCH; b.add(z); }   // slack: the DMA look-ahead may touch one stage past the end
  p->total_chunks = b.chunk;
  p->n_segs = (int32_t)p->segs.size();
  // Device copy of the segment table.  On a host without a GPU the plan is still usable for layout queries
  // (sizes, argument validation); every launch entry point then fails with I2SDF_EHIP.
  hipError_t e = hipMalloc((void**)&p->d_segs, sizeof(Seg) * p->segs.size());
  if (e == hipSuccess) e = hipMemcpy(p->d_segs, p->segs.data(), sizeof(Seg) * p->segs.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)i2sdf_hip_check(e, "plan table upload");
    if (p->d_segs) (void)hipFree(p->d_segs);
    p->d_segs = nullptr;
    (void)hipGetLastError();
  }
  {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) p->n_cu = n;
    else (void)hipGetLastError();
  }
  // Defaults (round 6): a fresh plan of a 256-wide configuration runs the kernels every test and profile of this library covers -- the
  // bf16x3 split-arithmetic twins (fp32-equivalent results on the bf16 matrix pipe), blocked saved tensors, the tail overlap -- not the
  // fp32-input MFMA forms, which remain selectable (value 0) as the references the parity tests compare with.  NOT on by default: the
  // options that are narrower than fp32 (I2SDF_OPT_WGRAD_BF16X2, I2SDF_OPT_SAMPLER_BF16X2: a C caller opts in; the Python module turns them
  // on from its conf) and I2SDF_OPT_PARTS (needs chains around the entry points to pay off).  64-wide nets: everything off, as before.
  if (p->H == 256 && p->F == 256)
    for (int32_t opt : {I2SDF_OPT_SDF_FWD_BF16X3, I2SDF_OPT_WGRAD_BF16X3, I2SDF_OPT_TRAIN_FWD_BF16X3, I2SDF_OPT_SDF_BWD_BF16X3, I2SDF_OPT_RGB_BF16X3,
                        I2SDF_OPT_BLOCKED_SAVES, I2SDF_OPT_TAIL_OVERLAP})
      (void)i2sdf_plan_set_option(p, opt, 1);
  *out = p;
  return I2SDF_OK;
}

extern "C" void i2sdf_plan_destroy(i2sdf_plan* p) {
  if (!p) return;
  if (p->d_segs) (void)hipFree(p->d_segs);
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  if (p->ev_join) (void)hipEventDestroy(p->ev_join);
  if (p->side) (void)hipStreamDestroy(p->side);
  for (hipEvent_t e : p->part_ev) if (e) (void)hipEventDestroy(e);
  for (hipStream_t s : p->part_st) if (s) (void)hipStreamDestroy(s);
  delete p;
}

hipStream_t i2sdf_tail_fork(const i2sdf_plan* p, hipStream_t st) {
  if (!p->tail_overlap) return st;
  if (!p->side) {
    // non-blocking: torch's current stream is normally the NULL stream, and a blocking stream would serialise against it
    if (hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking) != hipSuccess) { p->side = nullptr; (void)hipGetLastError(); return st; }
    if (hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamDestroy(p->side); p->side = nullptr;
      return st;
    }
  }
  if (hipEventRecord(p->ev_fork, st) != hipSuccess || hipStreamWaitEvent(p->side, p->ev_fork, 0) != hipSuccess) {
    (void)hipGetLastError();
    return st;
  }
  return p->side;
}

void i2sdf_tail_join(const i2sdf_plan* p, hipStream_t st, hipStream_t side) {
  if (side == st) return;
  (void)hipEventRecord(p->ev_join, side);
  (void)hipStreamWaitEvent(st, p->ev_join, 0);
}

// ---- point ranges (plan.h: PartRun) ---------------------------------------------------------------------------------
namespace {
constexpr int64_t PART_ALIGN = I2SDF_WG_CH;          // == i2sdf_wgrad_chunk_points(): a weight-gradient chunk never straddles two ranges

bool parts_resources(const i2sdf_plan* p) {
  for (int q = 0; q < I2SDF_MAX_PARTS; ++q)
    if (!p->part_ev[q] && hipEventCreateWithFlags(&p->part_ev[q], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
  for (int q = 0; q + 1 < p->parts; ++q)
    if (!p->part_st[q] && hipStreamCreateWithFlags(&p->part_st[q], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
// boundaries of n ranges over a batch of M points, in whole chunks.  Relative sizes: equal, or I2SDF_PART_WEIGHTS="w0,w1,..." (read
// once; an experiment knob: unequal ranges finish their kernels at different times, which is what fills the partly empty rounds)
void part_bounds(int64_t M, int n, int64_t (&b)[I2SDF_MAX_PARTS + 1]) {
  static double w[I2SDF_MAX_PARTS] = {0, 0, 0, 0};
  static int nw = -1;
  if (nw < 0) {
    nw = 0;
    if (const char* e = getenv("I2SDF_PART_WEIGHTS")) {
      while (*e && nw < I2SDF_MAX_PARTS) {
        char* end = nullptr;
        const double v = strtod(e, &end);
        if (end == e) break;
        w[nw++] = v > 0 ? v : 0;
        e = (*end == ',') ? end + 1 : end;
      }
    }
  }
  const int64_t nch = (M + PART_ALIGN - 1) / PART_ALIGN;
  double tot = 0, acc = 0;
  for (int q = 0; q < n; ++q) tot += (nw == n) ? w[q] : 1.0;
  b[0] = 0;
  for (int q = 1; q <= n; ++q) {
    acc += (nw == n) ? w[q - 1] : 1.0;
    int64_t c = tot > 0 ? (int64_t)(nch * (acc / tot) + 0.5) : nch * q / n;
    if (c < b[q - 1] / PART_ALIGN) c = b[q - 1] / PART_ALIGN;
    b[q] = (c > nch ? nch : c) * PART_ALIGN;
  }
  b[n] = nch * PART_ALIGN;
}
}  // namespace

void i2sdf_parts_fence(const i2sdf_plan* p, hipStream_t st) {
  (void)hipEventRecord(p->part_ev[0], st);
  for (int q = 0; q + 1 < p->parts; ++q) (void)hipStreamWaitEvent(p->part_st[q], p->part_ev[0], 0);
}
void i2sdf_parts_join_all(const i2sdf_plan* p, hipStream_t st) {
  for (int q = 0; q + 1 < p->parts; ++q) {
    if (!p->part_st[q] || !p->part_ev[q + 1]) continue;
    (void)hipEventRecord(p->part_ev[q + 1], p->part_st[q]);
    (void)hipStreamWaitEvent(st, p->part_ev[q + 1], 0);
  }
}
bool i2sdf_parts_begin(const i2sdf_plan* p, hipStream_t st, int64_t M, PartRun* pr) {
  pr->n = 1; pr->st[0] = st; pr->lo[0] = 0; pr->hi[0] = M; pr->own = false;
  if (!i2sdf_parts_on(p) || M <= 0) return false;
  const bool chain = p->chain_active != 0;
  const int64_t Mref = chain ? (p->chain_M > M ? p->chain_M : M) : M;
  if ((Mref + PART_ALIGN - 1) / PART_ALIGN < p->parts) return false;        // fewer chunks than ranges: one launch
  if (!parts_resources(p)) return false;
  int64_t b[I2SDF_MAX_PARTS + 1];
  part_bounds(Mref, p->parts, b);
  pr->n = p->parts;
  for (int q = 0; q < pr->n; ++q) {
    pr->st[q] = q == 0 ? st : p->part_st[q - 1];
    pr->lo[q] = b[q] < M ? b[q] : M;
    pr->hi[q] = b[q + 1] < M ? b[q + 1] : M;
  }
  if (!chain) { i2sdf_parts_fence(p, st); pr->own = true; }
  return true;
}
void i2sdf_parts_end(const i2sdf_plan* p, hipStream_t st, PartRun* pr) {
  if (pr->own) i2sdf_parts_join_all(p, st);
  pr->own = false;
}

extern "C" int i2sdf_chain_begin(const i2sdf_plan* p, int64_t M, void* stream) {
  if (!p || M < 0) return I2SDF_EINVAL;
  if (!i2sdf_parts_on(p) || M == 0) return I2SDF_OK;
  if (p->chain_active) return I2SDF_EINVAL;                  // chains do not nest
  if (!parts_resources(p)) return i2sdf_hip_check(hipErrorOutOfMemory, "chain_begin: streams / events");
  i2sdf_parts_fence(p, (hipStream_t)stream);
  p->chain_active = 1;
  p->chain_M = M;
  return i2sdf_hip_check(hipGetLastError(), "chain_begin");
}
extern "C" int i2sdf_chain_fence(const i2sdf_plan* p, void* stream) {
  if (!p) return I2SDF_EINVAL;
  if (!p->chain_active) return I2SDF_OK;
  i2sdf_parts_fence(p, (hipStream_t)stream);
  return i2sdf_hip_check(hipGetLastError(), "chain_fence");
}
extern "C" int i2sdf_chain_end(const i2sdf_plan* p, void* stream) {
  if (!p) return I2SDF_EINVAL;
  if (!p->chain_active) return I2SDF_OK;
  i2sdf_parts_join_all(p, (hipStream_t)stream);
  p->chain_active = 0;
  p->chain_M = 0;
  return i2sdf_hip_check(hipGetLastError(), "chain_end");
}

extern "C" int i2sdf_plan_set_option(i2sdf_plan* p, int32_t option, int32_t value) {
  if (!p) return I2SDF_EINVAL;
  if (option == I2SDF_OPT_PARTS) {
    if (value < 0 || value > I2SDF_MAX_PARTS || p->chain_active) return I2SDF_EINVAL;
    p->parts = value >= 2 ? value : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_SDF_FWD_BF16X3) {
    // the option is accepted only where a bf16x3 kernel will actually run (mlp_fwd.hip: launch_sdf_fwd): 256-wide nets on the 16-point-wave
    // stream, 64-wide nets on the 32-point stream -- a shape with neither would otherwise report success and fall through to fp32 MFMA
    const bool runs = (p->H == 256 && p->F == 256 && span_chunks(p->sdf, SPAN_FWD3H) > 0) || (p->H == 64 && p->F == 64 && span_chunks(p->sdf, SPAN_FWD3) > 0);
    if (value && !runs) return I2SDF_EINVAL;
    p->sdf_fwd_bf16x3 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_SAMPLER_BF16X2) {
    // only the passes inside i2sdf_sample_rays / i2sdf_render_image (they choose depths); i2sdf_sdf_forward and i2sdf_sdf_grid return values
    // and keep three planes.  Needs the 16-point-wave forward (I2SDF_OPT_SDF_FWD_BF16X3 on a 256-wide net).
    if (value && (span_chunks(p->sdf, SPAN_FWD2H) == 0 || p->H != 256 || p->F != 256)) return I2SDF_EINVAL;
    p->sampler_bf16x2 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_TRAIN_FWD_BF16X3) {
    if (value && (span_chunks(p->sdf, SPAN_REV3_CHAIN) == 0 || span_chunks(p->sdf, SPAN_FWD3H) == 0 || p->H != 256 || p->F != 256)) return I2SDF_EINVAL;
    p->train_fwd_bf16x3 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_SDF_BWD_BF16X3) {
    if (value && (span_chunks(p->sdf, SPAN_REV3_CHAIN) == 0 || p->H != 256 || p->F != 256)) return I2SDF_EINVAL;
    p->sdf_bwd_bf16x3 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_RGB_BF16X3) {
    if (value && (span_chunks(p->rgb, SPAN_REV3H) == 0 || p->rgb.d.hidden != 256 || p->F != 256 || p->rgb.d.n_lin < 3)) return I2SDF_EINVAL;
    p->rgb_bf16x3 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_WGRAD_BF16X3) {
    p->wgrad_bf16x3 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_WGRAD_BF16X2) {
    p->wgrad_bf16x2 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_BLOCKED_SAVES) {
    p->blocked_saves = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_SAVES24) {
    if (value && (p->H != 256 || p->F != 256 || span_chunks(p->sdf, SPAN_REV3_CHAIN) == 0)) return I2SDF_EINVAL;
    if (p->chain_active) return I2SDF_EINVAL;          // the layout of tensors in flight
    p->saves24 = value ? 1 : 0;
    return I2SDF_OK;
  }
  if (option == I2SDF_OPT_TAIL_OVERLAP) {
    p->tail_overlap = value ? 1 : 0;
    return I2SDF_OK;
  }
  return I2SDF_EINVAL;
}

extern "C" int i2sdf_plan_set_view_embed(i2sdf_plan* p, const float* B_host, int32_t rows, int32_t cols) {
  if (!p) return I2SDF_EINVAL;
  const auto refuse = [](const std::string& why) { g_hip_err = "i2sdf_plan_set_view_embed: " + why; return I2SDF_EINVAL; };
  if (rgb_embed(p->rgb.d) != I2SDF_RGB_EMBED_FOURIER) return refuse("the plan's radiance net has no Fourier view embedder (rgb.reserved bits 24..27)");
  if (!B_host) return refuse("B_host is NULL");
  if (rows != 3 || cols != p->rgb.d.multires)
    return refuse("B is (" + std::to_string(rows) + ", " + std::to_string(cols) + "), the plan's embedder takes (3, " + std::to_string(p->rgb.d.multires) + ")");
  for (int i = 0; i < 3 * cols; ++i)
    if (!(B_host[i] - B_host[i] == 0.0f)) return refuse("B[" + std::to_string(i / cols) + "][" + std::to_string(i % cols) + "] is not finite");
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < I2SDF_RGB_EMBED_MAX_CHANNELS; ++c) p->view_B[r * I2SDF_RGB_EMBED_MAX_CHANNELS + c] = c < cols ? B_host[r * cols + c] : 0.0f;
  p->view_B_set = 1;
  return I2SDF_OK;
}

extern "C" int i2sdf_plan_set_exchange(i2sdf_plan* p, const i2sdf_exchange* ex, int32_t flags) {
  if (!p || (flags & ~I2SDF_DP_GLOBAL_SAMPLER) || (ex && !ex->allreduce)) return I2SDF_EINVAL;
  p->exchange = ex ? *ex : i2sdf_exchange{nullptr, nullptr};
  p->dp_flags = ex ? flags : 0;
  return I2SDF_OK;
}

extern "C" int64_t i2sdf_plan_pack_floats(const i2sdf_plan* p) {
  return p ? p->scale_floats + p->total_chunks * CHUNK_FLOATS : 0;
}
extern "C" int64_t i2sdf_plan_wgrad_floats(const i2sdf_plan* p) { return p ? p->wgrad_floats : 0; }
