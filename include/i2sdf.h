/*
 * i2sdf.h -- C ABI of the MI355X-native volume-rendering core for I2-SDF.
 *
 * The upstream reference (jingsenzhu/i2-sdf) has no FFI / plugin interface: its hot path is entered
 * through one Python call form, `I2SDFNetwork.forward(input, predict_only)` (model/network/__init__.py:80),
 * plus bare `implicit_network(x)` queries (model/eval/recon.py:51,90).  This header is the boundary a
 * maintainer binds UNDER that Python module (ctypes stub in INTEGRATION.md): every entry point replaces a
 * span of stock-torch ops of the reference, cited per function as file:line relative to the upstream root.
 *
 * Conventions
 *   - plain C: raw device pointers, explicit sizes, no torch types;
 *   - all tensors fp32, row-major, contiguous unless a leading dimension is given;
 *   - stream-ordered on the `hipStream_t` passed last (as void*), re-entrant, no allocation inside,
 *     no hidden global state: everything a call needs travels in `i2sdf_net` + caller-owned buffers;
 *   - return 0 on success, a negative I2SDF_E* code otherwise (never exit(), unlike
 *     utils/rend_util.py:220-222); `i2sdf_strerror` maps codes to text.
 */
#ifndef I2SDF_H
#define I2SDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2SDF_VERSION 100          /* major*10000 + minor*100 + patch */
#define I2SDF_MAX_LAYERS 12
#define I2SDF_MAX_PARTS 4           /* I2SDF_OPT_PARTS: point ranges per batch (one HIP stream each) */

#define I2SDF_OK 0
#define I2SDF_EINVAL (-1)          /* bad argument / unsupported shape */
#define I2SDF_EHIP (-2)            /* HIP runtime error (see i2sdf_last_hip_error) */
#define I2SDF_ESPHERE (-3)         /* ray does not hit the bounding sphere (rend_util.py:220 `exit()`) */
#define I2SDF_EWORKSPACE (-4)      /* caller workspace too small */
#define I2SDF_ECOMM (-5)           /* RCCL error or RCCL unavailable, see i2sdf_last_comm_error() */

/* ------------------------------------------------------------------------------------------------
 * Network description.  Parameters live in ONE flat fp32 device buffer (`params`), laid out exactly in
 * the reference's state_dict order: for each net, for each layer l: bias[out], weight_g[out],
 * weight_v[out*in] (model/network/mlp.py:45-74, 196-203); then density.beta (density.py:6-8).
 * Offsets are in floats.
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_mlp_desc {
  int32_t n_lin;                          /* number of nn.Linear layers                              */
  int32_t hidden;                         /* hidden width H (multiple of 32, <= 256)                 */
  int32_t d_in;                           /* raw input dims of layer 0 before encoding               */
  int32_t in0;                            /* columns of lin0.weight_v                                */
  int32_t d_out;                          /* rows of the last layer                                  */
  int32_t multires;                       /* positional-encoding frequencies L (embedder.py:138-152); radiance net with another view
                                             embedder (I2SDF_RGB_EMBED_*): the SH degree or the Fourier channel count */
  int32_t skip_layer;                     /* l with `l in skip_in` (mlp.py:94), -1 if none           */
  int32_t reserved;                       /* radiance net: I2SDF_RGB_MODE_* | I2SDF_RGB_ACT_* << 8 | I2SDF_RGB_EMBED_* << 24 (0 = 'nerf', sigmoid,
                                             positional); 0 for the other nets */
  int32_t out_dim[I2SDF_MAX_LAYERS];      /* rows of weight_v per layer                              */
  int32_t in_dim[I2SDF_MAX_LAYERS];       /* cols of weight_v per layer                              */
  int64_t off_bias[I2SDF_MAX_LAYERS];
  int64_t off_g[I2SDF_MAX_LAYERS];
  int64_t off_v[I2SDF_MAX_LAYERS];
} i2sdf_mlp_desc;

/* rendering_network.mode (mlp.py:185-216), carried by i2sdf_net_desc.rgb.reserved.  It decides the columns of lin0.weight_v in front of the
 * feature columns -- the per-point "side row" of the radiance net:
 *   I2SDF_RGB_MODE_NERF  [PE4(view_dir) (27)]                          d_in = 3, in0 = 27 + F
 *   I2SDF_RGB_MODE_IDR   [point (3) | PE4(view_dir) (27) | normal (3)]  d_in = 9, in0 = 33 + F   (normal = the raw d sdf/dx, not normalised)
 *                        multires 0 (no view encoding): [point | view_dir | normal], in0 = 9 + F
 * d_in has to agree with the mode; i2sdf_plan_create refuses anything else. */
#define I2SDF_RGB_MODE_NERF 0
#define I2SDF_RGB_MODE_IDR 1
/* rendering_network.output_activation (mlp.py:153-157, 206, 227), the last operation of the radiance net, in bits 8..15 of the same field:
 * rgb.reserved = I2SDF_RGB_MODE_* | I2SDF_RGB_ACT_* << 8.  A descriptor written before the activations existed (bits 8..15 zero) keeps its
 * meaning: sigmoid.  With o the output of the last linear layer and y the value the forward entry points write to `rgb`:
 *   I2SDF_RGB_ACT_SIGMOID   y = 1 / (1 + exp(-o))                                 dy/do = y (1 - y)
 *   I2SDF_RGB_ACT_RELU      y = max(o, 0): radiance above 1 (HDR targets)         dy/do = y > 0 (0 at the kink, as torch)
 *   I2SDF_RGB_ACT_SOFTPLUS  y = o > 20 ? o : log1p(exp(o))  (nn.Softplus())       dy/do = y > 20 ? 1 : -expm1(-y)  (= sigmoid(o), exactly)
 * The backward entry points recover dy/do from the saved `rgb` alone; no further tensor is saved.  The packed weights, the state_dict and
 * every workspace are the same for the three.  i2sdf_plan_create refuses any other value (and any bit above 15) with I2SDF_EINVAL and a
 * text in i2sdf_last_hip_error().  Nothing behind the radiance net assumes rgb <= 1 (compositing and the rgb loss are linear in it). */
#define I2SDF_RGB_ACT_SIGMOID 0
#define I2SDF_RGB_ACT_RELU 1
#define I2SDF_RGB_ACT_SOFTPLUS 2
/* rendering_network.embed_type (embedder.py:138-160), the embedder E of the unit view direction v, in bits 24..27 of the same field;
 * rgb.multires carries its parameter.  e = the width of E(v); the side row is [E(v)] ('nerf', in0 = e + F) or [point | E(v) | normal]
 * ('idr', in0 = e + 6 + F).  Bits 16..23 and 28..31 must be zero.
 *   I2SDF_RGB_EMBED_POSITIONAL  multires = L in {4, 0}: [v | sin(2^k v), cos(2^k v), k < L], e = 3 + 6 L (L = 0: v itself).  A descriptor
 *                               written before the other embedders existed (bits 24..27 zero) keeps its value and meaning.
 *   I2SDF_RGB_EMBED_SH          multires = degree in 1..5: the real spherical harmonics below that degree in the polynomial forms and
 *                               constants of SHEncoder (embedder.py:84-122), e = degree^2.  No state.
 *   I2SDF_RGB_EMBED_FOURIER     multires = channels c in 1..12: [v | sin(2 pi v B) | cos(2 pi v B)] (FourierFeature, include_input), e = 2 c + 3.
 *                               B (3, c) is a buffer of the module, not a parameter: i2sdf_plan_set_view_embed hands it to the plan.
 * Every e up to 27 fits the columns the positional encoding already has (27 of 32 in 'nerf', 33 of 40 in 'idr' mode): the packed streams,
 * the saved side row (pev_save: (Mp,32) / (Mp,40), columns at and beyond the row's width exactly zero) and the weight-gradient blocks keep
 * the sizes of the positional plan.  i2sdf_plan_create refuses an unknown kind, a degree or channel count out of range and an in0 that
 * disagrees with e, each with I2SDF_EINVAL and a text in i2sdf_last_hip_error(). */
#define I2SDF_RGB_EMBED_POSITIONAL 0
#define I2SDF_RGB_EMBED_SH 1
#define I2SDF_RGB_EMBED_FOURIER 2
#define I2SDF_RGB_EMBED_MAX_CHANNELS 12

typedef struct i2sdf_net_desc {
  i2sdf_mlp_desc sdf;                     /* ImplicitNetwork: PE(x) -> softplus100 stack -> [sdf | feature]   */
  i2sdf_mlp_desc rgb;                     /* RenderingNetwork: [side row | feature] -> ReLU -> output act.    */
  i2sdf_mlp_desc light;                   /* light-mask head (n_lin == 0 when absent)                         */
  int64_t off_beta;                       /* density.beta                                                     */
  int64_t n_params;                       /* total floats in `params`                                         */
  float beta_min;                         /* density.py:17                                                    */
  float scene_bounding_sphere;            /* model/network/__init__.py:23                                     */
} i2sdf_net_desc;

/* Opaque, caller-owned plan: host copy of the derived layouts + a small device table.
 * i2sdf_plan_create allocates it (the only allocation in the library, one-time), i2sdf_plan_destroy frees. */
typedef struct i2sdf_plan i2sdf_plan;

int i2sdf_version(void);
const char* i2sdf_strerror(int code);
const char* i2sdf_last_hip_error(void);    /* thread-local text of the last HIP failure */

int i2sdf_plan_create(const i2sdf_net_desc* desc, i2sdf_plan** out);
void i2sdf_plan_destroy(i2sdf_plan* plan);
/* Plan options (host side, takes effect on the next launch).
 * Defaults (round 6): a plan of a 256-wide configuration is created with the five *_BF16X3 options, I2SDF_OPT_BLOCKED_SAVES and
 * I2SDF_OPT_TAIL_OVERLAP ON (fp32-equivalent results from the kernels the parity tests and profiles cover), I2SDF_OPT_WGRAD_BF16X2,
 * I2SDF_OPT_SAMPLER_BF16X2 and I2SDF_OPT_PARTS off; a 64-wide plan with everything off.  Value 0 selects the fp32-input MFMA form.
 *   I2SDF_OPT_SDF_FWD_BF16X3: evaluate the sdf-only forward (i2sdf_sdf_forward without features, and the SDF passes inside
 *   i2sdf_sample_rays) in bf16x3 split arithmetic: every fp32 operand is split into three bf16 terms and the six leading
 *   partial products are accumulated in fp32 on the bf16 matrix pipe -- results agree with the fp32 path to fp32 rounding
 *   level (same 1e-4 parity bar) at 3/8 of the matrix-pipe cycles.  (0 = plain fp32 MFMA.) */
#define I2SDF_OPT_SDF_FWD_BF16X3 1
/*   I2SDF_OPT_WGRAD_BF16X3: the 256x256 blocks of i2sdf_weight_grads in the same split arithmetic (both operands are split
 *   on the fly); the narrower blocks run the split form with three planes then, the fp32 MFMA kernel otherwise. */
#define I2SDF_OPT_WGRAD_BF16X3 2
/*   I2SDF_OPT_TRAIN_FWD_BF16X3: the full workgroups of i2sdf_sdf_forward_grad (256-wide nets) in the same arithmetic. */
#define I2SDF_OPT_TRAIN_FWD_BF16X3 4
/*   I2SDF_OPT_SDF_BWD_BF16X3: the full workgroups of i2sdf_sdf_backward (both sweeps, 256-wide nets). */
#define I2SDF_OPT_SDF_BWD_BF16X3 8
/*   I2SDF_OPT_RGB_BF16X3: the full workgroups of i2sdf_rgb_forward / i2sdf_rgb_backward and their _idr twins (256-wide nets), and i2sdf_light_forward of the
 *   128-unit light-mask head on 256 features. */
#define I2SDF_OPT_RGB_BF16X3 16
/*   I2SDF_OPT_TAIL_OVERLAP: the split-K tail workgroups of i2sdf_sdf_forward_grad and i2sdf_sdf_backward (the partial last
 *   round of a launch) and the narrow blocks of i2sdf_weight_grads run on a side stream owned by the plan,
 *   concurrently with the full workgroups / the 256x256 blocks; the entry point still returns stream-ordered on the
 *   caller's stream (fork/join with events; capturable in a hipGraph). */
#define I2SDF_OPT_TAIL_OVERLAP 32
/*   (64 was I2SDF_OPT_SRC_RING: saved-tensor reads through a per-wave LDS DMA ring -- built and measured in rounds 2-3, no gain, removed) */
/*   I2SDF_OPT_BLOCKED_SAVES: the 256-wide tensors saved for the backward (hs, abars, gus, gas, rs, gar) are stored in a blocked
 *   layout [Mp/32][16 k-chunks][32 points][16 floats] for the points handled by the bf16x3 full workgroups (point-major for the
 *   rest): a wave instruction of the K-outer kernels then moves one contiguous 2 KB run instead of touching 32 rows 1 KB apart.
 *   Set it before the first i2sdf_sdf_forward_grad of a step and leave it unchanged through i2sdf_weight_grads; the tensors are
 *   opaque to the caller (i2sdf_blocked_points below gives the address formula for inspecting a copy). */
#define I2SDF_OPT_BLOCKED_SAVES 128
/*   I2SDF_OPT_WGRAD_BF16X2 (needs I2SDF_OPT_WGRAD_BF16X3): the 256x256 weight-gradient blocks split every operand into TWO bf16
 *   terms and accumulate the three leading products a0b0 + a0b1 + a1b0 in fp32: per-product error <= 3 * 2^-18 (1.1e-5), i.e.
 *   16+ mantissa bits per operand -- more than the TF32 / bf16 internals the reference itself runs its matmuls with
 *   (main_recon.py:61: torch.set_float32_matmul_precision('medium')), less than fp32.  Only the weight gradients qualify: they are
 *   terminal sums over ~1e5 points (rounding errors of the terms average out and propagate nowhere), measured 1e-5-level
 *   max-norm error of every parameter gradient against fp64 (parity bar 1e-4).  Half the MFMAs and 2/3 of the split work of the
 *   bf16x3 form.  Default 0; every other kernel keeps the fp32-equivalent bf16x3 / fp32 arithmetic. */
#define I2SDF_OPT_WGRAD_BF16X2 256
/*   I2SDF_OPT_PARTS (value n = 2..I2SDF_MAX_PARTS, 0 / 1 = off; 256-wide nets with the bf16x3 options on): the per-point entry points
 *   (i2sdf_sdf_forward_grad, i2sdf_rgb_forward, i2sdf_rgb_backward and their _idr twins, i2sdf_sdf_backward, the GEMMs of i2sdf_weight_grads) cut their
 *   point batch into n ranges at multiples of i2sdf_wgrad_chunk_points(); range 0 runs on the caller's stream, the others on streams
 *   owned by the plan.  On its own an entry point forks and joins (it returns stream-ordered on the caller's stream, as without the
 *   option).  Between i2sdf_chain_begin and i2sdf_chain_end the ranges stay un-joined ACROSS entry points: every range runs its own
 *   chain of kernels, the ranges drift apart, and the partly empty last round of one kernel (M/128 workgroups on 256 CUs) is filled
 *   by another range's next kernel instead of idling -- which replaces the split-K tail workgroups (none in this mode: every point
 *   goes through the full-workgroup kernels and every saved tensor is blocked throughout).  Results do not depend on n.  Default 0. */
#define I2SDF_OPT_PARTS 512
/*   I2SDF_OPT_SAMPLER_BF16X2 (256-wide nets with I2SDF_OPT_SDF_FWD_BF16X3): the sdf-only passes INSIDE i2sdf_sample_rays and
 *   i2sdf_render_image -- the evaluations the error-bounded sampler chooses its depths from (ray_sampler.py:83-95, under no_grad) --
 *   split every operand into TWO bf16 terms and accumulate the three leading products (per-product error <= 3 * 2^-18): half the MFMAs
 *   of the bf16x3 form.  No returned value is computed from these passes (sdf, colours, gradients at the chosen depths come from the
 *   fp32-equivalent kernels); what changes is WHERE the samples sit, by a perturbation of the sdf of ~1e-5 relative -- well inside what
 *   the reference itself computes them with on its GPU (torch.set_float32_matmul_precision('medium'), main_recon.py:61).
 *   i2sdf_sdf_forward and i2sdf_sdf_grid (values that are returned) keep three planes.  Default 0. */
#define I2SDF_OPT_SAMPLER_BF16X2 1024
/*   I2SDF_OPT_SAVES24 (256-wide nets; takes effect only together with I2SDF_OPT_PARTS, I2SDF_OPT_BLOCKED_SAVES, the *_BF16X3 options and
 *   I2SDF_OPT_WGRAD_BF16X2 -- otherwise the tensors keep their fp32 form): abars, gus and gas -- the three saved SDF tensors whose consumers are
 *   the weight-gradient GEMMs (which in the two-plane form keep 16 significant bits of every operand) and, for abars / gus, the second-order
 *   injection of sweep 2 -- are stored with 16 significant bits (round to nearest, relative error <= 2^-16 per element) as 3 bytes per value
 *   inside their fp32 allocation (layout: mlp_common.h P24).  hs stays fp32.  8 of the 13 saved-tensor passes per layer move 3/4 of their bytes.
 *   Measured: every parameter gradient stays within 7e-7 (max-norm relative) of the fp32-storage result at 1024 rays; the parity bar is 1e-4
 *   against fp64.  The tensors are opaque to the caller in this form (i2sdf_amd.engine.saved_to_point_major decodes a copy).  Default 0. */
#define I2SDF_OPT_SAVES24 2048
/* number of leading points (a multiple of 32) of a batch whose saved tensors are blocked under the current options: which = 0
 * hs / abars / gus / gas of an i2sdf_sdf_forward_grad batch of M points (has_feat: feat != NULL in that call), which = 1 rs / gar
 * of an i2sdf_rgb_forward batch (of an i2sdf_rgb_forward_idr batch: Mp or 0, that mode has no split-K tail).  Element (point m < that count, column c) of a blocked (Mp,256) tensor lives at float offset
 * (m/32)*8192 + (c/16)*512 + (m%32)*16 + c%16; points behind the count are ordinary rows m*256 + c.
 * which = 2: the leading points whose abars / gus / gas are packed 24-bit records under the current options (I2SDF_OPT_SAVES24: Mp -- every point --
 * or 0).  A packed layer holds, per 32-point block (6144 floats, dense) and 16-column k-chunk (384 floats): 32 x 2 x 4 dwords of upper halves
 * (lane hi = 0, 1 of point p at dword p*8 + hi*4; value u of that lane = column 4 hi + u for u < 4, 8 + 4 hi + u - 4 for u >= 4; two values per dword)
 * and, from dword 256 on, 32 x 2 x 2 dwords of mid bytes (four per dword); value = upper half << 16 | mid byte << 8.  The top layer of gus stays fp32. */
int64_t i2sdf_blocked_points(const i2sdf_plan* plan, int32_t which, int64_t M, int64_t Mp, int32_t has_feat);
int i2sdf_plan_set_option(i2sdf_plan* plan, int32_t option, int32_t value);
/* A chain (I2SDF_OPT_PARTS): the per-point entry points called between begin and end leave their point ranges un-joined.
 *   i2sdf_chain_begin(plan, M, stream): the ranges are cut from a batch of M points (the LARGEST batch of the chain: entry points
 *     with fewer points clip them); the side streams wait for everything enqueued on `stream` so far.
 *   i2sdf_chain_fence(plan, stream): the side streams additionally wait for what was enqueued on `stream` since (call it after
 *     enqueueing, on `stream`, an input that a later entry point of the chain reads).
 *   i2sdf_chain_end(plan, stream): `stream` waits for every range; afterwards everything the chain wrote is visible on `stream`.
 * Inside a chain only the entry points named at I2SDF_OPT_PARTS may be called, with the same `stream`; i2sdf_weight_grads joins the
 * ranges itself before its final reduction.  Without I2SDF_OPT_PARTS all three calls do nothing. */
int i2sdf_chain_begin(const i2sdf_plan* plan, int64_t M, void* stream);
int i2sdf_chain_fence(const i2sdf_plan* plan, void* stream);
int i2sdf_chain_end(const i2sdf_plan* plan, void* stream);
/* floats of device memory the packed weight streams need (pass to i2sdf_pack_weights) */
int64_t i2sdf_plan_pack_floats(const i2sdf_plan* plan);
/* floats of ONE split-M chunk of effective-weight gradient partial sums: i2sdf_weight_grads takes n_chunks x this many floats of
 * workspace (`partials`) and reduces them, fused with the weight-norm backward, into the flat gradient */
int64_t i2sdf_plan_wgrad_floats(const i2sdf_plan* plan);

/* ------------------------------------------------------------------------------------------------
 * Weight-norm reparametrisation + packing.  Replaces `W = g * v/||v||` executed inside every `lin(x)`
 * (mlp.py:71-72,97,222) for all layers at once and lays W out in the order the MFMA kernels stream it.
 * Must be called after every parameter update, before any kernel below.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_pack_weights(const i2sdf_plan* plan, const float* params, float* packed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SDF network forward without gradient -- ImplicitNetwork.forward / get_sdf_vals (mlp.py:84-105,145-151),
 * the call the sampler (ray_sampler.py:88-89), marching cubes (model/eval/recon.py:51,90) and the bubble
 * loss (model/network/__init__.py:200) make.
 *   points   (M,3)
 *   sdf_out  (M)            or NULL
 *   feat_out (M, ld_feat)   or NULL : the feature columns out[:,1:]   (ld_feat >= feature size, multiple of 4)
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_sdf_forward(const i2sdf_plan* plan, const float* packed, const float* points, int64_t M,
                      float* sdf_out, float* feat_out, int64_t ld_feat, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Point batches.  The training kernels take a batch laid out as
 *     [ n_ray_pts points generated from rays | (M - n_ray_pts) explicit points ]
 * ray part:  x[m] = cam[r] + z[r*ldz + j]*dirs[r], r = m / n_per_ray, j = m % n_per_ray (model/network/__init__.py:103)
 * explicit:  x[m] = points[m - n_ray_pts]        (eikonal / neighbour / bubble points, :178-201)
 * Every per-point workspace below has Mp rows (Mp multiple of 128, >= M); rows >= M are never read (kernels may WRITE them: the saved
 * tensors' stores of padding points are unconditional instructions, which lets the stage waits count them -- csrc/x3.h).
 *
 * SDF network forward WITH d sdf/dx and saved activations -- ImplicitNetwork.get_outputs / .gradient
 * (mlp.py:107-143) as called by the main render pass (model/network/__init__.py:113) and the eikonal pass
 * (:188).  The reference obtains d sdf/dx from torch.autograd.grad(create_graph=True); here the reverse
 * chain is explicit and fused into the same kernel.
 *   sdf (M) ; feat (Mp,F) or NULL ; grad (M,3) or NULL
 *   hs      (L-1, Mp, H)  h_l = softplus100(a_{l-1}), l = 1..L-1   (required when grad != NULL)
 *   abars   (L-1, Mp, H)  d sdf / d a_l, l = 0..L-2                (NULL if no backward will follow)
 *   pe_save (Mp, 40)      PE(x), an operand of the weight-gradient GEMMs (NULL if no backward will follow)
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_sdf_forward_grad(const i2sdf_plan* plan, const float* packed, const float* points, const float* cam,
                           const float* dirs, const float* z, int64_t ldz, int32_t n_per_ray, int64_t n_ray_pts, int64_t M,
                           int64_t Mp, float* sdf, float* feat, float* grad, float* hs, float* abars, float* pe_save,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * The matrix B of a Fourier view embedder (I2SDF_RGB_EMBED_FOURIER): B_host (rows, cols) = (3, c) row-major fp32 in HOST memory, c the
 * plan's rgb.multires.  The plan keeps a copy; the radiance forward entry points (i2sdf_rgb_forward, i2sdf_rgb_forward_idr and everything
 * built on them: i2sdf_render_image) pass it to their kernels by value -- no device allocation, no copy, no synchronisation.  Call it once
 * after i2sdf_plan_create and again whenever B changes (a loaded checkpoint); a call takes effect for the launches enqueued after it.
 * I2SDF_EINVAL with a text in i2sdf_last_hip_error(): a plan of another embedder, rows != 3, cols != c, a NULL or non-finite B_host.
 * On a Fourier plan a radiance forward BEFORE the first call returns I2SDF_EINVAL (text in i2sdf_last_hip_error()) and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_plan_set_view_embed(i2sdf_plan* plan, const float* B_host, int32_t rows, int32_t cols);

/* ------------------------------------------------------------------------------------------------
 * Radiance network forward, 'nerf' mode -- RenderingNetwork.forward (mlp.py:208-229):
 * rgb = act(MLP([PE4(view_dir) | feature])), act = the plan's I2SDF_RGB_ACT_* (sigmoid unless the descriptor says otherwise).
 * dirs (B,3) unit view directions, point m uses dirs[m / n_per_ray].
 *   rgb (M,3) ; rs (L-1, Mp, H) post-ReLU activations and pev_save (Mp,32) PE(view) (NULL if no backward follows)
 * With I2SDF_RGB_EMBED_SH / _FOURIER, E(view_dir) takes the place of PE4(view_dir) here and in 'idr' mode; pev_save keeps its width.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_rgb_forward(const i2sdf_plan* plan, const float* packed, const float* dirs, int32_t n_per_ray, const float* feat,
                      int64_t M, int64_t Mp, float* rgb, float* rs, float* pev_save, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Radiance network forward, 'idr' mode (mlp.py:208-216; a plan whose rgb.reserved is I2SDF_RGB_MODE_IDR -- i2sdf_rgb_forward returns
 * I2SDF_EINVAL on such a plan, this entry point on a 'nerf' plan): rgb = act(MLP([x | PE4(view_dir) | normal | feature])).
 * The 33-wide side row [x | PE(view) | normal] is assembled per point in registers:
 *   x       points (M,3) when given, else cam[r] + z[r*ldz + j] * dirs[r] with r = m / n_per_ray, j = m % n_per_ray (as i2sdf_sdf_forward_grad)
 *   view    dirs[m / n_per_ray], as in 'nerf' mode
 *   normal  normals (M,3): the `grad` output of i2sdf_sdf_forward_grad, used as it is
 *   rgb (M,3) ; rs (L-1, Mp, H) post-ReLU activations and pev_save (Mp,40) the side row, zero padded (NULL if no backward follows)
 *   With the view directions unencoded (rgb.multires 0: embed_type null) the side row is [x | view_dir | normal], 9 wide, pev_save (Mp,16).
 * d loss / d x is not formed by the backward: the points carry no parameter dependence (the sampler runs without grad).
 * Honours I2SDF_OPT_RGB_BF16X3, I2SDF_OPT_PARTS and I2SDF_OPT_BLOCKED_SAVES as i2sdf_rgb_forward does; every point goes through full
 * 128-point workgroups (no split-K tail in this mode, so the blocked prefix of rs is the whole batch).
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_rgb_forward_idr(const i2sdf_plan* plan, const float* packed, const float* points, const float* cam, const float* dirs,
                          const float* z, int64_t ldz, int32_t n_per_ray, const float* normals, const float* feat, int64_t M, int64_t Mp,
                          float* rgb, float* rs, float* pev_save, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the radiance network (autograd through mlp.py:208-229).
 *   rgb (M,3) forward output, rgb_bar (M,3) upstream, rs from the forward; G(a_{L-1}) = rgb_bar * dy/do of the plan's I2SDF_RGB_ACT_*, from rgb
 *   -> gar (L-1, Mp, H) G(a_l) l=0..L-2 ; ga_last (Mp,4) G(a_{L-1}) ; fbar (Mp,F) d loss / d feature
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_rgb_backward(const i2sdf_plan* plan, const float* packed, const float* rgb, const float* rgb_bar, const float* rs,
                       int64_t M, int64_t Mp, float* gar, float* ga_last, float* fbar, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the radiance network in 'idr' mode (i2sdf_rgb_backward returns I2SDF_EINVAL on such a plan): as above, and in the same
 * kernel, from G(a_0) while it is in registers,
 *   nbar_rgb[m] = W_0[:, normal columns]^T G(a_0)[m]      (M,3)  d loss / d normal through the radiance net
 * accumulate == 0: nbar (M,3) is written ; != 0: nbar_rgb is ADDED to it -- the rows [0, M) of the `nbar` that i2sdf_sdf_backward takes,
 * after the compositing / loss backward has written them.  One lane owns a point: plain loads and stores, no atomics, deterministic.
 * The six extra columns of d W_0 come out of i2sdf_weight_grads through the 40-wide pev_save operand.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_rgb_backward_idr(const i2sdf_plan* plan, const float* packed, const float* rgb, const float* rgb_bar, const float* rs,
                           int64_t M, int64_t Mp, float* gar, float* ga_last, float* fbar, float* nbar, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the SDF network including the double backward through d sdf/dx (what loss.backward() does through
 * mlp.py:84-143 with create_graph=True): sweep 1 = adjoint of the d sdf/dx chain, sweep 2 =
 * ordinary backward.  Upstream: sbar (M) d/d sdf, fbar (Mp,F) d/d feature (rows >= m_fbar are zero), nbar (M,3) d/d grad;
 * any of them may be NULL (= 0).  Emits the operands of the weight-gradient GEMMs:
 *   gus (L, Mp, H)  G(hbar_l) for l = 1..L-1 (slot 0 unused) ; gpbar (Mp,40) G(pbar) ;
 *   gas (L-1, Mp, H) G(a_l), l = 0..L-2 ; ga_last4 (Mp,4) {sbar,0,0,0} ; ones4 (Mp,4) {1,0,0,0}
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_sdf_backward(const i2sdf_plan* plan, const float* packed, const float* points, const float* cam, const float* dirs,
                       const float* z, int64_t ldz, int32_t n_per_ray, int64_t n_ray_pts, int64_t M, int64_t Mp,
                       const float* hs, const float* abars, const float* sbar, const float* fbar, int64_t m_fbar,
                       const float* nbar, float* gus, float* gpbar, float* gas, float* ga_last4, float* ones4, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray set-up -- utils/rend_util.py:92-147 (get_camera_params + lift, pose-matrix form) and
 * model/network/__init__.py:88-93 (per-pixel cam_loc, ||d||, F.normalize).
 *   uv (batch, pixels, 2) pixel coords ; pose (batch,4,4) cam->world ; intrinsics (batch,4,4)
 *   -> cam_loc (N,3), dirs (N,3) unit, dnorm (N) with N = batch*pixels
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_ray_setup(const float* uv, const float* pose, const float* intrinsics, int64_t batch, int32_t pixels,
                    float* cam_loc, float* dirs, float* dnorm, void* stream);
/* Same with the pose given as (batch,7) = [qr qi qj qk tx ty tz] when pose_is_quat != 0 (rend_util.py:93-98, quat_to_rot :150-167). */
int i2sdf_ray_setup_ex(const float* uv, const float* pose, int32_t pose_is_quat, const float* intrinsics, int64_t batch,
                       int32_t pixels, float* cam_loc, float* dirs, float* dnorm, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray batcher -- replaces ReconDataset.__getitem__ + collate_fn (dataset/train_dataset.py:169-209),
 * which stack one 4x4 K and one 4x4 pose PER RAY on the host, and the get_camera_params call that consumes them.
 * The camera tables and (optionally) the ground-truth images stay resident in HBM; a batch is a list of global pixel
 * indices tidx = image * (H*W) + pixel (what the DataLoader's sampler yields).  One pass writes the rays and gathers
 * the ground truth.  uv follows dataset/train_dataset.py:67-70: uv = (column, row) as floats.
 * Any table / output pointer except intrinsics, pose, cam_loc, dirs, dnorm may be NULL (skipped).
 * Dtypes follow the dataset: mask / light_mask are float images (:82,:96), depth_mask / normal_mask are bool bytes (:123,:163).
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_ray_tables {
  const float* intrinsics;         /* (n_images,4,4) */
  const float* pose;               /* (n_images,4,4) cam->world, or (n_images,7) when pose_is_quat */
  int32_t pose_is_quat;
  int32_t n_images, height, width;
  const float* rgb;                /* (n_images, H*W, 3) */
  const float* depth;              /* (n_images, H*W)    */
  const float* normal;             /* (n_images, H*W, 3) */
  const float* mask;               /* (n_images, H*W, 1) */
  const float* light_mask;         /* (n_images, H*W, 1) */
  const uint8_t* depth_mask;       /* (n_images, H*W)    */
  const uint8_t* normal_mask;      /* (n_images, H*W)    */
} i2sdf_ray_tables;

typedef struct i2sdf_ray_batch_out {
  int64_t* image_idx;              /* (n_rays)   tidx / (H*W) */
  float* uv;                       /* (n_rays,2) */
  float* cam_loc;                  /* (n_rays,3) */
  float* dirs;                     /* (n_rays,3) unit */
  float* dnorm;                    /* (n_rays)   */
  float* rgb;                      /* (n_rays,3) */
  float* depth;                    /* (n_rays)   */
  float* normal;                   /* (n_rays,3) */
  float* mask;                     /* (n_rays,1) */
  float* light_mask;               /* (n_rays,1) */
  uint8_t* depth_mask;             /* (n_rays)   */
  uint8_t* normal_mask;            /* (n_rays)   */
  int32_t* n_bad;                  /* NULL or device counter (caller-zeroed): += number of tidx outside [0, n_images*H*W); such rays
                                      are produced from the clamped index, nothing is read out of bounds */
} i2sdf_ray_batch_out;

int i2sdf_ray_batch(const i2sdf_ray_tables* tables, const int64_t* tidx, int64_t n_rays, const i2sdf_ray_batch_out* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray / bounding-sphere intersection -- utils/rend_util.py:211-227 (reached only with a background network).
 *   -> t_near_far (n_rays,2) = clamp(+-sqrt((d.o)^2 - (|o|^2 - r^2)) - d.o, min 0).  Where the reference prints and exit()s
 *   (non-positive discriminant) this entry writes (0,0) for the ray and increments *n_miss (device int32, caller-zeroed).
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_sphere_intersections(const float* cam_loc, const float* dirs, int64_t n_rays, float radius, float* t_near_far,
                               int32_t* n_miss, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Laplace density + log-space alpha compositing -- LaplaceDensity (density.py:21-30),
 * I2SDFNetwork.volume_rendering (model/network/__init__.py:223-240) and the weighted sums (:120-125,
 * :169, :204-219).  beta = |*beta_param| + beta_min is read on the device (no host sync).
 *   z (B, ldz): n sample depths followed by z_max in column n ; sdf (B*n) ; rgb (B*n,3) ;
 *   grad (B*n,3) raw d sdf/dx (needed iff o_normal) ; lmask (B*n) (needed iff o_lmask) ; dnorm (B)
 *   -> o_rgb (B,3), o_depth (B), o_wsum (B), o_normal (B,3)|NULL, o_lmask (B)|NULL,
 *      w_save (B,n)|NULL weights, nsum_save (B,3)|NULL un-normalised normal sum (for the backward)
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_composite_forward(const float* beta_param, float beta_min, const float* z, int64_t ldz, const float* sdf,
                            const float* rgb, const float* grad, const float* lmask, const float* dnorm, int64_t B, int32_t n,
                            float* o_rgb, float* o_depth, float* o_wsum, float* o_normal, float* o_lmask, float* w_save,
                            float* nsum_save, void* stream);

/* The same and i2sdf_eikonal_outputs_forward (below) in ONE launch -- the two per-ray launches of a training forward between the radiance
 * net and the loss: grad_all (3B,3) = d sdf / d x of the extra points [uniform | near | neighbour] -> grad_theta (2B,3), diff_norm (B). */
int i2sdf_composite_forward_eik(const float* beta_param, float beta_min, const float* z, int64_t ldz, const float* sdf,
                                const float* rgb, const float* grad, const float* lmask, const float* dnorm, int64_t B, int32_t n,
                                float* o_rgb, float* o_depth, float* o_wsum, float* o_normal, float* o_lmask, float* w_save,
                                float* nsum_save, const float* grad_all, float* grad_theta, float* diff_norm, void* stream);

/* Backward of the above (what loss.backward() does through :118-125,:169,:204-209).
 * Upstream: g_rgb (B,3), g_depth (B)|NULL, g_wsum (B)|NULL, g_normal (B,3)|NULL (w.r.t. normal_values),
 * g_lmask (B)|NULL.  The normal / light composites use w.detach() as the reference does in training.
 *   -> sdf_bar (B*n), rgb_bar (B*n,3), grad_bar (B*n,3)|NULL, lmask_bar (B*n)|NULL,
 *      beta_partial (B) scratch; if beta_grad_accum != NULL: *beta_grad_accum += d loss / d density.beta */
int i2sdf_composite_backward(const float* beta_param, float beta_min, const float* z, int64_t ldz, const float* sdf,
                             const float* rgb, const float* grad, const float* dnorm, const float* nsum_save, int64_t B, int32_t n,
                             const float* g_rgb, const float* g_depth, const float* g_wsum, const float* g_normal,
                             const float* g_lmask, float* sdf_bar, float* rgb_bar, float* grad_bar, float* lmask_bar,
                             float* beta_partial, float* beta_grad_accum, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Weight gradients: the dW = G^T U GEMMs of every nn.Linear (autograd's mm/addmm backward nodes for mlp.py:97,222),
 * reduced over all points, then the weight-norm backward (d/dg, d/dv of W = g v/||v||) and bias gradients, written
 * into `grad_flat` (same layout as `params`; entries of nets that took no part are left untouched).
 * All pointers are the per-point workspaces the kernels above produced ([Mp][ld], see their comments).
 * Every one of them has Mp rows, Mp a multiple of 128 (as the producing kernels require): the bf16x3 kernel reads whole 16-point
 * stages, i.e. up to 15 rows past M_sdf / M_main, and masks them -- the padding rows may hold anything but must exist.
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_train_buffers {
  int64_t M_sdf;    /* points that went through the SDF network (render + eikonal + bubble points) */
  int64_t M_main;   /* leading points that also went through the radiance (and light) network        */
  int64_t Mp;
  const float *pe, *hs, *abars, *gus, *gpbar, *gas, *ga_last4, *ones4, *fbar;   /* SDF network   */
  const float *pev, *feat, *rs, *gar, *ga_last_rgb;                             /* radiance net  */
  const float *hl, *gal0, *gal_last;                                            /* light head (NULL if absent) */
} i2sdf_train_buffers;

int64_t i2sdf_wgrad_chunk_points(void);   /* points per split-M chunk: partials needs ceil(M_sdf/chunk) * wgrad_floats floats */
int i2sdf_weight_grads(const i2sdf_plan* plan, const i2sdf_train_buffers* bufs, const float* params, float* partials,
                       int64_t n_chunks_cap, float* grad_flat, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Data parallelism (the reference itself is single-GPU: main_recon.py:111-112).  One process per GPU; rays
 * are sharded, parameters replicated, and the only exchange of a training step is the parameter-gradient mean over the flat
 * buffer -- RCCL over xGMI.  RCCL is bound at run time (librccl.so.1); without it these calls return I2SDF_ECOMM.
 *   i2sdf_comm_unique_id : rank 0 makes the 128-byte id, the caller distributes it (any side channel)
 *   i2sdf_comm_init_rank : collective over all ranks; the calling thread's current HIP device is the rank's GPU
 *   i2sdf_allreduce_grads: in place, stream ordered, every rank ends with the MEAN over ranks (DDP convention)
 *   i2sdf_allreduce_max_i32 / i2sdf_broadcast: the small exchanges of 1-GPU-equivalent mode (below)
 * 1-GPU-equivalent mode: besides the gradient mean, a sharded step needs two SMALL exchanges to equal the single-GPU step on
 * the concatenated batch.  They go through an `i2sdf_exchange` hook (an in-place all-reduce of a few device words, enqueued on
 * the stream, never synchronising the host): i2sdf_comm_as_exchange() gives the RCCL implementation; a caller may supply its
 * own (i2sdf_amd/dist.py routes it through torch.distributed for gloo tests).
 *   i2sdf_plan_set_exchange(plan, ex, I2SDF_DP_GLOBAL_SAMPLER): the sampler's convergence test becomes the batch-global OR over
 *     ALL ranks' rays (ray_sampler.py:151: while any ray of the batch is unconverged every ray is up-sampled) -- one 4-byte MAX
 *     all-reduce per iteration;
 *   i2sdf_loss_cfg.exchange: every loss denominator (B, n_pc, masked-mean counts, model/network/__init__.py:320-336) becomes its
 *     mean over the ranks, so that the mean over ranks of the per-rank gradients is the gradient on the concatenated batch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_comm i2sdf_comm;
#define I2SDF_COMM_UNIQUE_ID_BYTES 128
#define I2SDF_DP_GLOBAL_SAMPLER 1
#define I2SDF_XCHG_F32 0
#define I2SDF_XCHG_I32 1
#define I2SDF_XCHG_SUM 0
#define I2SDF_XCHG_AVG 1
#define I2SDF_XCHG_MAX 2
typedef struct i2sdf_exchange {
  /* in-place all-reduce of n elements at device pointer buf, ordered on `stream`; returns 0 or a negative error code */
  int (*allreduce)(void* ctx, void* buf, int64_t n, int32_t dtype, int32_t op, void* stream);
  void* ctx;
} i2sdf_exchange;
int32_t i2sdf_comm_available(void);       /* 1 if RCCL could be bound in this process (creates nothing): agree on it across ranks before i2sdf_comm_init_rank */
int i2sdf_comm_unique_id(void* out, int64_t out_bytes);
int i2sdf_comm_init_rank(const void* unique_id, int32_t nranks, int32_t rank, i2sdf_comm** out);
void i2sdf_comm_destroy(i2sdf_comm* comm);
int32_t i2sdf_comm_size(const i2sdf_comm* comm);
int32_t i2sdf_comm_rank(const i2sdf_comm* comm);
const char* i2sdf_last_comm_error(void);
int i2sdf_allreduce_grads(float* flat, int64_t n, const i2sdf_comm* comm, void* stream);
int i2sdf_allreduce_max_i32(int32_t* flags, int64_t n, const i2sdf_comm* comm, void* stream);
int i2sdf_broadcast(void* buf, int64_t bytes, int32_t root, const i2sdf_comm* comm, void* stream);
int i2sdf_comm_as_exchange(const i2sdf_comm* comm, i2sdf_exchange* out);
int i2sdf_plan_set_exchange(i2sdf_plan* plan, const i2sdf_exchange* ex, int32_t flags);   /* ex = NULL detaches; *ex is copied */

/* ------------------------------------------------------------------------------------------------
 * Optimizer step over the flat parameter buffer -- torch.optim.Adam(model.get_param_groups(lr), eps=1e-15) of
 * model/trainer/recon.py:201-203 (same update rule and operation order, bias corrections in double on the host) as ONE
 * launch.  step = 1 for the first update.  grad_scale multiplies the gradient first (1/world for a summed all-reduce).
 *   params, grads, exp_avg, exp_avg_sq: (n) fp32, updated in place (grads is read-only)
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int64_t step, double grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Error-bounded ray sampler -- ErrorBoundSampler.get_z_vals incl. UniformSampler and get_error_bound
 * (model/network/ray_sampler.py:22-43,67-251), bg disabled.  Runs the whole Algorithm-1 loop on the device:
 * all max_total_iters iterations are enqueued, a device flag turns the remaining ones into no-ops once the
 * batch-global test `beta.max() > beta0` (ray_sampler.py:151) fails, so there is no host synchronisation.
 * Random draws are inputs (training): strat_u (B,N_eval) [:39], u_final (B,N_samples) [:190],
 * extra_idx (max_total_iters, N_extra): row it-1 = randperm(N_eval*it)[:N_extra], the draw for a loop that ran `it`
 * iterations [:223] (the row length is only known on the device), eik_idx (B) [:233].  Deterministic tables (eval and the
 * error-proportional up-sampling): t_lin = linspace(0,1,N_eval) [:30], u_more = linspace(0,1,N_eval) [:188],
 * u_final = linspace(0,1,N_samples) with ldu_final = 0 [:188], extra_tab (max_total_iters, N_extra) =
 * linspace(0, N_eval*(it+1)-1, N_extra).long() per possible row length [:225].
 *   force_iters > 0 replaces the data-dependent test by "exactly force_iters iterations" (fixed-work benchmarks).
 *   -> z_out (B, ldz): N_samples + N_extra + 2 sorted depths (last = far) ; z_eik (B)|NULL ; iters_out device int|NULL
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_sampler_cfg {
  float near, eps, add_tiny;
  int32_t N_samples, N_samples_eval, N_samples_extra, beta_iters, max_total_iters;
} i2sdf_sampler_cfg;

/* ErrorBoundSampler.get_error_bound (model/network/ray_sampler.py:243-251) and the Theorem-1 distance bound d* of
 * get_z_vals (:99-114) on caller-provided rows -- the device functions the Algorithm-1 loop uses, as their own entry point.
 *   z, sdf (B,n) sorted depths / sdf values, 2 <= n <= 640 ; beta: one value (ldbeta = 0) or one per ray (ldbeta = 1)
 *   d_star_in (B,n-1)|NULL: use these bounds instead of computing them ; d_star_out (B,n-1)|NULL ; bound (B)|NULL
 *   -> bound[r] = max_i (min(exp(cumsum err)_i, 1e6) - 1) * exp(-integral_i)                                       */
int i2sdf_error_bound(const float* z, const float* sdf, int64_t B, int32_t n, const float* beta, int64_t ldbeta,
                      const float* d_star_in, float* d_star_out, float* bound, void* stream);

/* The workspace of i2sdf_sample_rays, in floats.  Its layout is what the stage tests read (tests/sampler_ref.py), so it is fixed:
 * six row buffers of B*640 -- depths zA, zB, sdf values sA, sB, int32 merge indices iA, iB (iteration it, counted from 0, reads its row
 * from zA/sA when `it` is even and from zB/sB when odd, with the indices that produced it in iB / iA) --, then `samples` (B rows of 128:
 * the last inverse-CDF output), `sdf_new` (B*128 reserved, written packed as B rows of N_samples_eval), `beta` (B), 32 int32 state
 * words (0: done, 1: iterations run, 2+it: beta > beta0 seen, 16+it: workgroups finished) and 64 spare floats.  Entries of a row past
 * its current length, columns of `samples` past max(N_samples_eval, N_samples) and the spare floats are never written.           */
int64_t i2sdf_sampler_workspace_floats(int64_t B);
int i2sdf_sample_rays(const i2sdf_plan* plan, const float* packed, const float* params, const i2sdf_sampler_cfg* cfg,
                      const float* cam, const float* dirs, int64_t B, int32_t training, const float* t_lin, const float* u_more,
                      const float* u_final, int64_t ldu_final, const int32_t* extra_tab, const float* strat_u,
                      const int32_t* extra_idx, const int32_t* eik_idx, int32_t force_iters, float* workspace, float* z_out,
                      int64_t ldz, float* z_eik, int32_t* iters_out, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Light-mask head -- model/network/__init__.py:29-32,162-170:
 * lm = sigmoid(W1 softplus100(W0 relu(feature).detach() + b0) + b1).  Backward stops at the head's parameters
 * (detach_light_feature = True, the reference default).
 *   forward : feat (Mp,F) -> lm (M), hl (Mp,HL) softplus activations (NULL if no backward follows)
 *   backward: lm_bar (M) -> gal0 (Mp,HL) G(a_0), gal_last (Mp,4) {G(a_1),0,0,0}   (weight-gradient operands)
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_light_forward(const i2sdf_plan* plan, const float* packed, const float* feat, int64_t M, int64_t Mp, float* lm, float* hl,
                        void* stream);
int i2sdf_light_backward(const i2sdf_plan* plan, const float* packed, const float* lm, const float* lm_bar, const float* hl, int64_t M,
                         int64_t Mp, float* gal0, float* gal_last, void* stream);


/* ------------------------------------------------------------------------------------------------
 * I2SDFLoss -- model/network/__init__.py:289-406 -- value AND gradient w.r.t. every render output in one call
 * (SURVEY.md "next" row N1).  Per-ray tensors as returned by the module: rgb (B,3), depth (B), wsum (B),
 * normal (B,3)|NULL, grad_theta (2B,3)|NULL, diff_norm (B)|NULL, surface (n_pc)|NULL, lmask (B)|NULL; ground truth
 * gt_rgb (B,3), gt_depth (B)+depth_mask (B bytes)|NULL, gt_normal (B,3)+normal_mask|NULL, gt_mask (B)|NULL,
 * gt_lmask (B)|NULL.  `smooth_on` = the reference's `smooth_iter is None or step > smooth_iter` (:347).
 *   -> losses[10] = {loss, rgb, eikonal, smooth, mask, depth, normal, angular, bubble, light_mask} (device), loss_value (1)|NULL = the
 *      total once more as a tensor of its own (a scalar for autograd without a select on the vector),
 *      g_* = d loss / d (same-named input); scratch: i2sdf_loss_scratch_floats() floats of workspace, contents irrelevant on entry
 *      (nothing persists in it between calls: no counter, nothing to zero; calls in flight on DIFFERENT streams need different
 *      scratch buffers, calls on one stream can share one).
 *   Two launches: per-block partial sums; then the reported values + every gradient, where every workgroup first adds the block
 *   partials up itself, in block order (deterministic, no atomics).  With an exchange hook a one-workgroup reduction and the hook's
 *   collective sit between the two.
 * ---------------------------------------------------------------------------------------------- */
typedef struct i2sdf_loss_cfg {
  float eikonal_w, smooth_w, mask_w, depth_w, normal_w, angular_w, bubble_w, light_w;
  int32_t smooth_on;
  int32_t reserved;
  const i2sdf_exchange* exchange;  /* NULL, or: every denominator (B, n_pc, mask counts) becomes its mean over the ranks, so that the
                                      mean over ranks of the per-rank gradients is the gradient on the concatenated batch */
} i2sdf_loss_cfg;

int64_t i2sdf_loss_scratch_floats(void);
int i2sdf_loss_forward_backward(const i2sdf_loss_cfg* cfg, int64_t B, int64_t n_pc, const float* rgb, const float* depth,
                                const float* wsum, const float* normal, const float* grad_theta, const float* diff_norm,
                                const float* surface, const float* lmask, const float* gt_rgb, const float* gt_depth,
                                const uint8_t* depth_mask, const float* gt_normal, const uint8_t* normal_mask, const float* gt_mask,
                                const float* gt_lmask, float* scratch, float* losses, float* loss_value, float* g_rgb, float* g_depth, float* g_wsum,
                                float* g_normal, float* g_grad_theta, float* g_diff_norm, float* g_surface, float* g_lmask,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Eikonal / smoothness outputs -- model/network/__init__.py:188-193.  grad_all (3B,3) = d sdf/dx at the extra points
 * [B uniform | B near-surface | B neighbours] (the tail of i2sdf_sdf_forward_grad's `grad`):
 *   forward : grad_theta (2B,3)|NULL = rows [0,2B) (:189);  diff_norm (B) = ||normalize(g[B+i]) - normalize(g[2B+i])||,
 *             normalize = F.normalize(dim=1, eps=1e-6) (:190-192)
 *   backward: grad_theta_bar (2B,3)|NULL, diff_norm_bar (B)|NULL -> grad_all_bar (3B,3), every row written
 *             (torch's conventions: d||x|| = 0 at x = 0, no gradient through a norm below eps).
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_eikonal_outputs_forward(const float* grad_all, int64_t B, float* grad_theta, float* diff_norm, void* stream);
int i2sdf_eikonal_outputs_backward(const float* grad_all, const float* grad_theta_bar, const float* diff_norm_bar, int64_t B,
                                   float* grad_all_bar, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The extra points of a training step -- model/network/__init__.py:175-186 -- in one launch instead of a multiply, two adds and a
 * concatenation:  out (3B,3) = [ eik_pts (B,3) | cam + z_eik * dirs (B,3) | the same + nbr_off (B,3) ],  z_eik (B) the per-ray depth
 * i2sdf_sample_rays returned, the sum rounded as the reference's two fp32 operations (product, then sum; no fused multiply-add).
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_extra_points(const float* cam, const float* dirs, const float* z_eik, const float* eik_pts, const float* nbr_off, int64_t B,
                       float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Seeds of the backward pass (what autograd's accumulation does with a handful of fills and copies), one launch:
 *   beta_grad[0, n_beta) = 0                                   (i2sdf_composite_backward accumulates d loss / d beta into it)
 *   sdf_bar (M_sdf)    : rows [M_main, M_sdf) = 0, except rows [M_main + n_eik, M_main + n_eik + n_pc) = g_surf (n_pc)|NULL
 *   grad_bar (M_sdf,3) : rows [M_main, M_sdf) = 0, except rows [M_main, M_main + n_eik) = g_eik (n_eik,3)|NULL;
 *                        rows [0, M_main) = 0 too iff zero_main_grad (no normal output: the compositing backward does not write them)
 * The rays' rows [0, M_main) of sdf_bar (and of grad_bar otherwise) are left to i2sdf_composite_backward, which writes all of them.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_backward_seeds(float* beta_grad, int64_t n_beta, float* sdf_bar, float* grad_bar, int64_t M_main, int64_t M_sdf,
                         const float* g_eik, int64_t n_eik, const float* g_surf, int64_t n_pc, int32_t zero_main_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Loss + render backward fused (round 6): I2SDFLoss -- model/network/__init__.py:289-406 -- evaluated on the outputs of a TRAINING render,
 * together with the backward of everything between those outputs and the per-sample gradients the MLP backward starts from: the
 * compositing backward (:223-240,:120-125,:169,:204-219), the backward of the eikonal / smoothness outputs (:188-193) and the seeds of the
 * extra points.  Replaces i2sdf_loss_forward_backward + i2sdf_eikonal_outputs_backward + i2sdf_backward_seeds + i2sdf_composite_backward
 * (seven launches and, in between, two of autograd's own) by two launches, for an upstream gradient of 1; i2sdf_scale_seeds multiplies the
 * results by the gradient autograd delivers.  No data-parallel exchange hook here (cfg->exchange must be NULL: use the separate entry points).
 *   batch layout as in i2sdf_backward_seeds: M_main = B n ray samples, then n_eik (= 3 B or 0) extra points [uniform | near | neighbour],
 *     then n_pc bubble points (iff surface), M_sdf rows in all
 *   compositing inputs as in i2sdf_composite_backward: beta_param, z (B, ldz), sdf (M_sdf), rgb_pts (M_main,3), grad_pts (M_sdf,3)|NULL
 *     (d sdf / d x of every point: needed iff normal_term or n_eik), dnorm (B), nsum_save (B,3)|NULL (iff normal_term)
 *   render outputs / ground truth as in i2sdf_loss_forward_backward (grad_theta (2B,3) and diff_norm (B) iff n_eik; surface (n_pc)|NULL)
 *   -> losses (10), loss_value (1)|NULL, the output seeds g_* (as i2sdf_loss_forward_backward writes them),
 *      sdf_bar (M_sdf), rgb_bar (M_main,3), grad_bar (M_sdf,3) -- every row written; normal_term = 0: the ray samples' rows are zeros --,
 *      lmask_bar (M_main)|NULL, beta_grad (1) = d loss / d beta_param;  scratch: i2sdf_render_loss_scratch_floats(B) floats
 * ---------------------------------------------------------------------------------------------- */
int64_t i2sdf_render_loss_scratch_floats(int64_t B);
int i2sdf_render_loss_backward(const i2sdf_loss_cfg* cfg, int64_t B, int32_t n, int64_t n_pc, int64_t M_main, int64_t M_sdf, int64_t n_eik,
                               const float* beta_param, float beta_min, const float* z, int64_t ldz, const float* sdf, const float* rgb_pts,
                               const float* grad_pts, const float* dnorm, const float* nsum_save,
                               const float* rgb, const float* depth, const float* wsum, const float* normal, const float* grad_theta,
                               const float* diff_norm, const float* surface, const float* lmask,
                               const float* gt_rgb, const float* gt_depth, const uint8_t* depth_mask, const float* gt_normal,
                               const uint8_t* normal_mask, const float* gt_mask, const float* gt_lmask,
                               float* scratch, float* losses, float* loss_value,
                               float* g_rgb, float* g_depth, float* g_wsum, float* g_normal, float* g_grad_theta, float* g_diff_norm,
                               float* g_surface, float* g_lmask,
                               float* sdf_bar, float* rgb_bar, float* grad_bar, int32_t normal_term, float* lmask_bar, float* beta_grad,
                               void* stream);
/* x *= g[0] for the four per-sample gradient tensors (n_* = their float counts; a pointer may be NULL with a count of 0) and
 * beta_out[0] = beta_in[0] * g[0] (beta_out may be NULL); g = a device scalar (the gradient of the loss value autograd delivers). */
int i2sdf_scale_seeds(const float* g, float* sdf_bar, int64_t n_sdf, float* grad_bar, int64_t n_grad, float* rgb_bar, int64_t n_rgb,
                      float* lmask_bar, int64_t n_lmask, const float* beta_in, float* beta_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Full-image inference in one call -- the chunk loop of utils.split_input / model(chunk) /
 * utils.merge_output (utils/__init__.py:35-84) as used by model/eval/recon.py:161-182 and the plotting callbacks: eval mode,
 * `chunk` = split_n_pixels rays at a time, every chunk rendered exactly as the reference renders it (the sampler's convergence
 * test is per chunk), outputs written straight into the (P, C) image-order tensors.  Enqueues all chunks on `stream` without
 * allocating or synchronising; one chunk-sized workspace (i2sdf_render_image_workspace_floats) is reused by every chunk.
 *   uv (P,2) pixel coordinates of ONE view; pose (4,4) or (7); intrinsics (4,4); tables as for i2sdf_sample_rays (eval)
 *   -> o_rgb (P,3), o_depth (P), o_wsum (P), o_normal (P,3)|NULL = normal_map, o_lmask (P) (required iff the plan has a light
 *      head), o_z (P, N_samples+N_extra+2)|NULL the depths used, o_iters (ceil(P/chunk)) device ints|NULL sampler iterations
 * ---------------------------------------------------------------------------------------------- */
int64_t i2sdf_render_image_workspace_floats(const i2sdf_plan* plan, const i2sdf_sampler_cfg* cfg, int64_t chunk);
int i2sdf_render_image(const i2sdf_plan* plan, const float* packed, const float* params, const i2sdf_sampler_cfg* cfg,
                       const float* uv, const float* pose, int32_t pose_is_quat, const float* intrinsics, int64_t P, int64_t chunk,
                       const float* t_lin, const float* u_more, const float* u_final, const int32_t* extra_tab, float* workspace,
                       float* o_rgb, float* o_depth, float* o_wsum, float* o_normal, float* o_lmask, float* o_z, int32_t* o_iters,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * SDF volume for marching cubes -- model/eval/recon.py:46-51 (coarse uniform grid) and :75-103 (the
 * PCA-aligned fine grid evaluated through GridDataset / a 32-worker DataLoader), utils/plots.py:440-489 (get_grid_uniform,
 * get_grid: np.meshgrid(x, y, z) flattened to an (n,3) host tensor).  The axis vectors are the whole input: grid points are
 * generated on the device one chunk ahead of the SDF kernel and never exist on the host.
 *   x (nx), y (ny), z (nz)   device fp32 axis coordinates (the reference casts its float64 linspace / arange to float)
 *   order   I2SDF_GRID_ORDER_MESHGRID: output index ((iy*nx)+ix)*nz+iz = np.meshgrid(x,y,z).ravel() order, the order of the
 *           reference's flat `z` before its reshape(ny,nx,nz).transpose([1,0,2]);  I2SDF_GRID_ORDER_VOLUME: ((ix*ny)+iy)*nz+iz,
 *           i.e. that transposed (nx,ny,nz) volume itself, ready for measure.marching_cubes
 *   rot (9, row-major, HOST) | NULL, trans (3, HOST) | NULL : evaluated point = rot * (x,y,z) + trans; the aligned grid of
 *           model/eval/recon.py:82-85 passes rot = vecs^T, trans = s_mean
 *   [first, first+count) the output indices to evaluate (a rank's slab; count = nx*ny*nz for everything)
 *   sdf_out (count); workspace i2sdf_sdf_grid_workspace_floats(chunk_points) floats; chunk_points > 0
 * Enqueues ceil(count/chunk_points) generator + SDF launches on `stream`; no allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_GRID_ORDER_MESHGRID 0
#define I2SDF_GRID_ORDER_VOLUME 1
int64_t i2sdf_sdf_grid_workspace_floats(int64_t chunk_points);
int i2sdf_sdf_grid(const i2sdf_plan* plan, const float* packed, const float* x, const float* y, const float* z, int32_t nx,
                   int32_t ny, int32_t nz, int32_t order, const float* rot, const float* trans, int64_t first, int64_t count,
                   float* sdf_out, float* workspace, int64_t chunk_points, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Marching cubes -- the zero-level mesh of an SDF volume (model/eval/recon.py:53-60,91-95, utils/plots.py:197-206 run
 * skimage.measure.marching_cubes on the host).  vol (nx, ny, nz) device fp32, z fastest (I2SDF_GRID_ORDER_VOLUME); every
 * axis >= 2 points.  A corner is above iff v > level (NaN is not above); the case tables are derived by
 * i2sdf_amd/csrc/gen_mc_tables.py (ambiguous faces keep their above-level corners apart; no interior vertices).
 *   one vertex per lattice edge whose ends straddle the level, in order of (lattice-point linear index, axis x < y < z):
 *     verts   = origin + (i + t e) * spacing,  t = (level - v0) / (v1 - v0)                                 (V, 3) fp32
 *     normals = -normalize((1 - t) g0 + t g1), g = np.gradient(vol, *spacing) at the edge's ends         (V, 3) fp32
 *               (they point towards decreasing values, as scikit-image's do)
 *   faces  (F, 3) int32 vertex indices, in order of (cell linear index, table slot); the right-hand face normal points
 *          towards increasing values; the mesh is closed away from the volume's border.
 * Two calls on the same stream, one workspace of i2sdf_marching_cubes_workspace_bytes(nx, ny, nz) bytes (0: shape not
 * supported; it holds 5 bytes per lattice point):
 *   _count  enqueues the classification and scan; counts_out (device int64[2]) | NULL <- (V, F).
 *   _emit   same vol / level / workspace; reads (V, F) back (one stream synchronisation) and returns I2SDF_EINVAL when either
 *           exceeds INT32_MAX, I2SDF_EWORKSPACE when cap_v < V or cap_f < F, before anything is written; otherwise enqueues the
 *           emission.  spacing[3], origin[3] are HOST arrays.  Nothing is allocated.
 * ---------------------------------------------------------------------------------------------- */
int64_t i2sdf_marching_cubes_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int i2sdf_marching_cubes_count(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, void* workspace, int64_t* counts_out,
                               void* stream);
int i2sdf_marching_cubes_emit(const float* vol, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing,
                              const float* origin, void* workspace, float* verts, float* normals, int32_t* faces, int64_t cap_v,
                              int64_t cap_f, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh operations (csrc/meshops.hip) -- what the reference runs through trimesh on the host between its two marching-cubes
 * passes (utils/plots.py:280-297, model/eval/recon.py:61-71): split into components, keep the one with the largest area, draw
 * area-weighted surface points.  verts / normals (V, 3) fp32, faces (F, 3) int32, all device; F, V <= INT32_MAX (else
 * I2SDF_EINVAL); F = 0 is a no-op.  Every call only enqueues on `stream` (no allocation, no synchronisation) except
 * i2sdf_mesh_status.  Results are bitwise reproducible: no float atomics, fixed summation order.
 *   status   device int32 word, zeroed by the caller: a face with a vertex index outside [0, V) is never dereferenced; it
 *            sets the word instead (such a face has area 0, is connected to nothing and is dropped by the compaction).
 *            i2sdf_mesh_status copies it back (one stream synchronisation): I2SDF_EINVAL when set.
 *   _edge_keys         keys[3f + c] = min(a, b) << 32 | max(a, b) for side c = (v_c, v_{c+1}) of face f           (3F) int64
 *   _face_components   Two faces are connected when they share an edge (an unordered vertex pair), ALSO when three or more
 *                      faces share it (trimesh's face_adjacency ignores such edges); sharing one vertex does not connect.
 *                      The CALLER sorts the keys: sorted_keys (3F) ascending, perm (3F) int64 the position each sorted entry
 *                      came from (entry / 3 = its face).  labels[f] <- the smallest face index of f's component   (F) int32
 *   _face_areas        area[f] = 0.5 |(v1 - v0) x (v2 - v0)|, fp32, products and sums rounded separately          (F) fp32
 *   _cumsum_f64        cdf[i] = sum_{j <= i} (double) x[order[j]] (order NULL: x[j]; entries outside [0, n_x) count 0), a
 *                      reduce-then-scan in a fixed order; workspace of i2sdf_mesh_scan_workspace_bytes(n) bytes    (n) fp64
 *   _largest_label     sorted_labels (F) ascending (a STABLE sort of the labels by the caller), cdf the running sum of the
 *                      areas in that order.  best[0] <- bit pattern of the largest component area, best[1] <- its label
 *                      (ties: the smaller label); (0, INT64_MAX) for F = 0                                  device int64[2]
 *   _compact_mark      fkeep[f] <- mask[f] != 0 (mask: F bytes) and valid; vflag[v] <- 1 iff a kept face uses v   (F), (V) int32
 *   _compact_gather    fscan / vscan = INCLUSIVE int32 running sums of fkeep / vflag (by the caller, who reads their last
 *                      entries to size the outputs).  Kept faces in their order, re-indexed; used vertices (and normals, may be
 *                      NULL) in their order.  Rows beyond cap_f / cap_v are not written.
 *   _sample_surface    trimesh.sample.sample_surface with the caller's uniform draws u_face (count), u_bary (count, 2) in [0, 1):
 *                      pick = u_face * cdf[F-1]; face = first i with cdf[i] >= pick (np.searchsorted side='left'), at most F-1;
 *                      (a, b) = u_bary, reflected to (|a-1|, |b-1|) when a + b > 1; point = v0 + a (v1-v0) + b (v2-v0) in fp32.
 *                      cdf = _cumsum_f64 of _face_areas.  count > 0 with F = 0 is I2SDF_EINVAL.
 * ---------------------------------------------------------------------------------------------- */
int64_t i2sdf_mesh_scan_workspace_bytes(int64_t n);
int i2sdf_mesh_status(const int32_t* status, void* stream);
int i2sdf_mesh_edge_keys(const int32_t* faces, int64_t F, int64_t n_verts, int64_t* keys, int32_t* status, void* stream);
int i2sdf_mesh_face_components(const int64_t* sorted_keys, const int64_t* perm, int64_t F, int32_t* labels, void* stream);
int i2sdf_mesh_face_areas(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, float* area, int32_t* status,
                          void* stream);
int i2sdf_mesh_cumsum_f64(const float* x, int64_t n_x, const int64_t* order, int64_t n, double* cdf, void* workspace, void* stream);
int i2sdf_mesh_largest_label(const int32_t* sorted_labels, const double* cdf, int64_t F, int64_t* best, void* stream);
int i2sdf_mesh_compact_mark(const int32_t* faces, const uint8_t* mask, int64_t F, int64_t n_verts, int32_t* fkeep, int32_t* vflag,
                            int32_t* status, void* stream);
int i2sdf_mesh_compact_gather(const float* verts, const float* normals, int64_t n_verts, const int32_t* faces, int64_t F,
                              const int32_t* fkeep, const int32_t* fscan, const int32_t* vflag, const int32_t* vscan,
                              float* out_verts, float* out_normals, int32_t* out_faces, int64_t cap_v, int64_t cap_f, void* stream);
int i2sdf_mesh_sample_surface(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, const double* cdf,
                              const float* u_face, const float* u_bary, int64_t count, float* points, int32_t* face_index,
                              int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-set operations (csrc/pointops.hip) -- the scoring step after the mesh export (utils/mesh_util.py:evaluate, called by
 * model/eval/recon.py:111-129, where open3d and a scikit-learn KDTree run on the host): voxel down-sampling, exact nearest
 * neighbours, thresholded means.  points / query / ref (n, 3) fp32, device; counts <= INT32_MAX (else I2SDF_EINVAL).  Every call
 * only enqueues on `stream`: no allocation, no synchronisation; arguments are validated on the host before any launch.  Results
 * are bitwise reproducible: integer atomics only, fp64 sums in a fixed order.
 *   status   device int32[2], zeroed by the caller.  status[0]: bit 0 <- a non-finite coordinate, bit 1 <- a voxel index that
 *            does not fit 21 bits; status[1]: the number of queries handed to the fallback pass.  The caller reads it back.
 *   bounds   device int32[8], opaque: the per-axis minima / maxima of the finite coordinates.
 *   _bounds            bounds <- those of points (n may be 0)
 *   _voxel_keys        open3d's VoxelDownSample rule in fp64: lo = min - voxel_size / 2, index = floor((p - lo) / voxel_size) per
 *                      axis, keys[i] = ix << 42 | iy << 21 | iz (INT64_MAX and a status bit for a point that has no key).
 *                      voxel_size must be positive and finite                                                          (n) int64
 *   _voxel_heads       sorted_keys (n) ascending, a STABLE sort by the caller: heads[i] = 1 where a run of equal keys begins  (n) int32
 *   _voxel_mean        perm (n) int64 = the position each sorted entry came from, head_scan = INCLUSIVE int32 running sum of
 *                      heads (by the caller, whose last entry M sizes the outputs).  Voxel m (in ascending key order, that is
 *                      (ix, iy, iz) lexicographic): out_points[m] = fp32(fp64 sum of its points in original index order / count),
 *                      out_counts[m] = count.  Voxels beyond cap_m are not written                       (M, 3) fp32, (M) int32
 *   _grid_keys         hashes ref into a uniform grid over its bounding box, described at the head of `workspace`
 *                      (i2sdf_points_grid_workspace_bytes(n_ref) bytes, 0 for n_ref outside [1, INT32_MAX]): about 2 cells per
 *                      point, at most 1024 per axis and 2^22 in all -- the cell is enlarged until the grid fits the tables, whatever
 *                      the bounding box.  keys[i] = linear cell of ref[i]                                          (n_ref) int64
 *   _grid_build        sorted_keys / perm: the caller's STABLE sort of those keys.  Fills the cell start / end tables in
 *                      `workspace` and sorted_ref[i] = (x, y, z, bits of the original index) of sorted entry i  (n_ref, 4) fp32
 *   _nn_query          one query per lane: shells of cells of growing Chebyshev radius r <= max_ring around the query's cell
 *                      (clamped into the grid); ends once the best distance is within r cells or the shells cover the grid.
 *                      dist[q] = fp32 Euclidean distance (fp32 differences, squares and sums rounded separately), index[q] = the
 *                      reference index, the smallest among equal distances.  A query that exhausts max_ring gets a provisional
 *                      answer and is appended to fallback_list (n_query) int32, counted in status[1].  A non-finite query sets
 *                      status[0] and gets (NaN, -1)                                             (n_query) fp32, (n_query) int32
 *   _nn_fallback       answers the status[1] listed queries exactly: one wave per query over all of ref (original order)
 *   _threshold_reduce  out[0] = fp64 sum of dist, out[1] = count(dist < threshold) as fp64, in a fixed order; workspace of
 *                      i2sdf_points_reduce_workspace_bytes(n) bytes; n >= 1                                     device fp64[2]
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_points_bounds(const float* points, int64_t n, int32_t* bounds, int32_t* status, void* stream);
int i2sdf_points_voxel_keys(const float* points, int64_t n, const int32_t* bounds, double voxel_size, int64_t* keys, int32_t* status,
                            void* stream);
int i2sdf_points_voxel_heads(const int64_t* sorted_keys, int64_t n, int32_t* heads, void* stream);
int i2sdf_points_voxel_mean(const float* points, int64_t n, const int64_t* sorted_keys, const int64_t* perm, const int32_t* head_scan,
                            float* out_points, int32_t* out_counts, int64_t cap_m, void* stream);
int64_t i2sdf_points_grid_workspace_bytes(int64_t n_ref);
int i2sdf_points_grid_keys(const float* ref, int64_t n_ref, void* workspace, int64_t* keys, int32_t* status, void* stream);
int i2sdf_points_grid_build(const float* ref, int64_t n_ref, const int64_t* sorted_keys, const int64_t* perm, void* workspace,
                            float* sorted_ref, void* stream);
int i2sdf_points_nn_query(const float* query, int64_t n_query, const float* sorted_ref, int64_t n_ref, const void* workspace,
                          int32_t max_ring, float* dist, int32_t* index, int32_t* fallback_list, int32_t* status, void* stream);
int i2sdf_points_nn_fallback(const float* query, int64_t n_query, const float* ref, int64_t n_ref, const int32_t* fallback_list,
                             const int32_t* status, float* dist, int32_t* index, void* stream);
int64_t i2sdf_points_reduce_workspace_bytes(int64_t n);
int i2sdf_points_threshold_reduce(const float* dist, int64_t n, double threshold, void* workspace, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh depth (csrc/raster.hip) -- the depth render of utils/mesh_util.py:refuse (pyrender on EGL in the reference): for every
 * camera the camera-space z of the nearest triangle along each pixel's ray.  Cameras look along +z with x right and y down
 * (rend_util.load_K_Rt_from_P); the sample of pixel (column u, row v) is the ray through ((u - cx) / fx, (v - cy) / fy, 1).
 *   verts (V, 3) fp32, faces (F, 3) int32, device; V, F <= INT32_MAX.  w2c (n_cam, 3, 4) fp32 device: world-to-camera rows.
 *   K4 = (fx, fy, cx, cy), a HOST array; fx, fy > 0.  H, W >= 1, H W <= INT32_MAX; n_cam <= 65535.  0 < znear <= zfar < inf.
 *   cull 1: triangles whose right-hand normal points away from the camera (clockwise as the camera sees them) are dropped; 0: kept.
 *   depth (n_cam, H, W) fp32 <- z of the nearest covered sample with znear <= z <= zfar, 0 where there is none.  Coverage is an
 *   exact decision (fp64 edge functions, top-left rule: two triangles sharing an edge cover each sample once); samples, not
 *   triangles, are clipped at znear.  The arithmetic is written out at the head of csrc/raster.hip.  The image does not depend on
 *   scheduling (a 32-bit integer atomicMin per sample).
 *   counters (n_cam, 2) int32 <- per camera: triangles rasterised by a workgroup each (pixel box above I2SDF_RASTER_SMALL_MAX
 *   pixels), triangles rasterised by one lane each.  status: device int32 word, zeroed by the caller; set by a face with a vertex
 *   index outside [0, V) (such a face is skipped).
 *   workspace: i2sdf_raster_workspace_bytes(V, F, n_cam) bytes (0: sizes not supported); cameras are processed in chunks that fit
 *   it.  V = 0, F = 0 or n_cam = 0 enqueue at most the clearing of depth and counters.  Only enqueues; validated on the host first.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_RASTER_SMALL_MAX 64
int64_t i2sdf_raster_workspace_bytes(int64_t n_verts, int64_t F, int32_t n_cam);
int i2sdf_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, const float* w2c, int32_t n_cam,
                       const float* K4, int32_t H, int32_t W, float znear, float zfar, int32_t cull, void* workspace, float* depth,
                       int32_t* counters, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TSDF fusion and extraction (csrc/tsdf.hip) -- open3d's ScalableTSDFVolume as utils/mesh_util.py:refuse / :depth2mesh use it
 * (integrate every depth map, extract_triangle_mesh), restated from its sources; rule and arithmetic at the head of csrc/tsdf.hip.
 *   depths (n_cam, H, W) fp32 device, a value >= depth_trunc or not > 0 is no measurement; c2w / w2c (n_cam, 3, 4) fp32 device;
 *   K4 as above (HOST); voxel_length, sdf_trunc, depth_trunc > 0; unit_length = fp32(16 voxel_length), rounded by the caller;
 *   stride >= 1 (open3d's depth_sampling_stride); n_cam <= 65535.
 *   grid6 (HOST int32[6]) = lowest touched unit index per axis (|.| <= 2^21), number of units per axis: the dense table of unit
 *   slots.  i2sdf_tsdf_table_cells(grid6) = its cell count, 0 when a dimension is < 1 or the table would need more than
 *   I2SDF_TSDF_MAX_CELLS cells (every call that takes grid6 then returns I2SDF_EINVAL).
 *   _bounds     bounds (device int32[8], set by the caller to INT32_MAX x 3, INT32_MIN x 3, 0, 0) <- min / max unit index touched by
 *               any camera, bounds[6] <- 1 if a unit index left +-2^20 (that pixel is skipped)
 *   _mark       slot == NULL: stamp[cell] <- 1 for every cell any camera touches (stamp: device int32 per table cell, zeroed by the
 *               caller; cell = (ix dims[1] + iy) dims[2] + iz).  The caller turns the stamps into slot[cell] = running count - 1 (-1
 *               where untouched), unit_cell[slot] = cell, and zeroes them again.  slot != NULL: camera `cam` alone; stamp[cell] <-
 *               cam + 1, and the slots of the cells it touches are appended to list (n_units) int32, counted in *list_count (device
 *               int32, zeroed by the caller; cameras must be marked in ascending order).  *flag <- 1 on a cell outside the table.
 *   _integrate  camera `cam` into the listed units; tsdf, weight: (n_units, 4096) fp32 device, zeroed before the first camera;
 *               voxel (i, j, k) of a unit at i << 8 | j << 4 | k
 *   _count      classifies cells and edges; blocks (16 n_units, 2) int64 <- (vertices, faces) of every 256-voxel block.  workspace:
 *               i2sdf_tsdf_extract_workspace_bytes(n_units) bytes (0 for n_units outside [1, I2SDF_TSDF_MAX_CELLS])
 *   _emit       blocks_excl = the EXCLUSIVE running sums of `blocks` per column (by the caller, who reads the totals to size the
 *               outputs); same workspace.  verts / normals (cap_v, 3) fp32, faces (cap_f, 3) int32; rows beyond the capacities are
 *               not written; cap_v, cap_f <= INT32_MAX.  Vertex order: unit slot, voxel, axis; the right-hand face normal and the
 *               vertex normals point towards positive tsdf.
 * Only enqueues; validated on the host first.  Bitwise reproducible from run to run (integer atomics, or the
 * same constant from every writer as in _mark's union pass; one writer per voxel and per output element).
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_TSDF_MAX_CELLS (1 << 24)
int64_t i2sdf_tsdf_table_cells(const int32_t* grid6);
int64_t i2sdf_tsdf_extract_workspace_bytes(int64_t n_units);
int i2sdf_tsdf_bounds(const float* depths, int32_t n_cam, int32_t H, int32_t W, const float* c2w, const float* K4, float voxel_length,
                      float unit_length, float sdf_trunc, float depth_trunc, int32_t stride, int32_t* bounds, void* stream);
int i2sdf_tsdf_mark(const float* depths, int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float* c2w, const float* K4,
                    float voxel_length, float unit_length, float sdf_trunc, float depth_trunc, int32_t stride, const int32_t* grid6,
                    const int32_t* slot, int64_t n_units, int32_t* stamp, int32_t* list, int32_t* list_count, int32_t* flag, void* stream);
int i2sdf_tsdf_integrate(const float* depths, int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float* w2c, const float* K4,
                         float voxel_length, float unit_length, float sdf_trunc, float depth_trunc, const int32_t* grid6,
                         const int32_t* unit_cell, int64_t n_units, const int32_t* list, const int32_t* list_count, float* tsdf,
                         float* weight, void* stream);
int i2sdf_tsdf_count(const int32_t* grid6, const int32_t* slot, const int32_t* unit_cell, int64_t n_units, const float* tsdf,
                     const float* weight, void* workspace, int64_t* blocks, void* stream);
int i2sdf_tsdf_emit(const int32_t* grid6, float voxel_length, float unit_length, const int32_t* slot, const int32_t* unit_cell,
                    int64_t n_units, const float* tsdf, const float* weight, void* workspace, const int64_t* blocks_excl, float* verts,
                    float* normals, int32_t* faces, int64_t cap_v, int64_t cap_f, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rendered views (csrc/imgops.hip) -- what model/eval/recon.py does with a finished view (VolumeRenderSystem.test_step :161-203,
 * ViewInterpolateSystem.test_step :257-281): PSNR, SSIM, the camera-space normal map and the 8-bit frames given to the image writers.
 * Images have the render outputs' layout: pixel-major, channel-last fp32, (n_views, H W, C) contiguous, pixel p = y W + x, C = 3 for
 * rgb and normals and 1 for depth.  n_views <= 65535, H, W >= 1 (>= 11 for _ssim), H W <= INT32_MAX, else I2SDF_EINVAL; n_views = 0
 * returns I2SDF_OK and writes nothing.  workspace: i2sdf_image_workspace_bytes(n_views, H, W) bytes (0: sizes not supported), shared
 * by _stats and _ssim (disjoint parts).  Only enqueues; validated on the host first; no allocation.  Bitwise reproducible from run to
 * run: workgroups write fixed slots of the workspace that a second kernel adds in a fixed order (no floating-point atomics).
 *   _stats   stats (n_views, I2SDF_IMAGE_STATS) fp64 device <- per view
 *              [0] sum over the 3 H W values of ((double)pred - (double)gt)^2     (mse = [0] / (3 H W), psnr = -10 log10(mse):
 *                  utils/rend_util.py:get_psnr, which takes the mean in fp32)
 *              [1], [2] min, max of pred   [3], [4] min, max of gt   [5] max of depth   [6], [7] 0
 *            pred and gt (n_views, H W, 3) are given together or both NULL ([0] = 0, [1..4] = +inf, -inf, +inf, -inf); depth
 *            (n_views, H W) may be NULL ([5] = -inf); one of the two groups must be there.  NaNs are passed over by min / max.
 *   _ssim    ssim (n_views) fp64 device <- torchmetrics 0.11.4 structural_similarity_index_measure with its defaults (Gaussian
 *            window of 11 taps, sigma 1.5, k1 0.01, k2 0.03), restated from its source:
 *              g[i] = exp(-((i - 5) / 1.5)^2 / 2) / sum;  E[.] = the separable window mean, per channel;
 *              s_p = E[pp] - E[p]^2, s_t = E[tt] - E[t]^2, s_pt = E[pt] - E[p] E[t], c1 = (0.01 R)^2, c2 = (0.03 R)^2,
 *              ssim = ((2 E[p] E[t] + c1) (2 s_pt + c2)) / ((E[p]^2 + E[t]^2 + c1) (s_p + s_t + c2)),
 *            averaged over the 3 channels and the (H - 10) x (W - 10) pixels whose window lies inside the image (torchmetrics
 *            reflect-pads by 5 and crops 5 from the result: the same pixels).  R = data_range, finite and > 0; or NaN for
 *            max(max p - min p, max t - min t) of the view, read on the device from `stats` as _stats left it for the same pred, gt
 *            (torchmetrics' data_range=None for a batch of one view).  Moments in fp32 (as the reference's convolution), each
 *            product and sum rounded on its own; the per-pixel values are added in fp64.  One workgroup per
 *            I2SDF_SSIM_TILE_Y x I2SDF_SSIM_TILE_X tile of the result.
 *            map: NULL, or (n_views, H - 10, W - 10, 3) fp32 <- the per-pixel values; ssim is bit-identical either way.
 *   _frames  uint8 images (n_views, H, W, C); every output may be NULL (not written):
 *              rgb8       = trunc(clip(rgb * 255, 0, 255))                                     needs rgb
 *              normal_cam = pose[:3, :3]^T n  (summed in fp64, rounded to fp32 once; (n_views, H W, 3));  normal8 = trunc(clip((normal_cam + 1) / 2 * 255, 0, 255))
 *                           needs normal (world space) and pose (n_views, 4, 4) fp32 device, camera-to-world
 *              depth8     = trunc(clip(d / (stats[view][5] + 1e-6f) * 255, 0, 255))            needs depth and stats (_stats with depth)
 *              depth_rgb8 = lut[depth8], lut (256, 3) uint8 device: the caller's colour map    needs depth, stats and lut
 *            A NaN becomes 0.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_IMAGE_STATS 8
#define I2SDF_SSIM_TILE_X 32
#define I2SDF_SSIM_TILE_Y 16
int64_t i2sdf_image_workspace_bytes(int32_t n_views, int32_t H, int32_t W);
int i2sdf_image_stats(const float* pred, const float* gt, const float* depth, int32_t n_views, int32_t H, int32_t W, void* workspace,
                      double* stats, void* stream);
int i2sdf_image_ssim(const float* pred, const float* gt, int32_t n_views, int32_t H, int32_t W, float data_range, const double* stats,
                     void* workspace, double* ssim, float* map, void* stream);
int i2sdf_image_frames(const float* rgb, const float* normal, const float* depth, const float* pose, const double* stats,
                       const uint8_t* lut, int32_t n_views, int32_t H, int32_t W, uint8_t* rgb8, uint8_t* normal8, float* normal_cam,
                       uint8_t* depth8, uint8_t* depth_rgb8, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tone map of HDR validation views (csrc/imgops.hip), elementwise over n fp32 values of any layout.  Named outside the i2sdf_image_*
 * family: it takes no (n_views, H, W) and no workspace.
 *   dst[i] = srgb(clamp01 ? min(max(src[i], 0), 1) : src[i]) for i < n, srgb(x) = x <= 0.0031308 ? 12.92 x :
 * 1.055 x^(1/2.4) - 0.055 (utils/rend_util.py:linear_to_srgb; the validation of HDR data tone-maps prediction and ground truth
 * as `linear_to_srgb(x.clamp(0, 1))` before the metrics and the 8-bit images, model/trainer/recon.py:320-350).  fp32, every
 * product and sum rounded on its own; the upper branch is evaluated as 1.055 (x^(1/2.4) - 1) + 1, the same function, so that
 * 0 maps to 0 and 1 to 1 exactly (the formula as written gives 1 - 2^-24 at 1 in fp32, 254 instead of 255 in an 8-bit image).  Any n >= 0 (0: nothing is launched); dst == src (in place) is allowed, any other
 * overlap is not.  Without clamp01 a negative x takes the linear branch and a NaN stays a NaN; with it a NaN becomes 0.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_linear_to_srgb(const float* src, float* dst, int64_t n, int32_t clamp01, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bubble-PDF update (row N4) -- VolumeRenderSystem.update_pdf fused with the error it is fed (model/trainer/recon.py:142-152,
 * :195-199 in the initial sweep over all images, :246-252 every training step):
 *   channels == 1: v = |pred - target|                         (criterion DEPTH: depth_values vs depth image)
 *   channels == 3: v = mean_c |clamp(pred,0,1) - clamp(target,0,1)|   (criterion RGB)
 *   v = min(v, pdf_max) unless pdf_max is NaN / inf ("None");  v = 0 where v < pdf_prune;
 *   link = pointlinks[pixel];  pdf[link] = v where link != -1
 *   pixel_idx (n) global pixel indices, or NULL for the run first_pixel .. first_pixel+n-1 (a split of one image)
 *   n_bad: device counter of out-of-range pixels / links (skipped), or NULL.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_pdf_update(const float* pred, const float* target, int32_t channels, const int64_t* pixel_idx, int64_t first_pixel,
                     int64_t n, const int64_t* pointlinks, int64_t n_links, double pdf_max, double pdf_prune, float* pdf,
                     int64_t n_pdf, int32_t* n_bad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * All random draws of one training forward in one launch (Philox4x32-10 keyed by `seed`; a different stream, not torch's) --
 * the torch.rand / randperm / randint / uniform_ calls of ray_sampler.py:60-66,176-177,223,234 and
 * model/network/__init__.py:177,184.  Every output may be NULL (not drawn):
 *   strat_u (B, n_eval) in [0,1)      stratified jitter            cdf_u (B, n_samples) in [0,1)   inverse-CDF draws
 *   extra_idx (max_iters, n_extra)    row it = n_extra distinct columns of [0, n_eval*(it+1)) in random order
 *                                     (= randperm(n)[:n_extra] for the row length the sampler has after `it` iterations)
 *   eik_idx (B) in [0, n_z)           eik_pts (B,3) in [-eik_radius, eik_radius)    nbr_off (B,3) in [-w, w), w = nbr_half_width
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_training_draws(uint64_t seed, int64_t B, int32_t n_eval, int32_t n_samples, int32_t n_extra, int32_t max_iters,
                         int32_t n_z, float eik_radius, float nbr_half_width, float* strat_u, float* cdf_u,
                         int32_t* extra_idx, int32_t* eik_idx, float* eik_pts, float* nbr_off, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bubble points drawn by the PDF on the device (row N4) -- VolumeRenderSystem.sample_bubble (model/trainer/recon.py:154-170)
 * without its blocking torch.where and without torch.multinomial's 2^24 category limit: k of n entries without replacement,
 * proportional to `weights`, in one stream-ordered call (no allocation, no synchronisation, no host read).
 *
 * Law: successive sampling (the law of torch.multinomial(replacement=False), a different random stream).
 *   entry i is eligible iff 0 < weights[i] < inf (NaN, negative, zero and infinite entries are not); weights == NULL: every weight
 *   is 1 (the uniform_bubble ablation, randperm(n)[:k] without n indices);
 *   key_i = min(E_i / weights[i], FLT_MAX) in fp32 (the clamp keeps an eligible entry in front of every not-eligible one when the
 *           quotient overflows);  E_i = -log1pf(-v_i);  v_i = ((float)x_i + 0.5f) * 2^-32  (fp32 operations; the small end of E,
 *           which is where the k smallest keys of many entries lie, keeps all 32 random bits);
 *   x_i   = word (i & 3) of Philox4x32-10 with counter (lo32(i >> 2), hi32(i >> 2), 7, draw) and key (lo32(seed), hi32(seed)):
 *           one Philox call per four neighbouring entries = one 16-byte load of `weights`;  `draw`: the caller's call counter;
 *   result: the k eligible entries with the smallest composite (bits(key_i), i), in ascending order of the composite -- the order
 *           of the successive draws; ties on the key go to the lower index.
 * Outputs: idx (k) int64;  points (k, 3) = pointcloud[idx] (pointcloud == NULL or points == NULL: skipped);
 *   sample_count[idx] += 1 (fp32, n entries; NULL: skipped -- the indices are distinct, no atomics).
 * Shortfall: with only m < k eligible entries rows [0, m) are the draw and row j >= m repeats row j mod m; sample_count counts the m
 *   real draws; m = 0: idx = -1, points = 0.  *status (device int32, or NULL) accumulates k - m.  If so many keys EQUAL the k-th
 *   smallest that more than 2k entries have key <= it (collisions of 2^-32), the first k of the 2k captured are returned and
 *   *status grows by 1; nothing is written out of bounds.  The host never reads m.
 * Limits (checked on the host before any launch, I2SDF_EINVAL): 1 <= k <= I2SDF_BUBBLE_MAX_K, 0 <= n < 2^31, idx and workspace
 *   not NULL.  workspace: i2sdf_bubble_sample_workspace_bytes(k) bytes (0 for a k outside the limits), 16-byte aligned; the call
 *   clears what it needs on `stream`.
 * Method: an exact radix select over the key bits (12 + 10 + 9; bit 31 is 0): per-workgroup LDS histograms merged by integer atomics
 *   (order-independent, so the result is bitwise reproducible), a one-wave pick of the bin where the running count crosses k, then a
 *   collect of every key <= the threshold and one workgroup that sorts those by the composite.  The threshold is the upper end of
 *   the first chosen bin with at most 2k entries at or below it -- the later histogram passes then return at once; keys near the
 *   small end are evenly spread, so pass A alone decides unless the keys cluster -- and the k-th smallest key itself after pass C.
 *   The keys are recomputed from (i, weights[i]) in every pass and never stored: 4 n bytes are read per pass, 2 to 4 passes
 *   (1 to 3 histogram passes and the collect pass).  How many a call made is left in its workspace, for measurements: the uint32
 *   at byte I2SDF_BUBBLE_WS_PASSES_OFFSET, valid once the call has completed on `stream` and until the next call on that workspace.
 * i2sdf_bubble_keys: the fp32 keys themselves (keys_out (n); +inf for a not-eligible entry) from the device function the select uses.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_BUBBLE_MAX_K 4096
#define I2SDF_BUBBLE_WS_PASSES_OFFSET 24
int64_t i2sdf_bubble_sample_workspace_bytes(int64_t k);
int i2sdf_bubble_sample(const float* weights, int64_t n, const float* pointcloud, int64_t k, uint64_t seed, uint32_t draw,
                        void* workspace, int64_t* idx, float* points, float* sample_count, int32_t* status, void* stream);
int i2sdf_bubble_keys(const float* weights, int64_t n, uint64_t seed, uint32_t draw, float* keys_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point cloud and pixel <-> point links from the depth maps (dataset/train_dataset.py:112-141, utils/rend_util.py:81-89,134-147),
 * a stream compaction in the reference's order (image-major, pixel order within an image):
 *   depth (n_img, H W) fp32, intrinsics (n_img, 4, 4), pose (n_img, 4, 4) camera-to-world, all device;
 *   pixel p of an image: u = p mod W, v = p div W;  valid iff lo < d < hi (a NaN is not; the reference: lo = 1e-3, hi = 6);
 *   x_l = (u - cx + cy sk / fy - sk v / fy) / fx,  y_l = (v - cy) / fy   (fx = K00, fy = K11, cx = K02, cy = K12, sk = K01);
 *   point = (pose [x_l d, y_l d, d, 1]^T)[:3] / its fourth component.
 *   _count: depth_masks (n_img H W) bytes 0 / 1 (or NULL) and the per-block counts and their exclusive scan in `workspace`
 *           (i2sdf_depth_unproject_workspace_bytes(n_img, H, W) bytes; 0 for sizes outside the limits); n_points (HOST int64) is
 *           copied back -- ONE stream synchronisation: this is set-up, the caller sizes the outputs with it.
 *   _write: same inputs and workspace; pointlinks (n_img H W) int64, -1 where the pixel is not valid; pixlinks (n_points) int64
 *           global pixel index; pointcloud (n_points, 3).  n_points: what _count returned (writes past it are dropped).
 * Limits (I2SDF_EINVAL): n_img >= 0, H, W >= 1, H W <= INT32_MAX, n_img H W < 2^36; n_img = 0 is a no-op with n_points = 0.
 * Cost: the per-block counts (one per 1024 pixels) are scanned by ONE workgroup, 256 counts per round with three barriers a round:
 *   180 rounds for the reference's 150 views of 640 x 480 (45 000 blocks), but 262 144 serial rounds at the 2^36 limit -- the limit
 *   is what the indices allow, not a size at which this set-up call is quick.
 * ---------------------------------------------------------------------------------------------- */
int64_t i2sdf_depth_unproject_workspace_bytes(int64_t n_img, int32_t H, int32_t W);
int i2sdf_depth_unproject_count(const float* depth, int64_t n_img, int32_t H, int32_t W, float lo, float hi, void* workspace,
                                uint8_t* depth_masks, int64_t* n_points, void* stream);
int i2sdf_depth_unproject_write(const float* depth, const float* intrinsics, const float* pose, int64_t n_img, int32_t H, int32_t W,
                                float lo, float hi, const void* workspace, int64_t n_points, int64_t* pointlinks, int64_t* pixlinks,
                                float* pointcloud, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Surface shading -- RenderingLayer.forward (model/rendering/__init__.py) around its model call, with the parts of the BRDF library
 * it uses (model/rendering/brdf.py: create_frame, probabilityToSampleSpecular, square_to_cosine_hemisphere, sample_ggx_specular,
 * pdf_ggx, eval_ggx).  csrc/shade.hip; the per-sample arithmetic is csrc/brdf_dev.h, shared by host and device.  No plan: the layer
 * does not depend on the networks.  All tensors fp32, contiguous, device; per-point inputs (bn, 3), rough (bn, 1).
 *
 * Per point:
 *   frame   z = n / max(|n|, 1e-6);  s = z_z >= 0 ? 1 : -1;  a = -1 / (s + z_z);  b = z_x z_y a;
 *           x = (1 + s z_x^2 a, s b, -s z_x);  y = (b, s + z_y^2 a, -z_y)                              [Duff et al. 2017]
 *   wi      = (x.v, y.v, z.v) of view_direction v;  wi_mask = wi_z >= 1e-5;  then wi_z = max(wi_z, 1e-5) and wi / max(|wi|, 1e-6)
 *   pS      = lS / (lD + lS),  l = max(lum(K), 0.01),  lum(c) = 0.212671 r + 0.715160 g + 0.072169 b  (a constant of the backward)
 * Per sample s of point p, uniforms (u0, u1, u2) in [0, 1), with sq(t) = sqrt(max(t, 1e-8)) and nrm(v) = v / max(|v|, 1e-8):
 *   diffuse lobe iff u0 >= pS:   wo = (cos(2 pi u1) sq(u2), sin(2 pi u1) sq(u2), sq(max(1 - u2, 0)))
 *   else, alpha = rough^2:       Vh = nrm(alpha wi_x, alpha wi_y, wi_z);  q = Vh_x^2 + Vh_y^2;
 *                                T1 = q > 0 ? (-Vh_y, Vh_x, 0) / sq(q) : (1, 0, 0);  T2 = Vh x T1;
 *                                t1 = sq(u1) cos(2 pi u2);  t2 = sq(u1) sin(2 pi u2);  t2 <- lerp(sq(1 - t1^2), t2, (1 + Vh_z) / 2);
 *                                Nh = t1 T1 + t2 T2 + sq(max(1 - t1^2 - t2^2, 0)) Vh;  h = nrm(alpha Nh_x, alpha Nh_y, max(Nh_z, 0));
 *                                wo = 2 (wi.h) h - wi                                       [Heitz 2018, visible normals]
 *   direction = wo_x x + wo_y y + wo_z z (world);   points = surface_points + 0.01 direction
 *   H = nrm(wi + wo);  A = max(alpha^2, 1e-5) (inside D only);  D = A / (pi ((A - 1) H_z^2 + 1)^2)
 *   G1 = 2 / (sq((alpha^2 (1 - wi_z^2) + wi_z^2) / wi_z^2) + 1)
 *   pdf = pS D G1 / (4 wi_z) + (1 - pS) wo_z / pi;  pdf = 1e-4 where wi_z <= 1e-4 or wo_z <= 1e-4;  pdf = max(pdf, 1e-5)
 *   G2 = 1/2 / (wi_z sq(alpha^2 + wo_z (wo_z - alpha^2 wo_z)) + wo_z sq(alpha^2 + wi_z (wi_z - alpha^2 wi_z)))
 *   F = Ks + (F90 - Ks) (1 - wo.H)^5,  F90 = min(25 lum(Ks), 1);   f_spec = wo_z < 1e-4 ? 1e-4 : F G2 D;   f_diff = Kd / pi
 *   w = max(wo_z, 0) / pdf;   L = radiance[p spp + s] * radiance_scale (scale NULL: ones)
 *   colorDiffuse[p] = mean_s f_diff w L;   colorSpec[p] = mean_s f_spec w L
 * Uniforms: `samples` (bn, spp, 3) of the caller, or drawn in the kernels from `seed` (HOST pointer to the 64-bit seed, read during
 *   the call): Philox4x32-10, counter (p spp + s, 0, 8, 0), key (lo32(seed), hi32(seed)), u_k = (word_k >> 8) 2^-24 of words 0, 1, 2.
 *   Exactly one of samples / seed is given.  i2sdf_shade_draws writes the uniforms a seed stands for.
 * i2sdf_shade_sample:   direction, points (bn spp, 3), wi_mask (bn) bytes 0 / 1.
 * i2sdf_shade_reduce:   colorDiffuse, colorSpec (bn, 3) from radiance (bn spp, 3) and radiance_scale (3) or NULL.  Nothing per-sample
 *   is kept between the calls: wo, pdf and f are recomputed from the same uniforms.  Summation order: with G the smallest power of two
 *   >= min(spp, 64), lane j of G takes samples j, j + G, ... in order, then the G partial sums meet in a butterfly (distance G/2, ..., 1):
 *   fixed, no atomics, bitwise reproducible.
 * i2sdf_shade_backward: upstream g_colorDiffuse, g_colorSpec (bn, 3) give gKd, gKs (bn, 3), grough (bn, 1), optionally g_radiance
 *   (bn spp, 3, the gradient by `radiance` before the scale) and g_radiance_scale (3): per-workgroup partial sums in fixed slots of
 *   `workspace` (i2sdf_shade_backward_workspace_bytes(bn, spp) bytes; 0 for sizes outside the limits), summed by a second one-workgroup
 *   pass.  g_direction / g_points (bn spp, 3; each may be NULL) are the gradients a differentiable model returns for the rays: they
 *   add (g_direction + 0.01 g_points) . d direction / d rough to grough.  Either group of upstream gradients may be absent -- the
 *   colour group (g_colorDiffuse, g_colorSpec, radiance, gKd, gKs: all or none) or the ray group -- but not both; without the colour
 *   group gKd / gKs are not written and g_radiance / g_radiance_scale must be NULL.  d / d rough follows wo through alpha, as the
 *   reference's autograd does; a clamp passes the derivative where torch.clamp does (bound included); pS is a constant.  normal,
 *   view_direction and surface_points get no gradient: the geometry is frozen at this stage.
 * Limits (checked on the host before any launch, I2SDF_EINVAL with the reason in i2sdf_last_hip_error()): bn >= 0 (0: nothing is
 *   launched), spp >= 1, bn spp < 2^31, no required pointer NULL, exactly one of samples / seed.
 * ---------------------------------------------------------------------------------------------- */
int i2sdf_shade_draws(uint64_t seed, int64_t bn, int32_t spp, float* samples, void* stream);
int i2sdf_shade_sample(const float* surface_points, const float* view_direction, const float* normal, const float* Kd, const float* Ks,
                       const float* rough, const float* samples, const uint64_t* seed, int64_t bn, int32_t spp, float* direction,
                       float* points, uint8_t* wi_mask, void* stream);
int i2sdf_shade_reduce(const float* view_direction, const float* normal, const float* Kd, const float* Ks, const float* rough,
                       const float* samples, const uint64_t* seed, const float* radiance, const float* radiance_scale, int64_t bn,
                       int32_t spp, float* colorDiffuse, float* colorSpec, void* stream);
int64_t i2sdf_shade_backward_workspace_bytes(int64_t bn, int32_t spp);
int i2sdf_shade_backward(const float* view_direction, const float* normal, const float* Kd, const float* Ks, const float* rough,
                         const float* samples, const uint64_t* seed, const float* radiance, const float* radiance_scale,
                         const float* g_colorDiffuse, const float* g_colorSpec, const float* g_direction, const float* g_points,
                         int64_t bn, int32_t spp, void* workspace, float* gKd, float* gKs, float* grough, float* g_radiance,
                         float* g_radiance_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Emitter clustering -- I2SDFNetwork.init_emission_groups (model/network/__init__.py:49-75): k-means++ seeding
 * (utils.kmeans_pp_centroid, utils/__init__.py:111-123) and Lloyd's iteration (fast_pytorch_kmeans.KMeans.fit_predict) of a point cloud
 * on the device.  csrc/kmeans.hip.  No plan.  Every call only enqueues on `stream`: no allocation, no synchronisation, no host read;
 * no floating-point atomic, so every result is bitwise reproducible.
 *
 * points (n, 3) fp32, 1 <= k <= n < 2^31, k <= I2SDF_KMEANS_MAX_K.  The squared distance of a point to a centroid is the direct form
 *   ((x - cx)^2 + (y - cy)^2) + (z - cz)^2, every operation rounded to fp32 and none contracted into an FMA.  (The reference forms
 *   2ab - a^2 - b^2 in Lloyd; its cancellation is not imitated.)
 *
 * Seeding (i2sdf_kmeans_pp).  The law is the reference's: each next centroid is a data point drawn with probability proportional to its
 *   distance (not its squared distance) to the nearest centroid chosen so far.  The random stream is not numpy's: an exponential race on
 *   Philox4x32-10 with key (lo32(seed), hi32(seed)) and stream word 9 (1..6: the training draws, 7: the bubble sampler, 8: shading).
 *   round 0:        x = word 0 of counter (0, 0, 9, 0);  j_0 = (uint64(x) n) >> 32.
 *   round i = 1..k-1: d_j = min(d_j, sqrtf(dist2(p_j, c_{i-1}))) in fp32, d starting at +inf;
 *                   key_j = min(E_j / d_j, FLT_MAX), E_j = -log1pf(-v_j), v_j = ((float)x_j + 0.5f) 2^-32 (i2sdf_bubble_sample's key with
 *                   weight d_j), x_j = word (j & 3) of counter (lo32(j >> 2), hi32(j >> 2), 9, i);
 *                   point j is eligible iff 0 < d_j < inf;  j_i = the eligible j with the smallest (uint64(bits(key_j)) << 32) | j, so
 *                   ties go to the lowest index;  nothing eligible (every distance 0: more centroids than distinct points): j_i = 0,
 *                   the reference's argmax of an all-false mask.
 *   Outputs: idx_out (k) int64 = j_0 .. j_{k-1}, centroids_out (k, 3) = points[idx_out].
 *   Cost: one launch per round, one pass over the points each (12 B of point and 4 B of d read, 4 B of d written per point; d lives in
 *   the workspace), ending in one 64-bit integer atomicMin per workgroup into the round's own slot, which the next round's launch reads.
 *
 * Lloyd (i2sdf_kmeans_fit): fit_predict of fast-pytorch-kmeans 0.1.9 with its defaults (euclidean, no minibatch), restated from its
 *   source; the restatement has NOT been checked against the library itself (it is not installed where this project is developed).
 *   Per iteration, with c the current centroids (in: the initial ones, out: the final ones):
 *     1. labels_j = the index of the nearest centroid by dist2, the lowest index on ties (and for a point whose distances are all NaN);
 *     2. c_new    = the mean of each cluster's points; an empty cluster gets (0, 0, 0) (the library's nan_to_num);
 *     3. error    = sum over all 3k values of (c_new - c)^2  (fp64 of the fp32 values, fixed-order tree sum);
 *     4. c = c_new;   5. stop after this iteration iff error <= tol.      At most max_iter iterations (the library: 100, tol 1e-4).
 *   So the returned labels are those of the last iteration that ran: they belong to the centroids BEFORE the final update, as in the
 *   library.  *n_iter (device int32) = iterations that ran.  The stop is a device flag: 2 max_iter launches are always enqueued, and
 *   once the flag is set the remaining ones return at once.
 *   Sums: 64-bit integer FIXED POINT.  With m the largest finite |coordinate| of the cloud (found by a pass of its own at the start of
 *   the call) and 2^(e-1) <= m < 2^e, a coordinate x adds llrint(x 2^(31-e)) to its cluster's sum (|.| <= 2^31, so fewer than 2^31
 *   points stay below 2^62); integer adds commute, so per-workgroup LDS sums and one global integer atomic per non-empty (cluster,
 *   component, workgroup) give sums that do not depend on arrival order.  A coordinate below m 2^-8 in magnitude is rounded to a
 *   multiple of m 2^-31 (at most half of that off); mean = double(sum) 2^(e-31) / count, rounded once to fp32.  A non-finite coordinate
 *   adds 0 to the sum (its point still counts).
 * i2sdf_kmeans_assign: step 1 alone on any points (KMeans.predict), dist2 (n) = the squared distance to the chosen centroid, or NULL.
 *   Here k may exceed n (a few new points against many centroids); n = 0 is a no-op returning I2SDF_OK.
 * workspace: i2sdf_kmeans_workspace_bytes(n, k) bytes (0 for sizes outside the limits), 16-byte aligned, shared by _pp and _fit; each
 *   call clears what it reads on `stream`, so the contents before a call do not matter.
 * Limits, checked on the host before any launch (I2SDF_EINVAL): the sizes above, no pointer NULL (dist2 excepted), max_iter >= 1,
 *   tol >= 0 and not NaN, workspace alignment.
 * Not imitated: minibatch k-means, cosine mode, dimensions other than 3, numpy's random stream.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_KMEANS_MAX_K 256
int64_t i2sdf_kmeans_workspace_bytes(int64_t n, int64_t k);
int i2sdf_kmeans_pp(const float* points, int64_t n, int64_t k, uint64_t seed, void* workspace, int64_t* idx_out, float* centroids_out,
                    void* stream);
int i2sdf_kmeans_fit(const float* points, int64_t n, int64_t k, float* centroids, int32_t max_iter, double tol, void* workspace,
                     int64_t* labels, int32_t* n_iter, void* stream);
int i2sdf_kmeans_assign(const float* points, int64_t n, const float* centroids, int64_t k, int64_t* labels, float* dist2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Density clustering -- the `use_dbscan` seeding of I2SDFNetwork.init_emission_groups (model/network/__init__.py:50-65, where
 * sklearn.cluster.DBSCAN labels 10 000 sampled points on the host) for the whole cloud on the device.  csrc/dbscan.hip.  No plan.
 * Every call only enqueues on `stream`: no allocation, no synchronisation, no host read.  No (n, n) or neighbour-list storage: the
 * workspace is linear in n.
 *
 * The law.  points (n, 3) fp32, 1 <= n < 2^31, eps > 0, min_samples >= 1.
 *   Distance.  d2(i, j) = dx*dx + dy*dy + dz*dz: differences, products and sums in fp64 on the fp64 images of the fp32 coordinates,
 *              each rounded on its own (no FMA) and added x, y, z left to right.  i and j are neighbours iff d2 <= eps*eps, eps*eps
 *              formed once in fp64.  The bound is inclusive.
 *   Core.      core[i] iff at least min_samples points j, i itself counted, are neighbours of i.
 *   Clusters.  A cluster is a connected component of the core points under the neighbour relation.  Clusters are numbered 0, 1, ... by
 *              ascending smallest original index of their CORE points; a core point carries its cluster's number.
 *   Border.    A non-core point with at least one core neighbour carries the smallest number among its core neighbours' clusters.
 *   Noise.     Every other point is -1.
 *   Non-finite.  A point with a non-finite coordinate is -1, is nobody's neighbour, and sets status bit 0.
 * This is a RESTATEMENT of sklearn.cluster.DBSCAN(eps, min_samples).fit(X) (labels_, core_sample_indices_): the library expands
 * clusters depth first, serially, in index order, so its cluster numbers ascend with the first core point and a contested border point
 * goes to the cluster expanded first.  It was checked against the library (scikit-learn 1.7.2) where the library was importable:
 * tests/test_dbscan_ref.py holds the numpy form of the law (tests/dbscan_ref.py) to the library, tests/test_gpu_dbscan.py the device
 * to that form, exactly.  Not offered: metric, algorithm, leaf_size, p, sample_weight; dimensions other than 3.
 *
 * How it is computed (results do not depend on it; all four outputs are order-free functions of the input, so bitwise reproducible).
 *   Cells.  lo = the per-axis minimum of the finite points; cell edge c = (eps / 2)(1 + 2^-20); cell coordinate floor((p - lo) / c) in
 *     fp64; 21 bits per axis in one int64 key.  A quotient below 2^21 carries an absolute error below 2^-31 (two roundings of 2^-53).
 *     (a) Two points of one cell are neighbours: their quotients share a unit interval, so they differ by less than c (1 + 2^-30) on
 *         every axis, and d2 < 3 c^2 (1 + 2^-29) < 0.7501 eps^2 (the cell's diagonal is 0.867 eps).
 *     (b) Two neighbours lie at most 2 cells apart on every axis: |dx| <= eps (1 + 2^-52) gives quotients at most
 *         2 / (1 + 2^-20) + 2^-30 < 2 - 9e-7 apart, so their floors differ by at most 2 -- also for pairs at exactly eps on a lattice,
 *         whatever the rounding of the quotient: the 2^-20 of slack in c is a thousand times that rounding.
 *     So a point's neighbours are in the 5 x 5 x 5 cells around its own.  A coordinate beyond 2^21 cells sets status bit 1; such a call
 *     yields all labels -1, core 0 and n_clusters 0.  The cells are sparse: i2sdf_dbscan_cell_keys writes one key per point, the CALLER
 *     sorts them (stable, ascending, with the permutation: torch.sort), and i2sdf_dbscan_label finds the run heads, scans them and keeps
 *     the unique keys; a neighbour cell is a binary search in those, done once per occupied cell (by the wave that owns the cell), not
 *     once per point.  No dense cell table: two blobs 10^4 apart at eps = 0.01 cost no more than their points.
 *   Core.  A cell holding min_samples points or more makes all of them core by (a), without a distance; any other point counts its
 *     neighbours over the 125 cells and stops at min_samples.
 *   Unions, on original indices, lock-free (csrc/unionfind.h): the core points of a cell are hooked to the smallest of them; for two
 *     neighbouring cells whose roots differ when looked at, one core pair within eps is searched, the search ends at the first hit and
 *     unites the two.  A larger root is hooked under a smaller one by compare-and-swap, so the final root is the component's smallest
 *     core index whatever the schedule.  No kernel waits for another workgroup; a retry follows only a lost compare-and-swap.
 *   Labels.  A flag at every root, an exclusive scan, n_clusters = its total; a core point takes rank[root]; a non-core point the
 *     smallest rank over the neighbour cells holding a core point within eps of it.
 *
 * i2sdf_dbscan_cell_keys: keys (n) int64 (INT64_MAX for a point without a cell); *status = the status bits.
 * i2sdf_dbscan_label: sorted_keys, perm (n) int64 = the stable ascending sort of keys and its permutation; the SAME points, n, eps and
 *   workspace as the call that wrote the keys.  labels (n) int64, core (n) uint8 (0 / 1), *n_clusters, *status int32 (the same bits
 *   again).  A perm entry outside [0, n) is never dereferenced: its sorted entry holds no point.
 * workspace: i2sdf_dbscan_workspace_bytes(n) bytes: 0 for n < 1 or n >= 2^31, otherwise a multiple of 16, monotone in n and at most
 *   96 n + 65536 (about 41 n); 16-byte aligned; the contents before i2sdf_dbscan_cell_keys do not matter.
 * Refused with I2SDF_EINVAL before any launch: a NULL or misaligned pointer (stream excepted), n outside the range, eps not finite and
 *   positive (or eps*eps not), min_samples < 1.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_DBSCAN_NONFINITE 1      /* status bit 0 */
#define I2SDF_DBSCAN_CELLS 2          /* status bit 1 */
int64_t i2sdf_dbscan_workspace_bytes(int64_t n);
int i2sdf_dbscan_cell_keys(const float* points, int64_t n, double eps, void* workspace, int64_t* keys, int32_t* status, void* stream);
int i2sdf_dbscan_label(const float* points, int64_t n, double eps, int32_t min_samples, const int64_t* sorted_keys, const int64_t* perm,
                       void* workspace, int64_t* labels, uint8_t* core, int32_t* n_clusters, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sphere tracing of the SDF's zero level -- the `intersect_func` hook of RenderingLayer.forward / get_incident_radiance
 * (model/rendering/__init__.py, model/network/__init__.py).  The reference names the hook and released no implementation, so the
 * marching rule is defined HERE; tests/trace_ref.py restates it in fp32 and fp64.  csrc/mlp_trace.hip, csrc/trace_rule.h.
 * A march is a serial chain of network passes: its latency is steps x one sdf-only forward however few the rays.
 *
 * Per ray: origin o = cam[r], unit direction d = dirs[r], interval [t0, t1] = [t_min[r], t_max[r]].  State: t, lo, hi, bracketed, status,
 * steps.  Every operation of the rule is ONE fp32 operation, rounded to nearest, in the order written, none contracted into an FMA
 * (csrc/trace_rule.h switches contraction off for the rule).  The point of a depth t is the one the sdf-only forward forms from a ray,
 * fetch_point of csrc/mlp_common.h: its `cam + t * dirs` is contracted by hipcc, so a component is fma(t, d, o), rounded ONCE -- the
 * fused kernels form it from the same expression, and tests/test_gpu_trace.py holds every f to i2sdf_sdf_forward at that point bit for bit.
 *   Init.  status = MISS if not (t1 > t0) (a NaN bound too); otherwise ACTIVE.  t = lo = hi = t0, bracketed = 0, steps = 0.
 *   Step of an ACTIVE ray.  f = sdf(o + t d); steps += 1; then the FIRST of these that applies ends the step:
 *     1. f not finite                      -> UNRESOLVED, t stays.
 *     2. |f| <= eps                        -> HIT, t stays.
 *     3. f < 0 and steps == 1              -> INSIDE (the origin lies behind the surface), t = t0.
 *     4. f < 0: hi = t, bracketed = 1.  Otherwise lo = t.
 *     5. bracketed:      tn = lo + 0.5f * (hi - lo);  tn == lo or tn == hi (the bracket is one fp32 step wide) -> HIT, t = hi.
 *     6. not bracketed:  tn = t + step_scale * f;     tn >= t1 -> MISS, t = t1.
 *     7. t = tn.
 *   End.  A ray still ACTIVE after max_steps steps ends UNRESOLVED at its last t.
 * The bracket (4, 5) is what makes an overshoot harmless: |grad sdf| of a fitted net exceeds 1 in places, a sphere-tracing step then
 * lands behind the surface, and from there on the ray bisects between its last outside and its first inside depth.
 *
 *   cam, dirs (N,3) ; t_min, t_max (N) ; t_out (N) fp32 ; status_out, steps_out (N) int32
 *   f_trace (max_steps, N) or NULL: row s holds the f of step s + 1 for the rays that took that step; other entries are left untouched.
 *   workspace: i2sdf_trace_workspace_floats(N) floats (0 for N < 0), contents before the call do not matter.
 * cfg.route:
 *   I2SDF_TRACE_STEPWISE  per step one launch of the sdf-only forward of i2sdf_sdf_forward (three split planes under
 *                         I2SDF_OPT_SDF_FWD_BF16X3, never the sampler's two) on the ray-form points, then one launch that applies the rule;
 *                         finished rays are still evaluated.  Every plan has it.
 *   I2SDF_TRACE_FUSED     one kernel: a workgroup keeps its 128 rays for the whole march -- per pass it forms the points, rebuilds the
 *                         encoding, restarts the weight stream, runs the layer chain and applies the rule -- and leaves when none of its
 *                         rays is ACTIVE (a tile of misses costs one or two passes).  Plans whose sdf-only forward runs in bf16x3 split
 *                         arithmetic have one (I2SDF_OPT_SDF_FWD_BF16X3 on a 256/256 or 64/64 net); any other plan refuses this route.
 *   I2SDF_TRACE_AUTO      the fused kernel where the plan has one, the stepwise route otherwise.  Measured on the synthetic.yml net
 *                         (profiles/trace_timing.json): 37.0 against 79.5 ms at 307 200 rays, 6.5 against 6.8 ms at 1024.
 *   All launches are stream ordered; the host reads nothing back; t, status, steps and f_trace do not depend on the route, bit for bit.
 * Refused with I2SDF_EINVAL and a text in i2sdf_last_hip_error(), nothing launched: eps <= 0 or not finite; step_scale outside (0, 1];
 *   max_steps outside 1..I2SDF_TRACE_MAX_STEPS; an unknown route; I2SDF_TRACE_FUSED on a plan without a fused kernel; a NULL pointer
 *   (f_trace and stream excepted); N < 0 or N >= 2^31.  N = 0 succeeds and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_TRACE_ACTIVE 0          /* only inside the march: never returned */
#define I2SDF_TRACE_HIT 1
#define I2SDF_TRACE_MISS 2
#define I2SDF_TRACE_UNRESOLVED 3
#define I2SDF_TRACE_INSIDE 4
#define I2SDF_TRACE_AUTO 0
#define I2SDF_TRACE_STEPWISE 1
#define I2SDF_TRACE_FUSED 2
#define I2SDF_TRACE_MAX_STEPS 1024
typedef struct i2sdf_trace_cfg { float eps, step_scale; int32_t max_steps, route; } i2sdf_trace_cfg;
int64_t i2sdf_trace_workspace_floats(int64_t N);
int i2sdf_trace_rays(const i2sdf_plan* plan, const float* packed, const i2sdf_trace_cfg* cfg, const float* cam, const float* dirs,
                     const float* t_min, const float* t_max, int64_t N, float* t_out, int32_t* status_out, int32_t* steps_out,
                     float* f_trace, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ray casting against a triangle mesh -- the external ray caster the `intersect_func` hook of RenderingLayer.forward /
 * get_incident_radiance is meant for, on the mesh the library extracts itself; also occlusion queries.  csrc/bvh.hip, csrc/tri_isect.h.
 * No plan.  Every call only enqueues on `stream`: no allocation, no synchronisation, no host read.  tests/raycast_ref.py restates the
 * rule, the keys and the topology in numpy.
 *
 * The law.  verts (V, 3) fp32, faces (F, 3) int32, rays o = orig[r], d = dirs[r] (any length, t is in units of d), t_min[r], t_max[r].
 *   Ray.  kz = the axis of the largest |d| (the lowest such axis); kx = kz + 1, ky = kx + 1 (mod 3), swapped when d[kz] < 0;
 *         Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  A ray with a non-finite component of o or d, with d = 0, with a
 *         non-finite Sz, or with a NaN bound hits nothing and sets I2SDF_RAYCAST_BAD_RAY.
 *   Face (A, B, C), per vertex P:  Pkz = P[kz] - o[kz];  Px = (P[kx] - o[kx]) - Sx * Pkz;  Py = (P[ky] - o[ky]) - Sy * Pkz.
 *         U = Cx * By - Cy * Bx;  V = Ax * Cy - Ay * Cx;  W = Bx * Ay - By * Ax.
 *         If U == 0 or V == 0 or W == 0: all three are formed again from the fp64 images of the six sheared coordinates (products
 *         exact, one rounding of the difference) and rounded to fp32.
 *         Reject if one of U, V, W is < 0 and one is > 0.  det = (U + V) + W; reject if det == 0.
 *         cull: det < 0 is a BACK face -- its right-hand normal (B - A) x (C - A) points along the ray -- rejected under
 *         I2SDF_RAYCAST_CULL_BACK.  These are the faces i2sdf_mesh_depth calls back faces (its own determinant is positive there).
 *         Pz = Sz * Pkz;  T = (U * Az + V * Bz) + W * Cz;  t = T / det;  u = U / det, v = V / det (the weights of A and of B).
 *         The face counts iff t_min < t <= t_max.
 *         Every operation above is ONE fp32 operation, rounded to nearest, in the order written, none contracted into an FMA: a*b - c*d
 *         is the exact negative of c*d - a*b only without one, and that is what makes the two faces at a shared edge see exactly
 *         negated edge functions: a ray cannot slip between them (Woop, Benthin, Wald: Watertight Ray/Triangle Intersection, JCGT 2013).
 *   Faces that are never hit: an index outside [0, V) or a non-finite vertex (sets I2SDF_RAYCAST_BAD_FACE in every trace of that
 *         mesh, whatever the rays); two equal vertices (the zero-area faces marching cubes emits: their sheared image is degenerate,
 *         so U + V + W is exactly 0 and non-mixed signs mean U = V = W = 0).
 *   Result per ray: the smallest t among the faces that count; among equal t the smallest face index.  An order-free function of the
 *         inputs, so bitwise reproducible and the same by every route.  A miss returns face = -1, t = t_max, u = v = 0.
 *         any_hit: only hit[r] is written; it IS the closest-hit flag (the search may stop at the first face that counts).
 *   *status: the OR of the two bits over the call.
 *
 * The tree (i2sdf_bvh_keys -> the caller's sort -> i2sdf_bvh_build), a linear BVH, one face per leaf.
 *   Keys.  lo, hi = per-axis min / max of the vertices of the faces that can be hit (a device reduction).  Per axis, in fp64:
 *         c = ((a + b) + c') / 3;  q = hi > lo ? clamp(floor(((c - lo) / (hi - lo)) * 1024), 0, 1023) : 0.  code = the 30-bit Morton
 *         interleave of (qx, qy, qz), x highest; a face that is never hit for its indices or vertices takes code 2^30.
 *         key = code << 32 | face: unique, and the face index rides in the low word.  The CALLER sorts the keys ascending (torch.sort).
 *   Topology.  Karras (Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees, HPG 2012): internal node i of
 *         F - 1, node 0 the root, delta(i, j) = the number of leading bits sorted keys i and j share (-1 outside the array).
 *   Boxes.  The exact fp32 min / max of the vertex coordinates below a child (`b < a ? b : a` in the order A, B, C, then slot 0, slot 1),
 *         no padding; the empty box (+inf, -inf) below faces that are never hit.  Fitted bottom-up, one arrival counter per node.
 *   Records.  Internal node, 64 bytes: lo0[3], hi0[3], lo1[3], hi1[3], child[2] (>= 0: internal node; < 0: leaf ~child), 8 unused.
 *         Leaf, 48 bytes, in sorted order: A, B, C, face (-1: never hit), 8 unused.  Buffer: 256 header | 64 F nodes | 48 F leaves |
 *         3 x 4 F (parent links, arrival counters) = 124 bytes per face: i2sdf_bvh_bytes(F), a multiple of 16, monotone, at most
 *         124 F + 304; 0 for F < 0 or F > I2SDF_BVH_MAX_FACES = 2^28 (node indices, their complements and `node << 1 | slot` parent
 *         links stay inside int32, and the 33 GB of such a tree still fit one device beside its mesh).  F = 0 is a valid empty tree
 *         (every ray misses), F = 1 a single leaf, F = 2 one node.
 *
 * The trace: one lane per ray, the nearer child first, the other on a per-lane stack of 64 slots in LDS (the key has 63 significant
 * bits, so the tree is at most 63 deep).  A child is skipped only if box_may_hit (csrc/tri_isect.h) is false, and that is conservative
 * with respect to the rule itself, not to the geometry:
 *   (x, y)  The signs of U, V, W are exact signs of the edge functions of the COMPUTED sheared vertices: rounding is monotone, so a
 *         non-zero fp32 difference of two rounded products has the sign of the exact one, and a zero is recomputed exactly.  So a face
 *         counts only if the origin of the sheared plane lies in the closed triangle of its computed (Px, Py).  Px is a monotone
 *         function of P[kx] and of P[kz] (subtraction, multiplication by a constant and rounding all are), so over a box it lies
 *         between its values at two corners, formed with the SAME operations: x_min = (lo[kx] - o[kx]) - max(Sx zl, Sx zh),
 *         x_max = (hi[kx] - o[kx]) - min(Sx zl, Sx zh), zl = lo[kz] - o[kz], zh = hi[kz] - o[kz].  x_min > 0 or x_max < 0 puts all
 *         three Px strictly on one side of 0: the origin is outside, the signs are mixed (or the image degenerate): no ulp is needed.
 *   (t)   With U, V, W of one sign, T = sum U_i Pz_i (1 + a_i), |a_i| <= 3 e, det = sum U_i (1 + b_i), |b_i| <= 2 e, e = 2^-24, and
 *         t = (T / det)(1 + c): t is a convex combination of Pz_i (1 + a_i)(1 + c) / (1 + b_i), so it lies in the hull of the three
 *         Pz_i widened by a relative 6 e + O(e^2) < 2^-21.  Pz = Sz * (P[kz] - o[kz]) is monotone in P[kz]: the hull lies inside
 *         [Sz zl, Sz zh] formed with the same operations.  The test widens both ends by 2^-20 of their magnitude (twice the bound:
 *         the widening is itself rounded) and skips if near > best t or far < t_min; near == best t is ENTERED, since a tie may go
 *         to a smaller face index.  (The bound assumes no product underflows; coordinates of ordinary magnitude do not.)
 *   NaN   Sx, Sy, Sz are finite (|Sx|, |Sy| <= 1) and no division occurs per box, so a zero direction component or an origin on a box
 *         plane creates no 0 * inf; an overflowing difference can, and every skip is written so that a NaN operand does NOT skip.
 * i2sdf_mesh_trace_brute: every ray against every face through the same inline function: the reference route and the small-mesh route.
 *
 *   orig, dirs (n, 3); t_min, t_max (n); t (n) fp32, face (n) int32, bary (n, 2) fp32 (NULL allowed with any_hit), hit (n) uint8,
 *   status (1) int32.  0 <= n < 2^31; n = 0 still reports the face bit.  bvh: i2sdf_bvh_bytes(F) bytes, 16-byte aligned; the SAME
 *   verts, faces, F and buffer through keys, build and every trace; sorted_keys (F) int64.
 * Refused with I2SDF_EINVAL before any launch: a NULL or misaligned pointer (stream excepted; mesh pointers when F = 0 and ray
 *   pointers when n = 0 too), F outside 0..I2SDF_BVH_MAX_FACES, V outside 0..2^31-1, n outside the range, cull or any_hit not 0 / 1.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_RAYCAST_BAD_RAY 1       /* status bit 0 */
#define I2SDF_RAYCAST_BAD_FACE 2      /* status bit 1 */
#define I2SDF_RAYCAST_CULL_NONE 0
#define I2SDF_RAYCAST_CULL_BACK 1
#define I2SDF_BVH_MAX_FACES 268435456
int64_t i2sdf_bvh_bytes(int64_t F);
int i2sdf_bvh_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, void* bvh, int64_t* keys, void* stream);
int i2sdf_bvh_build(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys, void* bvh, void* stream);
int i2sdf_bvh_trace(const void* bvh, int64_t F, const float* orig, const float* dirs, const float* t_min, const float* t_max, int64_t n,
                    int32_t cull, int32_t any_hit, float* t, int32_t* face, float* bary, uint8_t* hit, int32_t* status, void* stream);
int i2sdf_mesh_trace_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* orig, const float* dirs,
                           const float* t_min, const float* t_max, int64_t n, int32_t cull, int32_t any_hit, float* t, int32_t* face,
                           float* bary, uint8_t* hit, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Closest point -- the point of a triangle mesh nearest to a query point, its distance, and the inside / outside sign: what trimesh's
 * `proximity` and open3d's compute_closest_points / compute_signed_distance answer on the host.  The reference has no such query of
 * its own (it calls those libraries), so the rule is defined here.  csrc/closest.hip, csrc/tri_closest.h; the tree is the one of "Ray
 * casting" above, unchanged.  No plan.  Every call only enqueues on `stream`: no allocation, no synchronisation, no host read.
 * tests/closest_ref.py restates the rule and the tables in numpy.
 *
 * The law.  verts (V, 3) fp32, faces (F, 3) int32, points (n, 3) fp32, one max_dist (fp32, >= 0 or +inf).
 *   Arithmetic.  fp64 on the exact images of the fp32 inputs; every operation is ONE IEEE operation, rounded to nearest, in the order
 *         written, none contracted into an FMA; a dot product x.y is (x0 y0 + x1 y1) + x2 y2.  fp64 and not the ray law's fp32: a closest
 *         point computed in fp32 is off by ulps of the COORDINATE (2.4e-7 at a coordinate of 2), so that a distance of 1e-4 to the
 *         surface -- the interesting range when an SDF is compared with a mesh -- would carry a relative error of 1e-3.
 *   Face (A, B, C) and point p (Ericson, Real-Time Collision Detection, 5.1.5); the first region that applies decides:
 *         ab = B - A, ac = C - A, ap = p - A, d1 = ab.ap, d2 = ac.ap.      d1 <= 0 and d2 <= 0: VERT_A, c = A.
 *         bp = p - B, d3 = ab.bp, d4 = ac.bp.                              d3 >= 0 and d4 <= d3: VERT_B, c = B.
 *         vc = d1 d4 - d3 d2.     vc <= 0 and d1 >= 0 and d3 <= 0: EDGE_AB, v = d1 / (d1 - d3), c = A + v ab.
 *         cp = p - C, d5 = ab.cp, d6 = ac.cp.                              d6 >= 0 and d5 <= d6: VERT_C, c = C.
 *         vb = d5 d2 - d1 d6.     vb <= 0 and d2 >= 0 and d6 <= 0: EDGE_CA, w = d2 / (d2 - d6), c = A + w ac.
 *         va = d3 d6 - d5 d4.     va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0: EDGE_BC, w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),
 *                                 c = B + w (C - B).
 *         Otherwise FACE: den = 1 / ((va + vb) + vc), v = vb den, w = vc den, c = (A + v ab) + w ac.
 *         d^2 = (p - c).(p - c).  The weights (of A, of B), in fp64: VERT_A (1, 0), VERT_B (0, 1), VERT_C (0, 0), EDGE_AB (1 - v, v),
 *         EDGE_CA (1 - w, 0), EDGE_BC (0, 1 - w), FACE ((1 - v) - w, v).
 *   Faces that are never closest: those the ray law never hits for their indices or vertices (an index outside [0, V), a non-finite
 *         vertex: they set I2SDF_CLOSEST_BAD_FACE in every query of that mesh, whatever the points), and faces whose ab x ac --
 *         (ab1 ac2 - ab2 ac1, ab2 ac0 - ab0 ac2, ab0 ac1 - ab1 ac0) -- is exactly zero in all three components: the zero-area faces
 *         marching cubes emits.
 *   Result per point: among the faces with d^2 <= (double)max_dist * (double)max_dist (a NaN d^2 fails that) the smallest d^2; among
 *         equal d^2 the smallest face index.  An order-free function of the inputs, so bitwise reproducible and the same by every
 *         route.  dist = (float)sqrt(d^2), point = (float)c, face, bary = the two weights rounded to fp32 (as in the ray caster's
 *         results), feature = one of I2SDF_CLOSEST_*.  No face counts (F = 0 too): face = -1, dist = +inf, point = bary = feature = 0.
 *         A point with a non-finite coordinate is such a miss and sets I2SDF_CLOSEST_BAD_POINT.
 *   *status: the OR of the two bits over the call.
 *   Sign (when the tables below are given): s = ((p - c).N >= 0) ? +1 : -1, sdist = s * dist (+inf on a miss), with c the unrounded
 *         fp64 closest point and N the entry of the closest feature, widened to fp64: the edge entry enormal[face][edge] for an edge,
 *         vnormal[vertex] for a vertex, and for FACE the face's own ab x ac as above (not normalised: only its direction matters).
 *         This is the angle-weighted pseudonormal test of Baerentzen and Aanaes (Signed distance computation using the angle weighted
 *         pseudonormal, IEEE TVCG 2005).  On a closed, consistently oriented mesh (right-hand normals outward) it is the inside (-) /
 *         outside (+) sign.  ON ANYTHING ELSE -- an open sheet, a soup, mixed orientations, self-intersections -- IT IS DEFINED AS
 *         ABOVE BUT MEANS NOTHING.
 *
 * The tables: vnormal (V, 3) fp32, enormal (F, 3, 3) fp32 indexed [face][AB, BC, CA].  Over the faces that may be closest, in fp64:
 *         n_f = (ab x ac) / sqrt((ab x ac).(ab x ac)), each component divided.  vnormal[i] = the sum, in ascending face index, of
 *         angle * n_f over the corners at vertex i, angle = atan2(sqrt(x.x), e1.e2), x = e1 x e2, e1 and e2 the edges from the corner to
 *         the next and to the previous vertex of the face.  enormal[f][e] = the sum, in ascending face index, of n_f over ALL faces
 *         that contain that undirected edge (two on a manifold, one on a boundary).  Each sum starts from 0, adds `angle * n_f`
 *         (one product, one sum per component) and is rounded to fp32 once.  Vertices and faces outside those faces get 0.
 *         (atan2 is not correctly rounded, so the tables are reproducible on one build and within an fp32 ulp across libraries.)
 *   Grouping works as the tree's keys do: i2sdf_closest_normal_keys writes 3 F corner keys (the vertex index) followed by 3 F
 *         half-edge keys (min << 32 | max), entry 3 f + k for corner / edge k of face f, INT64_MAX for faces that are never closest;
 *         the CALLER sorts EACH half on its own, stably, ascending, with its permutation (torch.sort(stable=True): positions 0 .. 3F-1
 *         inside the half); i2sdf_closest_normals takes both halves back, concatenated, and reduces every run in order.  No
 *         floating-point atomics: the tables are bitwise reproducible from run to run.  One lane walks one run, so a vertex shared by
 *         very many faces (a fan of 10^5) serialises; meshes from marching cubes have valence about 6.
 *
 * Two routes with the same bits.
 * i2sdf_closest_bvh: one lane per query through the tree.  The child with the smaller box distance first, the other on the per-lane
 *   stack of 64 slots in LDS (as the trace).  64 suffice for every tree i2sdf_bvh_build makes: a key has 63 significant bits (a 31-bit
 *   code, a 32-bit face index) and every level of Karras' tree splits at a further bit of the keys, so no leaf is deeper than 63; the
 *   walk is depth-first and holds at most one pending sibling per level of its current path, hence at most 63 entries.  (A buffer that
 *   is not such a tree cannot overrun the stack or loop -- pushes beyond 64 are dropped, visits are capped at 2 F -- but its result
 *   means nothing, as with the trace.)  A pending child is NOT tested again when it is popped (its box distance is not kept): it is
 *   fetched and its own children are tested against the bound of that moment.  q = (e0^2 + e1^2) + e2^2, e_k = max(lo_k - p_k, p_k - hi_k, 0), in fp64.  A child is
 *   skipped iff  q > (sqrt(b) (1 + 2^-20) + 2^-32 M)^2,  b = the best d^2 so far (max_dist^2 before there is one), M = the largest
 *   coordinate magnitude of p and of the mesh's bounds (the tree's header).  q equal to b is ENTERED, since a tie may go to a smaller
 *   face index; a NaN on either side never skips; b = +inf skips nothing.  This is conservative with respect to the RULE, not to the
 *   geometry -- the computed c can lie outside the box by rounding, so a computed d^2 can be below the true box distance:
 *   (edges, vertices)  Rounding is monotone, so the computed parameter of an edge case lies in [0, 1] exactly (d1 >= 0 >= d3 gives
 *         0 <= d1 <= d1 - d3, and so on), and each component of c = A + v ab lies between the computed A + 0 and A + ab, which is B up to
 *         2 u |B - A|, u = 2^-53.  With the roundings of p - c and of the sum of squares: sqrt(d^2) >= sqrt(q) (1 - 4 u) - 8 u M.
 *   (FACE)  With e = the error of the computed v and w, c lies within e (|ab| + |ac|) + 8 u M of the triangle.  va, vb, vc are
 *         differences of products of dot products, each good to 8 u |ab| |ac| |ap|^2-ish absolutely, and their sum is |ab x ac|^2, so
 *         e <= 2^-49 |ab| |ac| |p - A|^2 / |ab x ac|^2.  A relative term alone cannot cover this: d can be 0 while the coordinates are
 *         1000, and e (|ab| + |ac|) is then an absolute error in units of the coordinates.  The slack sqrt(b) 2^-20 + 2^-32 M covers
 *         every face with  L^3 |p - A| <= 2^28 |ab x ac|^2 (far queries, sqrt(b) ~ |p - A|, L the longest edge)  and
 *         L^5 <= 2^16 M |ab x ac|^2 (near queries, |p - A| <= L): a face of extent 2^-7 M may be a sliver of aspect 2^-11.  THE
 *         DERIVATION ASSUMES THAT; for thinner slivers the FACE branch of the rule is itself ill-conditioned and the two routes may
 *         differ there.  (It also assumes that no product underflows; coordinates of ordinary magnitude do not.)
 *   The threshold is rounded like any other fp64 expression; the factor 2 between the bounds above and the constants absorbs that.
 * i2sdf_closest_brute: every query against every face through the same inline function: the reference route and the small-mesh route.
 *
 *   points (n, 3); dist (n) fp32, point (n, 3) fp32, face (n) int32, bary (n, 2) fp32, feature (n) uint8, status (1) int32.
 *   vnormal, enormal, sdist (n) fp32: all three or all NULL.  0 <= n < 2^31; n = 0 still reports the face bit.  i2sdf_closest_bvh takes
 *   the SAME verts, faces, F the tree was built from (the sign reads them; the search reads only the tree).
 *   keys (6 F) int64; sorted_keys, perm (6 F) int64: the two sorted halves, concatenated.
 * Refused with I2SDF_EINVAL before any launch: a NULL or misaligned pointer (stream excepted; mesh pointers when F = 0, query
 *   pointers when n = 0 and vnormal when V = 0 too), F outside 0..I2SDF_BVH_MAX_FACES, V outside 0..2^31-1, n outside the range, a
 *   negative or NaN max_dist, only some of vnormal / enormal / sdist.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_CLOSEST_BAD_POINT 1     /* status bit 0 */
#define I2SDF_CLOSEST_BAD_FACE 2      /* status bit 1 */
#define I2SDF_CLOSEST_FACE 0
#define I2SDF_CLOSEST_EDGE_AB 1
#define I2SDF_CLOSEST_EDGE_BC 2
#define I2SDF_CLOSEST_EDGE_CA 3
#define I2SDF_CLOSEST_VERT_A 4
#define I2SDF_CLOSEST_VERT_B 5
#define I2SDF_CLOSEST_VERT_C 6
int i2sdf_closest_bvh(const void* bvh, const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points, int64_t n,
                      float max_dist, const float* vnormal, const float* enormal, float* dist, float* point, int32_t* face, float* bary,
                      uint8_t* feature, float* sdist, int32_t* status, void* stream);
int i2sdf_closest_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points, int64_t n, float max_dist,
                        const float* vnormal, const float* enormal, float* dist, float* point, int32_t* face, float* bary,
                        uint8_t* feature, float* sdist, int32_t* status, void* stream);
int i2sdf_closest_normal_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, int64_t* keys, int32_t* status,
                              void* stream);
int i2sdf_closest_normals(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int64_t* sorted_keys, const int64_t* perm,
                          float* vnormal, float* enormal, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Winding number -- the generalized winding number of a triangle mesh at a query point (Jacobson, Kavan, Sorkine-Hornung: Robust
 * inside-outside segmentation using generalized winding numbers, SIGGRAPH 2013): 1 inside a closed, outward-oriented mesh, 0 outside,
 * and a smooth function in between on the meshes "Closest point" gives no sign for -- open sheets, culled or cut level sets, rooms
 * seen from inside, soups.  |w| > 0.5 is the inside test.  csrc/winding.hip, csrc/tri_solid_angle.h; the tree is the one of "Ray
 * casting" above, unchanged and only read.  No plan.  Every call only enqueues on `stream`: no allocation, no synchronisation, no
 * host read.  tests/winding_ref.py restates the term, the moments and the rule in numpy.
 *
 * The law.  verts (V, 3) fp32, faces (F, 3) int32, points (n, 3) fp32.   w(q) = (1 / 4 pi) sum_f Omega_f(q).
 *   Arithmetic.  fp64 on the exact images of the fp32 inputs; every operation is ONE IEEE operation, rounded to nearest, in the order
 *         written, none contracted into an FMA; a dot product x.y is (x0 y0 + x1 y1) + x2 y2.
 *   Face (A, B, C) and point q (Van Oosterom and Strackee, The solid angle of a plane triangle, IEEE Trans. Biomed. Eng. 1983):
 *         a = A - q, b = B - q, c = C - q;  la = sqrt(a.a), lb = sqrt(b.b), lc = sqrt(c.c);  x = b x c =
 *         (b1 c2 - b2 c1, b2 c0 - b0 c2, b0 c1 - b1 c0);  det = a.x;  den = (((la lb) lc + (a.b) lc) + (b.c) la) + (c.a) lb;
 *         Omega = 2 atan2(det, den).  Positive when the right-hand normal (B - A) x (C - A) points away from q.
 *         atan2 is the library's: it is not correctly rounded, so w is reproducible on one build and within the library's bound
 *         times the number of faces summed across builds; det and den are the same bits everywhere.
 *   Faces that contribute 0: those the ray law never hits for their indices or vertices (an index outside [0, V), a non-finite
 *         vertex: they set I2SDF_WINDING_BAD_FACE in every query of that mesh, whatever the points).  Zero-area faces are NOT taken
 *         out: their det is 0 up to rounding and the formula gives 0 (or +-2 pi on the degenerate segment itself).
 *   A point with a non-finite coordinate gives NaN and sets I2SDF_WINDING_BAD_POINT.  A point ON the surface gets what the formula
 *         gives -- atan2(0, 0) = 0 at a vertex and where den cancels inside an edge, atan2(+-0, < 0) = +-pi inside a face -- always
 *         finite.  F = 0: w = 0.
 *   w = sum / (4 pi), 4 pi = 4 * M_PI as an fp64 constant, one division.  *status: the OR of the two bits over the call.
 *
 * The far field (Barill, Dickson, Schmidt, Levin, Jacobson: Fast winding numbers for soups and clouds, SIGGRAPH 2018; orders 0, 1).
 *   Per internal node of the tree, over the faces below it (a_f n_f = 1/2 (B - A) x (C - A) the area vector, each component one
 *   difference of products times 0.5; a_f = sqrt of its dot with itself; c_f = ((A + B) + C) / 3 the face centroid):
 *         p~ = (sum a_f c_f) / (sum a_f)        the area-weighted centroid;
 *         N0 = sum a_f n_f;     N1 = sum (c_f - p~) (x) (a_f n_f), N1_ij = (c_f - p~)_i (a_f n_f)_j -- exact for triangles;
 *         r  = the largest distance from p~ to a corner of the node's box (the union of the two child boxes the tree stores):
 *              e_k = max(p~_k - lo_k, hi_k - p~_k), r = sqrt(e.e).  Conservative: every face below lies inside the box.
 *   With rho = p~ - q, d2 = rho.rho: iff  d2 > beta^2 r^2  (fp64; beta^2 = (double)beta (double)beta, r^2 = r r, one product each; a
 *   NaN on either side is "no") the node contributes
 *         Omega ~ rho.N0 / d^3 + ((N1_00 + N1_11) + N1_22) / d^3 - 3 (sum_ij (rho_i rho_j) N1_ji) / d^5,
 *         d = sqrt(d2), d^3 = d2 d, d^5 = d^3 d2, the double sum i-major from 0, and nothing below it is visited; otherwise both
 *   children are visited, child 0 first.  A leaf contributes the exact term.  The sum is fp64 in visit order, so the result is a
 *   fixed function of (tree, table, q, beta) -- bitwise reproducible -- but NOT the same bits as the brute route.
 *   beta = +inf accepts no node (inf * 0 is NaN, also "no"): the exact sum in tree order.  beta = 2 is the default of the paper.
 *   What the approximation costs is measured in tests/test_winding_ref.py, against the exact sum, at queries at least 0.05 of the
 *   diameter from the surface (icosphere of 1280 faces, an open cap of it, a 3000-face soup; the Karras tree, box radii):
 *           icosphere(3), 1280 faces   beta = 2: 5.11e-2 (39 terms per query)    beta = 3: 2.15e-2 (97 terms per query)
 *           open cap of it, 456 faces  beta = 2: 2.17e-2 (28)                    beta = 3: 7.65e-3 (65)
 *           soup, 3000 faces           beta = 2: 3.11e-3 (50)                    beta = 3: 1.04e-3 (178)
 *         (500 queries each.  On meshes this small the order-1 term does not lower the maximum; it does lower the far field of a
 *         single node as the law says, d^-4 against d^-3: the same test file holds that.)
 *   No bar is set for these; the properties held are that round(w) is round(w_exact) at every such query at beta = 2 and that the
 *   largest error at beta = 3 is below that at beta = 2.
 *
 * The moments are composable, so one bottom-up pass over the tree's parent links fits them (i2sdf_winding_moments): per node
 *         A = sum a_f,  S = sum a_f c_f,  N0,  M = sum (c_f - o) (x) (a_f n_f),   o = ((lo + hi) 0.5) of the root box (the header),
 *   so that a mesh shifted by +1000 does not cancel; a parent is child 0 + child 1 in that order whatever the arrival order, so the
 *   table is bitwise reproducible; then p~ = S / A, N1_ij = M_ij - (p~_i - o_i) N0_j.  A = 0 (nothing but degenerate or rejected faces
 *   below) gives r = +inf: such a node is always descended.
 *   The table: 16 fp64 per internal node i at moments + 128 i: p~[3], r, N0[3], N1[9] (row-major).  i2sdf_winding_moments_bytes(F) =
 *   128 max(F - 1, 0) + the build's own arrival counters (4 bytes per node, rounded up to 16) + 16: never 0 for a legal F, 0 for
 *   F < 0 or F > I2SDF_BVH_MAX_FACES.  The tree buffer and i2sdf_bvh_bytes are unchanged; the tree is not written (the counters
 *   of its own build are left alone, so a tree may be shared between streams).
 *
 * i2sdf_winding_bvh: one lane per query, child 0 first, child 1 on the per-lane stack of 64 slots in LDS (as the trace; the tree is at
 *   most 63 deep, pushes beyond 64 are dropped and visits capped at 2 F for a buffer that is not such a tree).
 * i2sdf_winding_brute: every query against every face in ascending face order through the same inline function: the reference route
 *   and the small-mesh route.
 *
 *   points (n, 3) fp32; w_out (n) fp64; status (1) int32.  0 <= n < 2^31; n = 0 still reports the face bit.  bvh: the buffer
 *   i2sdf_bvh_build filled for the same F; moments: i2sdf_winding_moments_bytes(F) bytes, 16-byte aligned, filled by
 *   i2sdf_winding_moments from that tree.  F = 0, 1 (no node: the table is empty) and 2 are legal.
 * Refused with I2SDF_EINVAL before any launch: a NULL or misaligned pointer (stream excepted; mesh pointers when F = 0 and query
 *   pointers when n = 0 too), F outside 0..I2SDF_BVH_MAX_FACES, V outside 0..2^31-1, n outside the range, a negative or NaN beta.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_WINDING_BAD_POINT 1     /* status bit 0 */
#define I2SDF_WINDING_BAD_FACE 2      /* status bit 1 */
int64_t i2sdf_winding_moments_bytes(int64_t F);
int i2sdf_winding_moments(const void* bvh, int64_t F, void* moments, void* stream);
int i2sdf_winding_bvh(const void* bvh, const void* moments, int64_t F, const float* points, int64_t n, float beta, double* w_out,
                      int32_t* status, void* stream);
int i2sdf_winding_brute(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* points, int64_t n, double* w_out,
                        int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh simplification -- vertex clustering with quadric placement (Lindstrom, Out-of-core simplification of large polygonal models,
 * SIGGRAPH 2000; DeCoro and Tatarchuk, Real-time mesh simplification using the GPU, I3D 2007), mesh cleaning, and the edge statistics
 * of a topology report: the step between the mesh producers (marching cubes, TSDF fusion) and the consumers (the tree, closest point,
 * winding number, the scores).  The decimation that needs no priority queue and whose result is an order-free function of its input.
 * csrc/simplify.hip, csrc/quadric.h.  No plan.  Every call only enqueues on `stream`: no allocation, no synchronisation, no host
 * read; the caller sorts (stable) and scans between the calls and reads the counts that size the results.  tests/simplify_ref.py
 * restates the law in numpy.
 *
 * The law.  verts (V, 3) fp32, faces (F, 3) int32, normals (V, 3) fp32 or none; cell edge h, finite and positive; reg, finite and
 * positive (1e-3: Lindstrom's truncation level).
 *   Arithmetic.  fp64 on the exact images of the fp32 inputs; every operation is ONE IEEE operation, rounded to nearest, in the order
 *         written, none contracted into an FMA; a dot product x.y is (x0 y0 + x1 y1) + x2 y2.
 *   Grid.  Exactly that of "Point sets" (voxel_down_sample): lo = min(verts) - h / 2 per axis over ALL vertices, referenced by a face or
 *         not; cell index = floor((p - lo) / h), 21 bits per axis, key = ix << 42 | iy << 21 | iz; a non-finite coordinate or an index
 *         beyond 21 bits is refused through the status word of i2sdf_points_voxel_keys.  Cells are numbered in ascending key order, i.e.
 *         ascending (ix, iy, iz).  Cell centre cc_k = lo_k + (i_k + 0.5) h.
 *   Face quadric about a centre cc.  For face (a, b, c):  n = (b - a) x (c - a) = (e1 g2 - e2 g1, e2 g0 - e0 g2, e0 g1 - e1 g0) with
 *         e = b - a, g = c - a (not normalised: a face weighs in by its squared area);  d = -(n . (a - cc)), taken about the centre of
 *         the cell it is added to, so that a mesh at +1000 does not cancel;  nine values: n0 n0, n0 n1, n0 n2, n1 n1, n1 n2, n2 n2 (A)
 *         and d n0, d n1, d n2 (bvec).
 *   Corners.  The quadric of face f is added once per corner to the cell of that corner (a face inside one cell adds three times:
 *         measured better than once per distinct cell, 6.3e-3 against 7.7e-3 of the radius on the icosphere at h = 0.25).  A face with
 *         an index outside [0, V) is never dereferenced: it sets I2SDF_SIMPLIFY_BAD_FACE and adds nothing.
 *   Sums.  The 3 F corners are grouped by a stable sort of their cell id, so a cell's run is in ascending corner index 3 f + k.  The
 *         corner at position j of its run (j = 0, 1, ...) belongs to lane j mod 64; a lane adds its corners in ascending j into nine
 *         partials that start at +0; the 64 partials p[0..63] of a value are combined by the xor butterfly: for s = 32, 16, 8, 4, 2, 1:
 *         p[l] <- p[l] + p[l xor s] for all l at once; the sum is p[0].  No floating-point atomics: the order does not depend on arrival.
 *   Cell mean.  m = (the sum of the cell's vertices in ascending index, from +0) / count - cc, per axis.
 *   Representative, I2SDF_SIMPLIFY_QUADRIC.  tr = (A00 + A11) + A22;  lambda = reg tr;  M = A + lambda I;  r = lambda m - bvec;
 *         cofactors c00 = M11 M22 - M12 M12, c01 = M02 M12 - M01 M22, c02 = M01 M12 - M02 M11, c11 = M00 M22 - M02 M02,
 *         c12 = M01 M02 - M00 M12, c22 = M00 M11 - M01 M01;  det = M0 . (c00, c01, c02);  x_i = ((c_i0, c_i1, c_i2) . r) / det.
 *         If tr is not finite and positive, or |x_i| <= h / 2 fails for some i (the minimiser left its cell, or is not a number):
 *         x = m and the cell's fallback flag is set.  Output vertex = fp32(cc + x).
 *   Representative, I2SDF_SIMPLIFY_AVERAGE.  fp32(sum / count): bit-equal to the matching row of i2sdf_points_voxel_mean.  No flag.
 *   Normals (when given).  s = the sum of the cell's input normals in ascending vertex index; len = sqrt(s . s); fp32(s / len), zeros
 *         when len is not finite and positive.
 *   Faces.  Corners are replaced by cell ids.  A face with two corners in one cell is dropped.  Two surviving faces with the same
 *         cyclic sequence of cells (the same orientation) are duplicates: the smallest input face index is kept; opposite orientations
 *         are both kept.  The key of a face is the lexicographically smallest rotation (t0, t1, t2) of its triple: key_hi = t0,
 *         key_lo = t1 << 32 | t2; two stable sorts (by key_lo, then by key_hi) bring equal keys together in ascending face order.
 *         Output faces come in ascending input face index with the corner order of the input; output vertices are the cells a
 *         surviving face references, in ascending (ix, iy, iz) (i2sdf_mesh_compact_mark / _gather over the cell table).
 *   Cleaning uses the same face kernel with another vertex map: vertices with bit-equal positions (-0.0 = +0.0) merged into the smallest
 *         index among them; I2SDF_SIMPLIFY_DROP_REPEATED drops a face with a repeated (mapped) index, I2SDF_SIMPLIFY_DROP_ZERO_AREA one
 *         whose n above is exactly (0, 0, 0) -- "Closest point"'s never-closest rule.  Without DROP_REPEATED the key is still one per
 *         cyclic sequence.
 *   F = 0, 1, 2 and V = 0 are legal.
 *
 * i2sdf_simplify_vertex_cells: from the sorted vertex keys, the permutation and the inclusive scan of i2sdf_points_voxel_heads:
 *   vertex_cell (V) = the cell of every vertex, cell_start (n_cells + 1) = where every cell's run begins in the sorted order (the last
 *   entry is V).
 * i2sdf_simplify_corner_keys: corner_keys (3 F) int32 = the cell of every corner; n_cells for the corners of a refused face.
 * i2sdf_simplify_corner_runs: corner_runs (n_cells, 2) int32 = begin and end of every cell's corners in the sorted corner order
 *   (0, 0 for a cell no face touches).
 * i2sdf_simplify_cells: the hot kernel, one wave per cell: out_verts (n_cells, 3), out_normals (n_cells, 3; untouched when normals is
 *   NULL), fallback (n_cells) uint8.  bounds: what i2sdf_points_bounds wrote.  With I2SDF_SIMPLIFY_AVERAGE faces, corner_perm and
 *   corner_runs are not read.
 * i2sdf_simplify_face_keys: out_faces (F, 3) = the mapped corners (vertex_map NULL: the identity; -1 for a refused face), the key pair
 *   (INT64_MAX twice for a face that is not kept).  A face with an index outside [0, V), or mapped outside [0, n_map), sets
 *   I2SDF_SIMPLIFY_BAD_FACE and is not kept.
 * i2sdf_simplify_run_heads: keep[perm[i]] = 1 where sorted entry i is the first of its run of equal key pairs and not INT64_MAX twice,
 *   else 0; first[i] = i at the first of a run, else 0 (its running maximum is the head of every entry's run).  Either may be NULL.
 * i2sdf_simplify_position_keys: key_hi = the bits of x, key_lo = the bits of y << 32 | the bits of z, -0.0 as +0.0.
 *
 * Edge statistics (the topology report).  Faces with an index outside [0, V) set I2SDF_SIMPLIFY_BAD_FACE and are left out; faces with
 *   a repeated index are counted and their edges left out.  Of the others: every side is an undirected edge (min, max) with a
 *   direction bit; after the caller's sort, an edge with 1 face is a boundary edge, with 2 faces a manifold edge, with 3 or more a
 *   non-manifold edge; a 2-face edge traversed in the same direction by both is misoriented.  counts (I2SDF_TOPO_COUNTS) int64, integer
 *   atomics only.  Euler = VERTICES - EDGES + FACES, over the counted faces and the vertices they reference.
 * i2sdf_mesh_edge_stats_keys: clears counts and vflag (V) int32, writes keys (3 F; INT64_MAX for a side left out), marks and counts
 *   the referenced vertices, counts the faces.  i2sdf_mesh_edge_stats: the edge counts from the sorted keys, then the Euler number.
 *
 * Refused with I2SDF_EINVAL before any launch: a NULL or misaligned pointer (stream excepted; pointers of empty arrays too), V or
 *   n_cells outside 0..2^31-1, F outside 0..(2^31-1)/3, n_cells > V, a voxel_size or reg that is not finite and positive, an unknown
 *   contraction or flag.
 * ---------------------------------------------------------------------------------------------- */
#define I2SDF_SIMPLIFY_QUADRIC 0
#define I2SDF_SIMPLIFY_AVERAGE 1
#define I2SDF_SIMPLIFY_BAD_FACE 1          /* status bit 0 */
#define I2SDF_SIMPLIFY_DROP_REPEATED 1     /* flags of i2sdf_simplify_face_keys */
#define I2SDF_SIMPLIFY_DROP_ZERO_AREA 2
#define I2SDF_TOPO_EDGES 0                 /* indices into counts */
#define I2SDF_TOPO_BOUNDARY 1
#define I2SDF_TOPO_MANIFOLD 2
#define I2SDF_TOPO_NONMANIFOLD 3
#define I2SDF_TOPO_MISORIENTED 4
#define I2SDF_TOPO_REPEATED_FACES 5
#define I2SDF_TOPO_VERTICES 6
#define I2SDF_TOPO_EULER 7
#define I2SDF_TOPO_FACES 8
#define I2SDF_TOPO_COUNTS 10               /* (entry 9 is reserved and 0) */
int i2sdf_simplify_vertex_cells(const int64_t* sorted_keys, const int64_t* perm, const int32_t* head_scan, int64_t V, int64_t n_cells,
                                int32_t* vertex_cell, int32_t* cell_start, void* stream);
int i2sdf_simplify_corner_keys(const int32_t* faces, int64_t F, int64_t V, const int32_t* vertex_cell, int64_t n_cells, int32_t* corner_keys,
                               int32_t* status, void* stream);
int i2sdf_simplify_corner_runs(const int32_t* sorted_corner_keys, int64_t F, int64_t n_cells, int32_t* corner_runs, void* stream);
int i2sdf_simplify_cells(const float* verts, const float* normals, int64_t V, const int32_t* faces, int64_t F, const int32_t* bounds,
                         double voxel_size, double reg, int32_t contraction, const int64_t* sorted_keys, const int64_t* perm,
                         const int32_t* cell_start, const int64_t* corner_perm, const int32_t* corner_runs, int64_t n_cells, float* out_verts,
                         float* out_normals, uint8_t* fallback, void* stream);
int i2sdf_simplify_face_keys(const float* verts, int64_t V, const int32_t* faces, int64_t F, const int32_t* vertex_map, int64_t n_map,
                             int32_t flags, int32_t* out_faces, int64_t* key_hi, int64_t* key_lo, int32_t* status, void* stream);
int i2sdf_simplify_run_heads(const int64_t* sorted_hi, const int64_t* sorted_lo, const int64_t* perm, int64_t n, uint8_t* keep,
                             int32_t* first, void* stream);
int i2sdf_simplify_position_keys(const float* verts, int64_t V, int64_t* key_hi, int64_t* key_lo, void* stream);
int i2sdf_mesh_edge_stats_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, int32_t* vflag, int64_t* counts, int32_t* status,
                               void* stream);
int i2sdf_mesh_edge_stats(const int64_t* sorted_keys, int64_t F, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* I2SDF_H */
