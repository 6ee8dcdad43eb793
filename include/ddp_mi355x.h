/* ddp_mi355x.h - C ABI of libddp_mi355x.so: the MI355X (gfx950) implementation of the DDP
 * multi-step denoising inference loop.
 *
 * The reference has no FFI for this path: the loop is Python/torch
 * (segmentation/mmseg/models/segmentors/ddp.py:215-246 `DDP.ddim_sample`, :248-290 `ddpm_sample`;
 * depth/depth/models/depther/ddp.py:229-247 `DDP.sample`;
 * bev/mmdet3d/models/fusion_models/ddp.py:268-301 `DDP.ddim_sample`) calling
 * `DeformableHeadWithTime.forward` (segmentation/mmseg/models/decode_heads/deformable_head_with_time.py:90-132)
 * and, below it, mmcv's only custom kernel `ext_module.ms_deform_attn_forward`
 * (controlnet/annotator/uniformer/mmcv/ops/multi_scale_deform_attn.py:47-53).  This header is the
 * boundary a maintainer would bind instead (ctypes stub: INTEGRATION.md); `ddp_amd`'s registered
 * drop-in classes call exactly these symbols.
 *
 * Conventions
 *  - plain C, no torch types.  Every pointer named `d_*` or living in `ddp_weights` is a DEVICE
 *    pointer to contiguous fp32, 16-byte aligned.  The caller (PyTorch) owns every buffer,
 *    including the workspace; the library never allocates or frees device memory.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream);
 *    no host synchronisation happens inside any entry point.
 *  - return value: DDP_OK (0) or a negative DDP_E_* code; `ddp_last_error()` gives a message.
 *    No exception crosses the boundary.
 *  - thread-safety: re-entrant per (workspace, stream); no global mutable state except the
 *    thread-local last-error string and the measurement hook at the end of this header
 *    (ddp_profile_*: ONE process-wide session, armed by bench.py only - not thread-safe, see there).
 *  - fixed architecture constants of the reference configs: embed 256, 8 heads x 32, 4 points,
 *    1 level, FFN 1024, time dim 1024, 16 learned sinusoid features.
 */
#ifndef DDP_MI355X_H
#define DDP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_ABI_VERSION 7
#define DDP_MAX_LAYERS 12
#define DDP_MAX_STEPS 64
#define DDP_EMBED 256
#define DDP_HEADS 8
#define DDP_POINTS 4
#define DDP_FFN 1024
#define DDP_TIME_DIM 1024
#define DDP_SINU_FEATS 17 /* 1 + 16 */
#define DDP_SAMP_STRIDE 96 /* per token: 64 sample coords (head,point,xy) + 32 weights */

enum { DDP_OK = 0, DDP_E_BADCFG = -1, DDP_E_ALIGN = -2, DDP_E_LAUNCH = -3, DDP_E_NULL = -4 };
enum { DDP_TASK_SEG = 0, DDP_TASK_DEPTH = 1, DDP_TASK_BEV = 2 };
enum { DDP_SAMPLER_DDIM = 0, DDP_SAMPLER_DDPM = 1 };
/* How the channel contractions are evaluated (both are fp32-accurate; csrc/gemm_f32.h, csrc/gemm_bf16x3.h):
 *   DDP_GEMM_F32_MFMA   exact f32-input MFMA (v_mfma_f32_32x32x2_f32), 157 TFLOP/s ceiling
 *   DDP_GEMM_BF16X3     every fp32 operand is split exactly into 3 bf16 pieces and the 6 significant cross
 *                       products run on the bf16 matrix cores with fp32 accumulation (error <= ~3 * 2^-24 per
 *                       product, i.e. fp32 round-off class), 417 TFLOP/s fp32-equivalent ceiling */
enum { DDP_GEMM_F32_MFMA = 0, DDP_GEMM_BF16X3 = 1 };
/* Binned depth head (ddp_cfg.depth_n_bins > 0; depth/depth/models/decode_heads/decode_head.py:233-250): how the n_bins logits of a
 * pixel become the weights of the bin centres.  LINEAR: relu(l) + 0.1, / sum;  SOFTMAX: softmax;  SIGMOID: sigmoid(l), / sum. */
enum { DDP_DEPTH_NORM_LINEAR = 0, DDP_DEPTH_NORM_SOFTMAX = 1, DDP_DEPTH_NORM_SIGMOID = 2 };
#define DDP_MAX_DEPTH_BINS 256
/* bev grid_transform.prescale_factor: the prescaled map (floor(h p), floor(w p)) gets a workspace buffer of its own (B r maps of 256
 * channels).  Two bounds, both checked by validate(): the library carves it up to DDP_BEV_MAX_PRESCALE_AREA times the pixels of the
 * map itself (p <= 4 on both axes), and - like the head grid - up to DDP_MAX_CALL_TOKENS prescaled tokens per call
 * (batch * randsteps * floor(h p) * floor(w p)), which keeps 32-bit row counters and row * 1024 offsets safe */
#define DDP_BEV_MAX_PRESCALE_AREA 16
#define DDP_MAX_CALL_TOKENS 1464843 /* 1.5e9 / 1024 */
/* ddp_cfg.flags (diagnostics, bf16x3 engine): run the decoder layer / the head of a step as the separate tile GEMMs they
 * were fused from (identical arithmetic per contraction; used by same-box A/B runs and by the parity tests that keep
 * the unfused kernels covered).  UNFUSED_LAYER implies the unfused step head and seg tail as well.
 * GATHER_GUESS_ZERO: the LDS-staged gather starts every window from a zero guess of the head's mean sampling offset instead
 * of the mean of its offset biases, which forces its "actual mean is far from the guess: refill" branch (identical results:
 * the window origin only decides which taps are served from LDS).
 * FORCE_X0 (seg, test instrument): teacher forcing.  Every step feeds back the class the CALLER supplies (ddp_x0_trace's
 * buffer, filled before ddp_sample) instead of its own argmax (ddp.py:235); scores, softmax accumulation, update and
 * everything else are unchanged, and the step's OWN argmax is still recorded next to the supplied one.  With the
 * decisions of a reference run supplied, the loop has no discontinuity left and the outputs must agree with that run to
 * rounding (tests/test_full_size_parity.py).  Separate kernel instantiations: the product's tails are not touched. */
enum { DDP_FLAG_UNFUSED_LAYER = 1, DDP_FLAG_UNFUSED_PROLOGUE = 2, DDP_FLAG_RECORD_X0 = 4, DDP_FLAG_GATHER_GUESS_ZERO = 8,
       DDP_FLAG_FCN_PREPARED = 16 /* ddp_sample_fcn: the workspace holds what ddp_prepare_fcn wrote */,
       DDP_FLAG_FORCE_X0 = 32,
       /* depth head variants (depth/depth/models/decode_heads/decode_head.py:252-262; model configuration, not diagnostics): */
       DDP_FLAG_DEPTH_SCALE_UP = 256 /* depth = sigmoid(conv_depth) * eps, eps = max_depth (or 1 with NO_EPS) instead of relu(conv_depth) + eps */,
       DDP_FLAG_DEPTH_NO_EPS = 512 /* use_eps=False: eps = 0 (relu branch) / 1 (scale_up branch) instead of min_depth / max_depth */,
       DDP_FLAG_STEP_RECORD = 1024 /* model surface, all three tasks, both samplers, both engines, ddp_sample and ddp_sample_fcn: keep every
                                      step's prediction (the reference's `outs`, segmentors/ddp.py:241-245) and compute the step-
                                      disagreement map on the device - see ddp_x0_trace.  Refused together with DDP_FLAG_FORCE_X0; any
                                      other flag may be combined.  Clear: launches, workspace sizes and outputs are unchanged */,
       DDP_FLAG_SEEDED_NOISE = 2048 /* model surface, all three tasks, both samplers, both engines, ddp_sample and ddp_sample_fcn: the start
                                       noise and the ddpm step noise are generated on the device from a key instead of being read from
                                       the caller's tensors - see "Seeded noise" below.  Any other flag may be combined.  Clear: launches,
                                       workspace sizes and outputs are unchanged */,
       DDP_FLAG_DDPM_CHAIN = 4096 /* model surface, seg + DDP_SAMPLER_DDPM through ddp_sample only (any other task or sampler, and
                                     ddp_sample_fcn, refuse it): ddpm_sample on the fused step boundary of the ddim sampler - the first
                                     step's head from NCHW, the u chain and the last layer + tail kernel (k_layer MODE 7 / 4 / 6) - with
                                     the step noise folded into u by ONE pre-pass per noise-adding step (csrc/ddp_ddpm_chain.hip:
                                     U <- ua' U + std (E W_m^T), ua' = ((1 - c) / alpha) alpha_next; the tail then runs u' = U + c alpha_next
                                     T[argmax]; a step without noise runs the tail with (ua', c alpha_next); the last step has no update,
                                     no noise fill or transpose and no pre-pass).  The same operators regrouped: results agree with the
                                     flag-clear sampler to rounding, not bit for bit.  Without effect on the fp32 engine and with
                                     DDP_FLAG_UNFUSED_LAYER / _UNFUSED_PROLOGUE (the flag-clear launches run).  Combines with
                                     DDP_FLAG_UNFUSED_TAIL, _SB_HEAD, _RECORD_X0, _FORCE_X0, _STEP_RECORD, _SEEDED_NOISE and
                                     _GATHER_GUESS_ZERO as the ddim chain does.  Nothing new is carved: ddp_query_workspace and
                                     ddp_query_const_workspace return the bytes of the cfg without the flag.  Clear: launches, workspace
                                     sizes and outputs are unchanged */,
       DDP_FLAG_X0_HINTS = 16384 /* model surface, seg and depth through ddp_sample, both samplers, both engines, every route: where the
                                    caller knows the answer, that is fed back as x0 at every step in place of the model's own
                                    prediction - see "x0 hints" below.  Refused (DDP_E_BADCFG) for bev, by ddp_sample_fcn and its
                                    workspace query, together with DDP_FLAG_FORCE_X0 and for seg with 256 classes; ddp_head_forward
                                    ignores it.  Clear: launches, workspace sizes and outputs are unchanged */,
       DDP_FLAG_PRIOR_START = 65536 /* model surface, all three tasks, both samplers, both engines, every route, through ddp_sample
                                       only: the chain starts from the caller's prior map noised to steps[0] (the time the host layer
                                       calls t_start) instead of from pure noise - see "prior start" below.  Combines with every other
                                       flag of ddp_sample.  Refused (DDP_E_BADCFG) by ddp_sample_fcn, ddp_prepare_fcn and
                                       ddp_sample_fcn_workspace and for bev with more than 32 classes; ddp_head_forward ignores it.
                                       (Bits 8192 and 32768 stay undefined.)  Clear: launches, workspace sizes and outputs are
                                       unchanged */,
       DDP_FLAG_CLASS_PRIOR = 131072 /* model surface, seg through ddp_sample, both samplers, both engines, every route: a per-image
                                        additive prior on the conv_seg scores, read from a caller-written table (B, 256) and applied
                                        in front of everything that reads the scores - see "class prior" below.  Combines with every
                                        other flag of ddp_sample.  Refused (DDP_E_BADCFG) for depth and bev and by ddp_sample_fcn,
                                        ddp_prepare_fcn and ddp_sample_fcn_workspace; ddp_head_forward ignores it.  (Bits 8192 and
                                        32768 stay undefined; the bits above this one: DDP_FLAG_SCORE_PRIOR.)  Clear: launches, workspace sizes
                                        and outputs are unchanged */,
       DDP_FLAG_SCORE_PRIOR = 1048576 /* model surface, seg through ddp_sample, both samplers, both engines, every route: a per-pixel
                                         additive prior on the conv_seg scores, read from a caller-written NCHW map (B, num_classes,
                                         h, w) and applied in front of everything that reads the scores - see "score prior" below.
                                         Combines with every other flag of ddp_sample, DDP_FLAG_CLASS_PRIOR (both priors add) and 256
                                         classes included.  Refused (DDP_E_BADCFG) for depth and bev and by ddp_sample_fcn,
                                         ddp_prepare_fcn and ddp_sample_fcn_workspace; ddp_head_forward ignores it.  (Bits 8192, 32768,
                                         262144 and 524288 stay undefined and every bit above this one is refused.)  Clear: launches,
                                         workspace sizes and outputs are unchanged */,
       DDP_FLAG_SB_HEAD = 128 /* the first step's head as the four launches it was fused from (NCHW -> split fragments of x and of
                                  the start noise, the x-projection GEMM, k_layer MODE 2) instead of ONE kernel that reads the
                                  caller's NCHW tensors directly (k_layer MODE 7); A/B runs and parity tests of the separate kernels */,
       DDP_FLAG_UNFUSED_TAIL = 64 /* the step boundary as the launches it was fused from (same-box A/B runs, parity tests of the separate
                                     kernels).  seg: the last decoder layer of a step and the step's tail as two kernels (k_layer MODE 0 +
                                     MODE 4 / 1 instead of MODE 6; identical arithmetic, bit-identical results).  depth: the GEMM step
                                     head (k_layer MODE 3), the 9-tap head GEMM on the SB layer output and k_depth_update per step instead
                                     of k_depth_head + k_layer MODE 10 / MODE 9.  bev: the concat-conv GEMM, grid resampling, head GEMM and
                                     k_bev_update on the 256-channel map per step instead of the u chain (k_bev_u_update, k_bev_q, k_layer
                                     MODE 8).  depth / bev: the same operators regrouped - results agree to rounding, not bit for bit.
                                     bev with the 3x3 conv_seg: the same launches with the 3x3 head (+ k_bev_seg3) in place of the head GEMM */ };

/* Problem description.  Mirrors the constructor kwargs of the reference `DDP` classes
 * (segmentors/ddp.py:57-67; depther/ddp.py:42-54; fusion_models/ddp.py:67-80). */
typedef struct ddp_cfg {
  int32_t abi_version;    /* must be DDP_ABI_VERSION */
  int32_t task;           /* DDP_TASK_* */
  int32_t sampler;        /* DDP_SAMPLER_* (ddpm: seg only) */
  int32_t batch;          /* B independent images (the reference loop is b = 1 per call) */
  int32_t randsteps;      /* r noise replicas per image */
  int32_t timesteps;      /* K sampling steps, <= DDP_MAX_STEPS */
  int32_t num_layers;     /* L encoder layers, <= DDP_MAX_LAYERS */
  int32_t num_classes;    /* K_cls (seg, bev <= 256); ignored for depth */
  int32_t feat_channels;  /* channels of x (multiple of 32) */
  int32_t h, w;           /* spatial size of x / of the noisy map */
  int32_t head_h, head_w; /* token grid of the encoder: == h,w except bev (grid transform output) */
  int32_t accumulation;   /* seg: average softmax over steps (ddp.py:241-245); bev always accumulates */
  float bit_scale;
  float min_depth, max_depth; /* depth */
  float threshold;            /* bev x0 threshold (fusion_models/ddp.py:290) */
  /* bev grid transform (heads/segm/deformable_head_with_time.py:70-97): per axis (y then x)
   * input [min,max], output first centre and step: c_k = out_first + k * out_step */
  float bev_in_min[2], bev_in_max[2], bev_out_first[2], bev_out_step[2];
  int32_t gemm_mode;          /* DDP_GEMM_* */
  int32_t flags;              /* DDP_FLAG_* (0 = the product path) */
  /* ---- ABI 6 (depth only; a zeroed field keeps the behaviour of ABI 5) ---- */
  int32_t depth_n_bins;       /* 0: regression head (conv_depth to 1 channel); 1..DDP_MAX_DEPTH_BINS: binned head (classify=True):
                                 conv_depth to n_bins channels, normalised over the bins (depth_norm), expectation over the bin
                                 centres ddp_weights.depth_bins.  DDP_FLAG_DEPTH_SCALE_UP / _NO_EPS play no part there */
  int32_t depth_norm;         /* DDP_DEPTH_NORM_* (binned head) */
  float head_min_depth, head_max_depth; /* the decode head's depth range: eps of the regression head (decode_head.py:258-266).
                                           0 / 0: the same as min_depth / max_depth, which keep normalising x0 (depther/ddp.py:240) */
  /* ---- ABI 7 (bev only; a zeroed field keeps the behaviour of ABI 6) ---- */
  float bev_prescale;         /* grid_transform.prescale_factor (heads/segm/deformable_head_with_time.py:70-77): 0 or 1 = none; else a
                                 bilinear F.interpolate(scale_factor = p, align_corners = False) of the feature map to (floor(h p),
                                 floor(w p)) runs in front of the grid resampling, whose normalisation then uses the prescaled size.
                                 Both prescaled sides must be >= 1, their product <= DDP_BEV_MAX_PRESCALE_AREA * h * w and
                                 batch * randsteps * product <= DDP_MAX_CALL_TOKENS.  THE FIELD IS A FLOAT and the library computes
                                 the sizes as floor(h * (double)bev_prescale): for a factor float cannot hold exactly the rounded
                                 value can give one row / column fewer than PyTorch's floor(h * p) of the Python double (0.9 on a
                                 10-wide map: 8 against 9).  The caller must pass a float whose sizes equal those of its double -
                                 the neighbouring float above does where rounding went below - or refuse the factor
                                 (ddp_amd.engine.check_bev_head does both).  The source coordinates use 1 / p of the value passed:
                                 a relative difference of <= 2^-23 from PyTorch's */
  int32_t bev_seg_kernel;     /* seg_conv_kernel (:136-139): 0 or 1 = the 1x1 conv_seg; 3 = Conv2d(256, K_cls, 3, padding = 1) with
                                 ddp_weights.head_w (K_cls,256,3,3).  Other values are refused (the reference builds a 3x3 for ANY
                                 value other than 1) */
} ddp_cfg;

typedef struct ddp_layer_weights {            /* decode_head.encoder.layers.<l>.* */
  const float *sampling_offsets_w, *sampling_offsets_b;   /* (64,256),(64)  attentions.0.sampling_offsets */
  const float *attention_weights_w, *attention_weights_b; /* (32,256),(32)  attentions.0.attention_weights */
  const float *value_proj_w, *value_proj_b;               /* (256,256),(256) */
  const float *output_proj_w, *output_proj_b;             /* (256,256),(256) */
  const float *ffn0_w, *ffn0_b;                           /* (1024,256),(1024) ffns.0.layers.0.0 */
  const float *ffn1_w, *ffn1_b;                           /* (256,1024),(256)  ffns.0.layers.1 */
  const float *norm0_w, *norm0_b, *norm1_w, *norm1_b;     /* (256) each        norms.{0,1} */
  const float *time_w, *time_b;                           /* (512,1024),(512)  time_mlp.1 ; may be NULL */
} ddp_layer_weights;

typedef struct ddp_weights {
  const float *transform_w, *transform_b; /* (256, Cx+Cm) 1x1 conv as matrix, (256): transform.conv / down.conv */
  const float *time_freq;                 /* (8)         time_mlp.0.weights */
  const float *time1_w, *time1_b;         /* (1024,17),(1024) time_mlp.1 */
  const float *time3_w, *time3_b;         /* (1024,1024),(1024) time_mlp.3 */
  const float *embedding;                 /* (K_cls+1,256) embedding_table.weight; NULL for depth */
  const float *head_w, *head_b;           /* seg/bev conv_seg (K_cls,256),(K_cls); bev with bev_seg_kernel = 3: (K_cls,256,3,3),(K_cls);
                                             depth conv_depth (1,256,3,3),(1), binned depth (n_bins,256,3,3),(n_bins) */
  ddp_layer_weights layers[DDP_MAX_LAYERS];
  const float* depth_bins;                /* (n_bins) bin centres of the binned depth head (the caller evaluates the reference's
                                             torch.linspace / torch.logspace); NULL otherwise */
} ddp_weights;

/* Host-computed per-step schedule scalars.  The cosine log-SNR is ill-conditioned at t = 1, so the
 * Python host layer evaluates the schedule with torch CPU fp32 ops in the reference's op order
 * (segmentors/ddp.py:22-28,225-231) and hands the scalars over; the library never re-derives them.
 *   seg/bev : time_in = log_snr(t_now); alpha, sigma, alpha_next, sigma_next as in ddp.py:229-231
 *   depth   : time_in = t_now; alpha = sqrt(gamma_now), sigma = 1/sqrt(1-gamma_now),
 *             alpha_next = sqrt(gamma_next), sigma_next = sqrt(1-gamma_next)  (depther/ddp.py:220-227)
 *   ddpm    : ddpm_c = -expm1(ls - ls_next), ddpm_std = exp(0.5*log(max(sigma_next^2*c,1e-20))),
 *             ddpm_add_noise = (t_next > 0)                                     (ddp.py:276-284) */
typedef struct ddp_step {
  float time_in, alpha, sigma, alpha_next, sigma_next, ddpm_c, ddpm_std;
  int32_t ddpm_add_noise;
} ddp_step;

const char* ddp_last_error(void);
int ddp_abi_version(void);

/* Size in bytes of the caller-provided workspace for `cfg` (constants + activations).
 * THE TAIL OF THE WORKSPACE: the buffers a caller reads or writes directly are the LAST of the workspace, in one fixed order.  Each
 * group exists only with its flag, each buffer is rounded up to 256 bytes (round256), and nothing follows the last one (the sizes
 * are the formulas of the sections named on the right):
 *   0. DDP_FLAG_SCORE_PRIOR: round256(rows_bytes), then round256(map_bytes)                                       "score prior"
 *   1. DDP_FLAG_CLASS_PRIOR    round256(bias_bytes), then round256(table_bytes)                                    "class prior"
 *   2. DDP_FLAG_PRIOR_START    [DDP_FLAG_SEEDED_NOISE clear: round256(start_bytes)], then round256(prior_bytes)    "prior start"
 *   3. DDP_FLAG_X0_HINTS       round256(row_bytes), then round256(hint_bytes)                                      "x0 hints"
 *   4. DDP_FLAG_SEEDED_NOISE   round256(noise_bytes)                                                               "Seeded noise"
 *   5. DDP_FLAG_STEP_RECORD    round256(record_bytes), then round256(map_bytes)                                    at ddp_x0_trace
 * A buffer starts at ddp_query_workspace(cfg) minus its own rounded size and the rounded sizes of everything behind it in this
 * list: the hint map of a cfg with flags 3, 4 and 5 at ddp_query_workspace(cfg) - round256(map_bytes) - round256(record_bytes)
 * - round256(noise_bytes) - round256(hint_bytes).  Setting one of the six flags grows ddp_query_workspace by exactly its group;
 * every offset in front of the group and ddp_query_const_workspace are those of the cfg without the flag.
 * ddp_sample_fcn_workspace ends with groups 4 and 5 in the same way (ddp_sample_fcn refuses flags 0 to 3).
 * ddp_amd.engine.caller_regions is this list on the host side. */
int ddp_query_workspace(const ddp_cfg* cfg, size_t* bytes);

/* Fill the constant region of the workspace: time embeddings and per-layer FiLM vectors for every
 * step (ddp.py:31-46,107-112; utils/transformer.py:275-278), sine positional tables folded through
 * the offset/attention projections (utils/transformer.py:78-113), the x0 look-up table
 * (ddp.py:236-237) and packed projection weights.  Must be re-run when weights, (h,w) or the
 * schedule change; `steps` is a HOST array of cfg->timesteps entries. */
int ddp_prepare(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_step* steps,
                void* d_workspace, void* stream);

/* Serving the reference's own test protocol - ONE image per call, a different (h, w) almost every call
 * (segmentation/tools/test.py:214-219 forces samples_per_gpu = 1; configs/_base_/datasets/ade20k.py:23 resizes keep-ratio):
 * the workspace starts with a MODEL region (everything ddp_prepare derives from the weights and the schedule: time
 * embeddings, FiLM, folded affines, x0 LUT and T = LUT.W_m^T, split weight planes, the layer kernels' weight streams) whose
 * size and content do not depend on batch / randsteps / (h, w) / (head_h, head_w) / the bev grid.  When only those change:
 *   - keep a buffer of at least ddp_query_workspace(new cfg) bytes whose first ddp_query_const_workspace(cfg) bytes are the
 *     prepared model region (same buffer, or a device-to-device copy of that prefix into a larger one),
 *   - call ddp_prepare_geometry(new cfg, ...) : L positional-table launches + one memset, no weight is touched.
 * Every other cfg field (task, sampler, timesteps, num_layers, num_classes, feat_channels, gemm_mode, flags, bit_scale, ...)
 * must be unchanged since ddp_prepare. */
int ddp_query_const_workspace(const ddp_cfg* cfg, size_t* bytes);
int ddp_prepare_geometry(const ddp_cfg* cfg, void* d_workspace, void* stream);

/* The whole K-step loop for B images: replaces DDP.ddim_sample / ddpm_sample / sample.
 *   d_x          (B, Cx, h, w)           frozen neck feature, NCHW
 *   d_noise      (B, r, Cm, h, w)        start noise (the reference draws torch.randn in-method)
 *   d_step_noise (K, B, r, Cm, h, w)     per-step noise, ddpm only, else NULL
 *   (DDP_FLAG_SEEDED_NOISE: d_noise is the 8-word device key and d_step_noise is ignored - "Seeded noise" below)
 *   d_out        seg: (B, K_cls, h, w); depth: (B, 1, h, w); bev: (B, K_cls, head_h, head_w) */
int ddp_sample(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_step* steps,
               const float* d_x, const float* d_noise, const float* d_step_noise, float* d_out,
               void* d_workspace, void* stream);

/* Diagnostic trace (seg, cfg->flags & DDP_FLAG_RECORD_X0): after ddp_sample, *d_idx points at (K, B*r*h*w) uint8 inside
 * the workspace - the x0 class (argmax of the step's scores, ddp.py:235) every step fed back.  The loop's only
 * discontinuity is this discrete choice; with it recorded, parity splits into "same decisions -> outputs agree to
 * rounding" and "decisions differ only where the reference's own top-2 gap is at rounding level"
 * (tests/test_full_size_parity.py).
 * With DDP_FLAG_FORCE_X0 the buffer is (2, K, B*r*h*w): [0] = the decisions to feed back, written by the caller BEFORE
 * ddp_sample (values < num_classes); [1] = the argmax the engine itself found at every step under that forcing.  The library
 * cannot tell whether [0] was filled: a caller that sets DDP_FLAG_FORCE_X0 and does not write it feeds back whatever the
 * workspace held (values >= num_classes are read as class 0) - ddp_amd.engine.DDPEngine refuses to sample until
 * set_x0_decisions() ran.  Both flags are rejected (DDP_E_BADCFG) for tasks other than DDP_TASK_SEG.
 * The workspace LAYOUT (which bytes hold what, incl. this buffer's place) is an implementation detail of one build: it is
 * queried, never assumed, and may change between library builds of the same DDP_ABI_VERSION. */
/* DDP_FLAG_STEP_RECORD (any task): *d_idx is the base of the STEP RECORD instead, and no other flag is needed.  After ddp_sample
 * the record holds one slice per step s, (K, B, r, H, W) with (H, W) = (head_h, head_w) (== (h, w) for seg and depth); the element
 * type behind the `unsigned char*` depends on the task:
 *   seg   uint8   the argmax class of the step's scores per replica - the value ddp.py:235 feeds back, i.e. the DDP_FLAG_RECORD_X0
 *                 trace (with both flags set ONE buffer is carved and both describe it)
 *   depth float   the head's metric prediction of the step (`depth_pred`, depther/ddp.py:239), before normalisation and before the
 *                 clamp of encode_decode
 *   bev   uint32  bit c = (prob_c > threshold) at the head-grid pixel (fusion_models/ddp.py:290), before the nearest resize
 * Sizes, as formulas of the cfg:
 *   record_bytes = timesteps * batch * randsteps * head_h * head_w * (seg: 1, depth / bev: 4)
 *   map_bytes    = batch * head_h * head_w * 4
 * Both are carved at the END of the workspace (group 5 of the list at ddp_query_workspace), each rounded up to 256 bytes.
 * The STEP-DISAGREEMENT MAP, (B, H, W) float, starts at *d_idx + round256(record_bytes) and is written once per
 * ddp_sample by k_step_disagreement, after the output (same stream, hipGraph-capturable like the rest):
 *   seg   the fraction of the K * r recorded decisions of the pixel that differ from its final decision = argmax over the classes
 *         of the output ddp_sample returned (first maximum wins, as ddp_seg_postprocess)
 *   bev   the mean over the K * r records and the K_cls classes of [bit_c != (out_c > threshold)], out = the returned mean probability
 *   depth the standard deviation of the K * r recorded predictions (two passes in fp32, population form)
 * K * r = 1 gives zeros.  ddp_sample_fcn honours the flag the same way (seg record and map); ddp_x0_trace does not know that
 * loop's layout: there the two buffers are the last of ITS workspace, the record at
 * ddp_sample_fcn_workspace(cfg) - round256(map_bytes) - round256(record_bytes), the map behind it as above.
 * Extra launches with the flag set: one k_step_disagreement per call; bev + one k_bev_record per step; depth + one head-only
 * k_depth_update per step whose update runs fused inside the next step's head (the fused step boundary); seg none. */
int ddp_x0_trace(const ddp_cfg* cfg, void* d_workspace, const unsigned char** d_idx);

/* Seeded noise (DDP_FLAG_SEEDED_NOISE, any task; csrc/ddp_noise.hip).  With the flag set, ddp_sample / ddp_sample_fcn read
 *   d_noise       a DEVICE array of 8 uint32 words {seed_lo, seed_hi, image_base, stream_base, call, 0, 0, 0}, 16-byte aligned.  The
 *                 kernels read the words from device memory when they run, so a captured graph picks up a new key without being
 *                 captured again.  Words 5..7 are reserved: the kernels ignore them, the caller writes zeros
 *   d_step_noise  ignored, may be NULL
 * and generate every value with Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments
 * 0x9E3779B9 / 0xBB67AE85):
 *   key     = (seed_lo, seed_hi)
 *   counter = (e >> 2, image_base + b, stream, call), e = the flat index of the element inside image b's (r, Cm, h, w) block;
 *             the element's value is output lane e & 3 of that counter
 *   stream  = stream_base for the start noise, stream_base + 1 + s for the noise added after step s (ddpm, ddpm_add_noise != 0;
 *             other steps generate nothing)
 *   normals = Box-Muller on u = ((x >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1)): rad = sqrtf(-2 logf(u0)),
 *             lanes (0, 1) = rad * (cospi(2 u1), sinpi(2 u1)) from words (0, 1), lanes (2, 3) the same from words (2, 3)
 * A value is thus a function of (seed, image, stream, call, e) only - not of batch, of the position in the batch, of the layout
 * it is written in or of the grid that wrote it: image i of a batch whose image_base is a equals a one-image call with
 * image_base = a + i.  The start noise is written NCHW by k_noise_fill_nchw into a workspace buffer that every consumer reads in
 * place of the caller's tensor; a ddpm step's noise is written token-major by k_noise_fill_tok straight into the buffer the update
 * kernel reads (no (K, B, r, Cm, h, w) tensor, no per-step transpose).  Size and place, as formulas of the cfg:
 *   noise_bytes = batch * randsteps * Cm * h * w * 4      (Cm = 1 for depth, else 256)
 * carved IMMEDIATELY IN FRONT of the step-record buffers - at the END of the workspace when DDP_FLAG_STEP_RECORD is clear - (group 4
 * of the list at ddp_query_workspace; ddp_sample_fcn_workspace follows the same rule).  The buffer holds the (B, r, Cm, h, w) start
 * noise of the LAST call until the next one.
 * Extra launches with the flag set: one k_noise_fill_nchw per call; per noise-adding ddpm step one k_noise_fill_tok in place of the
 * NCHW -> token-major transpose. */

/* x0 hints (DDP_FLAG_X0_HINTS, seg and depth; csrc/ddp_hints.hip).  The replacement form of conditioning: the loop's only feedback
 * into the next step is the x0 projection (segmentors/ddp.py:235-239, depther/ddp.py:240-246), and at the pixels where the caller
 * knows the answer that answer is projected instead of the model's prediction.  The HINT MAP is per image at the map resolution,
 * (B, h, w); all r replicas and all K steps share it:
 *   seg    uint8.  A value < num_classes is fed back as the class in place of the argmax (ddp.py:235); any value >= num_classes
 *          (255 by convention) leaves the pixel free.  num_classes <= 255 (256 classes are refused: no free value would be left)
 *   depth  float32 metric depth.  A finite value > 0 replaces depth_pred in the x0 normalisation only (depther/ddp.py:240-241, with
 *          the clamp of :224 - a hint outside [min_depth, max_depth] clamps like a prediction would); 0, a negative value, NaN or
 *          +-inf leaves the pixel free
 * What ddp_sample returns stays the model's own prediction (scores / depth), and the step record (DDP_FLAG_STEP_RECORD,
 * DDP_FLAG_RECORD_X0) keeps the model's own decision of every step: a caller sees where the model disagrees with its hints.  Hints
 * act through the update, i.e. from the SECOND step on: timesteps = 1 is accepted and the hints have no effect there.
 * Sizes, as formulas of the cfg - two buffers, group 3 of the list at ddp_query_workspace, which gives their place:
 *   hint_bytes = batch * h * w * (seg: 1, depth: 4)              the caller-written hint map
 *   row_bytes  = batch * randsteps * h * w * (seg: 1, depth: 4)  library-private, immediately in front of the hint map: the hints per
 *                row m = (b * r + rr) * N + n (the order of the x0 trace) with the "free" encodings normalised (seg 255, depth 0)
 * The library never initialises the hint map: the caller writes it (all free = every byte 255 / every float 0) before the first
 * ddp_sample; ddp_amd.engine.DDPEngine does so whenever it allocates the workspace or changes the geometry.  The kernels read the
 * caller's buffer from device memory when they run, so a captured graph picks up new hints without being captured again.
 * Extra launches with the flag set: one k_hint_rows_seg / k_hint_rows_depth per call, first.  seg runs the teacher-forcing
 * instantiations of its decision kernels (the ones DDP_FLAG_FORCE_X0 runs, which have no non-temporal variant) with the row buffer
 * as the forced class and "keep the argmax where the forced value is >= num_classes" semantics; depth the same kernels as without
 * the flag, which read one more float per pixel and step. */

/* prior start (DDP_FLAG_PRIOR_START, all three tasks; csrc/ddp_prior_start.hip).  forward_train noises a known map to a time t and asks
 * the head to recover it (segmentors/ddp.py:149-165, depther/ddp.py:133-143, the bev model likewise); with the flag set the same
 * arithmetic starts the sampling chain: the loop's first read comes from the caller's PRIOR MAP noised to steps[0], and a caller who
 * holds a good estimate (the previous frame, the coarse scale, an edited map) runs fewer steps from a smaller time.  The library
 * takes alpha and sigma from steps[0] as passed to ddp_sample; the host layer evaluates the whole steps array on a time grid that
 * begins at t_start instead of 1 (ddp_amd.schedule, t_start=).  The steps are independent of the flag: a flag-clear call with such a
 * steps array and a caller-made start map in d_noise is legal.
 * The prior map is per image at the map resolution, (B, h, w); all r replicas share it, each keeps its own noise:
 *   seg    uint8.  A value < num_classes is that class; any other value is the ignore row embedding[num_classes] (ddp.py:151).  With
 *          256 classes every value is a class
 *   depth  float32 metric depth.  Finite and > 0: x0 = clamp(((d - min_depth) / (max_depth - min_depth) * 2 - 1) * bit_scale,
 *          +-bit_scale) with the depther's range, clamped like a prediction; anything else (0, negative, NaN, +-inf): x0 = 0, the
 *          middle of the range
 *   bev    uint32.  Bit c set = class c present, bits >= num_classes are ignored:
 *          x0 = (sigmoid(mean_c embedding[bit_c ? c + 1 : 0]) * 2 - 1) * bit_scale (fusion_models/ddp.py)
 * Start map, for image b, replica rr, channel ch, pixel n, eps = the caller's d_noise or the seeded start noise:
 *   seg / bev   m0 = steps[0].alpha * x0[b][ch][n] + steps[0].sigma * eps[b][rr][ch][n]
 *   depth       m0 = steps[0].alpha * x0[b][n]     + eps[b][rr][0][n] / steps[0].sigma     (depth's ddp_step.sigma is 1 / sqrt(1 - gamma))
 * each as ONE fused multiply-add on the rounded second term.  Every route then reads m0 where it would read d_noise.
 * Sizes, as formulas of the cfg - group 2 of the list at ddp_query_workspace, which gives their place:
 *   prior_bytes = batch * h * w * (seg: 1, depth / bev: 4)        the caller-written prior map
 *   start_bytes = batch * randsteps * Cm * h * w * 4              the start map m0 (B, r, Cm, h, w), immediately in front of the prior
 *                 map; carved only when DDP_FLAG_SEEDED_NOISE is clear.  With both flags set the seeded-noise buffer is the start
 *                 buffer: it is filled with eps and then mixed in place, and after the call it holds m0, not eps
 * The library never initialises the prior map: the caller writes it before ddp_sample (ddp_amd.engine.DDPEngine clears it - seg
 * 255, depth 0, bev 0 - whenever it allocates the workspace or changes the geometry).  The kernel reads it from device memory when it
 * runs, so a captured graph picks up a new prior on replay.
 * Extra launches with the flag set: one k_prior_start_tab (seg, bev) / k_prior_start_depth per call, behind the hint-row launch and the noise fill. */

/* class prior (DDP_FLAG_CLASS_PRIOR, seg; csrc/ddp_class_prior.hip).  Image-level knowledge about the answer: which classes can
 * occur in image b and how likely each is (a tagger's candidate list, logit adjustment log p_target / p_train, classes a user
 * switched off).  The CLASS PRIOR TABLE is (B, 256) float32; row b, entry k < num_classes is added to the conv_seg score of class k
 * at every token of image b, for all r replicas and all K steps, in front of everything that reads the score: the argmax fed back
 * as x0 (segmentors/ddp.py:235-239), the accumulated softmax, the returned last-step scores, the step record and the
 * DDP_FLAG_RECORD_X0 trace.  The call computes what B one-image calls with conv_seg.bias + prior[b] would compute.  Entries
 * k >= num_classes are ignored.  With DDP_FLAG_FORCE_X0 the forced decision is fed back and the returned scores carry the prior.
 * One launch per call (k_class_prior, behind the hint-row launch) normalises the table as read THEN - NaN reads as 0, every value is
 * clamped to [-1e30, 1e30] - so -inf (anything <= -1e30) means "class excluded": its score stays finite, its softmax term is
 * exactly 0 and the returned scores never hold an infinity (the bilinear epilogues would turn 0 * inf into NaN).  An image with
 * every class excluded is a uniform shift.
 * Sizes, as formulas of the cfg - two buffers, group 1 of the list at ddp_query_workspace, which gives their place:
 *   table_bytes = batch * 256 * 4       the caller-written table
 *   bias_bytes  = 2 * batch * 256 * 4   library-private, immediately in front of the table: per image the vector
 *                 fl32(conv_seg.bias + clamp(prior[b])), zero padded to 256 (the accumulator start of conv_seg in the layer
 *                 kernel's seg tails, which a lane reads for the image of its token, m / (r N) - a 32-token tile may straddle two
 *                 images), then per image clamp(prior[b]) (added to the head GEMM's scores by k_seg_update on the routes that run
 *                 conv_seg as a tile GEMM: the fp32 engine, DDP_FLAG_UNFUSED_LAYER, ddpm without DDP_FLAG_DDPM_CHAIN)
 * The library never initialises the table: the caller writes it (all zeros = no prior, the bits of the flag-clear call) before the
 * first ddp_sample; ddp_amd.engine.DDPEngine does so whenever it allocates the workspace or changes the geometry.  The kernel
 * reads the caller's table from device memory when it runs, so a captured graph picks up a new table on replay.
 * Extra launches with the flag set: one k_class_prior per call.  The layer kernel's seg tails run their conditioned instantiations
 * (the ones DDP_FLAG_FORCE_X0 and DDP_FLAG_X0_HINTS run, which have no non-temporal variant); the flag-clear instantiations are
 * untouched. */

/* score prior (DDP_FLAG_SCORE_PRIOR, seg; csrc/ddp_score_prior.hip).  Soft knowledge about the answer that varies over the image:
 * the logits of a cheaper model, last frame's scores warped to this frame, a scribble with a strength, a region where some classes
 * cannot occur.  The SCORE PRIOR MAP is (B, num_classes, h, w) float32 at the map resolution, NCHW - the layout of d_out; entry
 * [b][k][n] is added to the conv_seg score of class k at pixel n of image b, for all r replicas and all K steps, in front of
 * everything that reads the score: the argmax fed back as x0 (segmentors/ddp.py:235-239), the accumulated softmax, the returned
 * last-step scores, the step record and the DDP_FLAG_RECORD_X0 trace.  The call computes what the reference's sampler computes when
 * its decode head returns scores + prior[b].  One launch per call (k_score_prior_rows, behind k_class_prior) normalises the map as
 * read THEN by the class prior's rule - NaN reads as 0, every value is clamped to [-1e30, 1e30] - so -inf excludes a class at that
 * pixel: its score stays finite, its softmax term is exactly 0 and no infinity reaches the bilinear epilogues.
 * Combination rules: with DDP_FLAG_CLASS_PRIOR both priors add (the image's row first, then the pixel's); with DDP_FLAG_FORCE_X0 /
 * DDP_FLAG_X0_HINTS the forced or hinted decision is fed back and the returned scores carry the prior; an all-zero map gives the bits
 * of the flag-clear call; a map that is constant over the pixels of each image gives the bits of DDP_FLAG_CLASS_PRIOR with that row,
 * on every route.
 * Sizes and places, as formulas of the cfg - two buffers, each rounded up to 256 bytes, group 0 of the list at ddp_query_workspace;
 * ddp_query_workspace grows by exactly round256(rows_bytes) + round256(map_bytes), every other offset and
 * ddp_query_const_workspace are those of the cfg without the flag:
 *   map_bytes  = batch * num_classes * h * w * 4   the caller-written map, carved IMMEDIATELY IN FRONT of the class-prior buffers (of
 *                the prior-start, x0-hint, seeded-noise, step-record buffers - whichever come first - or the end of the workspace)
 *   rows_bytes = batch * h * w * KP * 4, KP = 64 * ceil(num_classes / 64)   library-private, immediately in front of the map: the
 *                normalised prior token-major, row b * N + n (N = h * w), zero in columns >= num_classes.  A lane of the layer
 *                kernel's seg tails adds the row of its token's pixel, (m / (r N)) * N + m % N, to the accumulator start of
 *                conv_seg (lg = fl32(start + p), the start being the class-prior row or conv_seg.bias); k_seg_update adds the same
 *                row to the head GEMM's scores and writes the sums back on the routes that run conv_seg as a tile GEMM (the fp32
 *                engine, DDP_FLAG_UNFUSED_LAYER, ddpm without DDP_FLAG_DDPM_CHAIN)
 * The library never initialises the map: the caller writes it (all zeros = no prior) before the first ddp_sample;
 * ddp_amd.engine.DDPEngine does so whenever it allocates the workspace or changes the geometry.  The kernel reads the caller's map
 * from device memory when it runs, so a captured graph picks up a new map on replay.
 * Extra launches with the flag set: one k_score_prior_rows per call.  The layer kernel's seg tails run their conditioned
 * instantiations (the ones DDP_FLAG_FORCE_X0, DDP_FLAG_X0_HINTS and DDP_FLAG_CLASS_PRIOR run, which have no non-temporal variant) and
 * read KP * 4 bytes more per token and step; the flag-clear instantiations are untouched. */

/* ---- finer-grained entry points (unit tests, and the decode_head plugin surface) ------------- */

/* DeformableHeadWithTime.forward: feat (R,256,hh,wh) NCHW + time embedding (1024) -> head output
 * seg: logits (R,K_cls,hh,wh); depth: metric depth (R,1,hh,wh); bev: sigmoid maps.  Uses step slot 0
 * of the workspace constants for FiLM, recomputed from d_temb.  R = batch*randsteps.  bev: cfg->bev_prescale and
 * cfg->bev_seg_kernel are honoured as in ddp_sample. */
int ddp_head_forward(const ddp_cfg* cfg, const ddp_weights* weights, const float* d_feat,
                     const float* d_temb, float* d_out, void* d_workspace, void* stream);

/* One deformable attention core (mmcv ms_deform_attn_forward for 1 level):
 *   d_value (R, N, 256) token-major; d_samp (R*N, 96): per token 64 pixel-unit sample coordinates
 *   [head][point][x,y] followed by 32 softmaxed weights [head][point]; d_out (R*N, 256). */
int ddp_msda_forward(const float* d_value, const float* d_samp, float* d_out, int rows, int h, int w,
                     void* stream);

/* The same core computed by the kernel the SAMPLING LOOP runs (k_msda_gather_lds: one head per block, the head's 128-B
 * slices of a window of the zero-padded value map staged in LDS, taps outside the window served from global memory), behind
 * the same plain interface: the entry pads the map, transposes the table to head-major, launches the loop's gather exactly
 * as ddp_sample does and converts its split-bf16 output back to fp32 rows (exact).  d_guess: (8,2) per-head (x, y) guess of
 * the mean sampling offset that positions the LDS window before the table is read (the loop derives it from the offset bias
 * and the positional tables), or NULL = zero guess; results do not depend on it (it only decides which taps hit LDS).
 * This is the entry the adversarial tests use: on-pixel, far-outside, NaN and border-straddling sample points. */
int ddp_msda_forward_lds_workspace(int rows, int h, int w, size_t* bytes);
int ddp_msda_forward_lds(const float* d_value, const float* d_samp, const float* d_guess, float* d_out, int rows, int h, int w,
                         void* d_workspace, void* stream);

/* out[M][N] = A[M][K] * W[N][K]^T + bias  (fp32 MFMA), optional exact GELU. K % 32 == 0. */
int ddp_linear(const float* d_a, const float* d_w, const float* d_bias, float* d_out, int m, int n, int k,
               int gelu, void* stream);

/* The same contraction in the arithmetic of the DEFAULT engine (DDP_GEMM_BF16X3, csrc/gemm_bf16x3.h): A and W are split
 * exactly into three bf16 pieces each and the six significant cross products run on the bf16 matrix cores with fp32
 * accumulation.  Exposed so that the accuracy claim above is a unit test (tests/test_b3_arithmetic.py: error against
 * fp64 <= c * 2^-24 * sum_k |a||w| on normal-range, wide-dynamic-range, cancelling and near-subnormal operands), not a
 * comment.  out[M][N] = A[M][K] * W[N][K]^T + bias; K % 32 == 0, N % 4 == 0; d_workspace from ddp_linear_b3_workspace. */
int ddp_linear_b3_workspace(int m, int n, int k, size_t* bytes);
int ddp_linear_b3(const float* d_a, const float* d_w, const float* d_bias, float* d_out, int m, int n, int k,
                  void* d_workspace, void* stream);

/* time_mlp + per-layer FiLM on device: d_temb (S,1024), d_film (S,L,512) for S time inputs. */
int ddp_time_embed(const ddp_weights* weights, int num_layers, const float* time_in_host, int s,
                   float* d_temb, float* d_film, float* d_scratch /* >= S*(17+1024) floats */, void* stream);

/* DDIM x0-projection + update for seg on token-major buffers (ddp.py:235-239):
 *   d_logits (M, ld_logits), d_lut (K_cls+1... rows of 256), d_mask (M,256) updated in place. */
int ddp_ddim_update_seg(const float* d_logits, int ld_logits, int num_classes, const float* d_lut,
                        float* d_mask, int rows, const ddp_step* step, void* stream);

/* x0 projection alone (segmentors/ddp.py:235-237), NCHW: d_x0 (B,256,h,w) = (sigmoid(embedding[argmax_k d_scores]) * 2 - 1) *
 * bit_scale for d_scores (B,K,h,w).  With the scores of ONE decoder pass at t = 1 this is the self-aligned pre-pass of
 * SelfAlignedDDP (segmentors/self_aligned_ddp.py:150-164: t = 1 head forward -> argmax -> embedding -> bit scaling). */
int ddp_seg_x0_project(const float* d_scores, int batch, int num_classes, int n_pix, const float* d_embedding,
                       float bit_scale, float* d_x0, void* stream);

/* Post-loop epilogue of the segmentor, fused: replaces
 *   resize(out, img.shape[2:]) (segmentors/ddp.py:124-128), whole_inference's crop to img_shape + resize to
 *   ori_shape (encoder_decoder.py:236-248), softmax (:277), flip (:278-285) and argmax (:296).
 * d_scores (B,K,h,w) = ddp_sample's output; image (img_h,img_w) = padded network input; crop = img_shape;
 * out = ori_shape (== crop: no second resize); flip: 0 none, 1 horizontal, 2 vertical.
 * d_seg (B,out_h,out_w) uint8 class indices (first maximum wins).  K <= 256. */
int ddp_seg_postprocess(const float* d_scores, int batch, int num_classes, int h, int w, int img_h, int img_w,
                        int crop_h, int crop_w, int out_h, int out_w, int align_corners, int flip,
                        unsigned char* d_seg, void* stream);

/* Multi-scale / flip test-time augmentation epilogue, fused (encoder_decoder.py:306-331 `aug_test` over :251-287 `inference`
 * over :229-248 `whole_inference` over segmentors/ddp.py:124-128): for every augmentation a
 *   resize of its low-resolution scores to its network input -> crop to img_shape -> resize to ori_shape -> softmax ->
 *   flip undone,
 * then the mean over the augmentations and argmax.  One thread per output pixel walks all augmentations: neither the per-
 * augmentation (B,K,H,W) tensors nor the (B,K,ori_h,ori_w) running sum of the reference are materialised.
 * d_seg (B,out_h,out_w) uint8; d_prob optional (B,K,out_h,out_w) mean probabilities (tests / callers that need them). */
#define DDP_MAX_AUGS 16
typedef struct ddp_seg_aug {
  const float* d_scores;   /* (B,K,h,w): ddp_sample's output for this augmentation */
  int32_t h, w;            /* its map size */
  int32_t img_h, img_w;    /* its (padded) network input */
  int32_t crop_h, crop_w;  /* its img_shape */
  int32_t flip;            /* 0 none, 1 horizontal, 2 vertical: undone on the probabilities */
} ddp_seg_aug;
int ddp_seg_aug_postprocess(const ddp_seg_aug* augs, int n_aug, int batch, int num_classes, int out_h, int out_w,
                            int align_corners, unsigned char* d_seg, float* d_prob, void* stream);

/* Sliding-window inference epilogue, fused (encoder_decoder.py:180-227 `slide_inference` over segmentors/ddp.py:114-129
 * `encode_decode`, then :266-296 `inference` / `simple_test`): the image is covered by a grid of n_rows x n_cols windows of
 * crop_h x crop_w pixels (top-left corners win_y1[i], win_x1[j]: the reference's y1 / x1 after clamping to the image); every
 * window went through the K-step loop on its own and left low-resolution scores (B,K,h,w).  Per output pixel this kernel does
 * what the reference does with full-size tensors: resize each covering window's scores to the window size, sum them in window
 * order (row-major), divide by the number of covering windows, crop to (keep_h, keep_w) = img_shape, resize to (out_h, out_w) =
 * ori_shape, [softmax,] undo the flip, argmax.  Neither the per-window (B,K,crop_h,crop_w) logits nor `preds` / `count_mat` at
 * image size exist.  A pixel may be covered by at most 4 window rows and 4 window columns (stride >= crop / 4).
 * d_scores[i * n_cols + j] (B,K,h,w); d_seg (B,out_h,out_w) uint8 or NULL; d_prob optional (B,K,out_h,out_w):
 * prob_mode 1 = softmax probabilities (`inference`), 2 = the averaged scores themselves (`slide_inference`'s return value). */
#define DDP_MAX_WINDOWS 64
int ddp_seg_slide_postprocess(const float* const* d_scores, const int* win_y1, const int* win_x1, int n_rows, int n_cols, int batch,
                              int num_classes, int h, int w, int crop_h, int crop_w, int img_h, int img_w, int keep_h, int keep_w,
                              int out_h, int out_w, int align_corners, int flip, int prob_mode, unsigned char* d_seg, float* d_prob,
                              void* stream);

/* Post-loop epilogue of the depth toolbox, fused (depth/depth/models/depther/ddp.py:95-109 `encode_decode`: clamp to
 * [min_depth, max_depth], bilinear resize to the network input; encoder_decoder.py:187-194 `inference`: flip undone;
 * :198-209 `simple_test`; :210-229 `aug_test`: running sum over the augmentations in list order, / n).  One thread per 4
 * output pixels walks all augmentations: neither the per-augmentation (B,1,H,W) maps nor the running sum are materialised.
 * With n_aug == 1 this is `simple_test` / `inference` / `encode_decode(rescale=True)` (x / 1 is exact); out == map size:
 * no resize (`rescale=False`).  d_out (B,1,out_h,out_w) fp32. */
typedef struct ddp_depth_aug {
  const float* d_depth;    /* (B,1,h,w): ddp_sample's output (task depth) for this augmentation */
  int32_t h, w;            /* its map size */
  int32_t flip;            /* 0 none, 1 horizontal, 2 vertical: undone on the resized map */
} ddp_depth_aug;
int ddp_depth_postprocess(const ddp_depth_aug* augs, int n_aug, int batch, int out_h, int out_w, int align_corners,
                          float min_depth, float max_depth, float* d_out, void* stream);

/* MultiStageMerging neck (necks/multi_stage_merging.py:40-52): the step that produces the frozen
 * feature x of the sampling loop from the four FPN levels: bilinear resize of every level to level 0's grid, concat
 * (1024 ch), down = ConvModule(1024, 256, 1, bias=False, GroupNorm(32), no activation).
 * d_levels[l] (B,256,h_l,w_l) NCHW; d_conv_w = neck.down.conv.weight (256,1024,1,1); d_gn_w/d_gn_b = neck.down.gn.*;
 * d_out (B,256,h_0,w_0) NCHW.  Workspace from ddp_neck_msm_workspace (caller-owned). */
int ddp_neck_msm_workspace(int batch, const int* level_h, const int* level_w, size_t* bytes);
/* flags of the two neck entries: the workspace starts with a weight region (split weight planes as the stage images of the
 * stream GEMM) whose layout depends on the channel counts only; a caller that runs the same weights again through the same
 * workspace buffer - on the same stream, or after synchronising with the call that packed them - passes
 * DDP_NECK_WEIGHTS_READY and the weights are not re-packed. */
#define DDP_NECK_WEIGHTS_READY 1
int ddp_neck_msm(const float* const* d_levels, const int* level_h, const int* level_w, int batch,
                 const float* d_conv_w, const float* d_gn_w, const float* d_gn_b, int align_corners, int flags, float* d_out,
                 void* d_workspace, void* stream);

/* FPN neck (necks/fpn.py:163-213) as the DDP configs build it: 4 levels, lateral ConvModule(C_l,256,1,
 * bias=False, GN(32), no act), top-down nearest upsample + add, output ConvModule(256,256,3,padding=1,bias=False,GN(32),
 * no act); num_outs = 4 (no extra levels).  d_in[l] (B,C_l,h_l,w_l) NCHW, C_l % 32 == 0, 64 <= C_l <= 4096; d_out[l]
 * (B,256,h_l,w_l) NCHW. */
typedef struct ddp_fpn_level {
  const float* lat_w;      /* lateral_convs.l.conv.weight (256,C_l,1,1) */
  const float* lat_gn_w;   /* lateral_convs.l.gn.weight / bias (256) */
  const float* lat_gn_b;
  const float* out_w;      /* fpn_convs.l.conv.weight (256,256,3,3) */
  const float* out_gn_w;   /* fpn_convs.l.gn.weight / bias (256) */
  const float* out_gn_b;
  int in_channels, h, w;
} ddp_fpn_level;
int ddp_neck_fpn_workspace(const ddp_fpn_level* levels, int batch, size_t* bytes);
int ddp_neck_fpn(const ddp_fpn_level* levels, int batch, const float* const* d_in, float* const* d_out, int flags,
                 void* d_workspace, void* stream);

/* FPN followed by MultiStageMerging - the neck list of every DDP config (configs/ade/ddp_swin_t_2x8_512x512_160k_ade20k.py: neck =
 * [FPN, MultiStageMerging]; the segmentor uses only the merged map): the four FPN outputs stay in the GEMM operand layout and
 * feed the merging directly; their NCHW form is never produced.  d_in[l] as ddp_neck_fpn, the three MSM parameters as
 * ddp_neck_msm, d_out (B,256,h_0,w_0) NCHW. */
int ddp_neck_fpn_msm_workspace(const ddp_fpn_level* levels, int batch, size_t* bytes);
int ddp_neck_fpn_msm(const ddp_fpn_level* levels, int batch, const float* const* d_in, const float* d_msm_conv_w,
                     const float* d_msm_gn_w, const float* d_msm_gn_b, int align_corners, int flags, float* d_out,
                     void* d_workspace, void* stream);

/* FCNHeadWithTime.forward (decode_heads/fcn_head_with_time.py:285-305), eval mode:
 *   x = inputs[0]; for each ConvWithTimeModule: x = ReLU( norm(conv3x3(x)) * (scale + 1) + shift ),
 *   (scale, shift) = Linear(SiLU(temb)).chunk(2)  (:205-225);  out = conv_seg(x)  (cls_seg, dropout is identity in eval).
 * 256 channels in and out; per conv the norm is an eval-mode BatchNorm (running statistics), a GroupNorm(32, 256) or absent - a
 * head may mix them.  The reference's conv_cat is constructed but never called by _forward_feature (:285-299) and is
 * therefore not part of the path.
 * The norm of a conv is told by its four bn_* pointers:
 *   all four set                          eval-mode BatchNorm, eps = bn_eps (folded with the FiLM into the weights and the bias)
 *   bn_w, bn_b set, bn_mean = bn_var = NULL
 *                                         GroupNorm(32 groups of 8 channels), gamma = bn_w, beta = bn_b, eps = bn_eps; the
 *                                         statistics are taken per map m = b * r + rr on its own, over the conv output with its
 *                                         bias:  y = ReLU( (conv(x) + conv_b - mu[m,g]) * rstd[m,g] * gamma * (scale + 1)
 *                                                          + beta * (scale + 1) + shift )
 *   bn_w NULL                             no norm
 *   anything else (bn_b missing, only one of bn_mean / bn_var)    DDP_E_NULL, "incomplete norm"
 * The scratch of a GroupNorm conv lies inside the bytes ddp_fcn_head_workspace / ddp_sample_fcn_workspace return for any head. */
typedef struct ddp_fcn_conv {
  const float* conv_w;   /* convs.i.conv.weight (256,256,3,3) */
  const float* conv_b;   /* convs.i.conv.bias (256) or NULL (bias='auto' with a norm) */
  const float* bn_w;     /* convs.i.bn.weight / bias / running_mean / running_var (256 each), or all NULL; GroupNorm:
                          * convs.i.gn.weight / bias with bn_mean = bn_var = NULL (see above) */
  const float* bn_b;
  const float* bn_mean;
  const float* bn_var;
  float bn_eps;
  const float* time_w;   /* convs.i.time_mlp.1.weight (512,1024) */
  const float* time_b;   /* convs.i.time_mlp.1.bias (512) */
} ddp_fcn_conv;
int ddp_fcn_head_workspace(int maps, int h, int w, int num_classes, size_t* bytes);
int ddp_fcn_head_forward(const ddp_fcn_conv* convs, int num_convs, int dilation, const float* d_cls_w, const float* d_cls_b,
                         int num_classes, const float* d_feat /* (maps,256,h,w) */, const float* d_temb /* (1024) or NULL */,
                         int maps, int h, int w, float* d_out /* (maps,num_classes,h,w) */, void* d_workspace, void* stream);

/* The K-step sampler with FCNHeadWithTime as the decode head: what `DDP.ddim_sample` / `ddpm_sample`
 * (segmentors/ddp.py:215-290) compute when `_decode_head_forward_test` (:192-196) dispatches to
 * `FCNHeadWithTime.forward_test` (decode_heads/fcn_head_with_time.py:327-343).  Same inputs, outputs, schedule scalars and
 * x0 projection / update / accumulation as ddp_sample; cfg->task must be DDP_TASK_SEG, cfg->num_layers is ignored;
 * `weights` supplies transform, time_mlp, embedding and conv_seg (head_w / head_b), `convs` the head's ConvWithTimeModules. */
int ddp_sample_fcn_workspace(const ddp_cfg* cfg, int num_convs, int dilation, size_t* bytes);
/* Everything of that loop that depends on weights and schedule only - the time embeddings of the K steps, the x0 table, the
 * split column blocks of the concat-conv and, per (step, conv), the FiLM vector (fcn_head_with_time.py:216-221), the folded
 * norm x FiLM affine and the 72 stage images of the scaled 3x3 weights (the FiLM scale is folded INTO the weights, so every
 * step has its own images), plus conv_seg's images - written once into the model region of the workspace.  A caller that
 * samples repeatedly through the same workspace buffer (same stream, or after synchronising with this call) passes
 * DDP_FLAG_FCN_PREPARED in cfg->flags to ddp_sample_fcn and none of these ~12 kernels per (step, conv) runs again; without
 * the flag ddp_sample_fcn calls this itself.
 * A GroupNorm conv has ONE set of images, of its plain weights, for all steps (slot (step 0, conv i); its other slots stay
 * unused) and its bias vector; nothing of it is rebuilt under DDP_FLAG_FCN_PREPARED either.  Its FiLM vector (512 floats; the
 * prepared region holds 256 per (step, conv)) is evaluated inside the loop, one matvec per (step, conv), from convs[i].time_w /
 * time_b, and the apply pass reads convs[i].bn_w / bn_b: those four tensors must stay valid during ddp_sample_fcn. */
int ddp_prepare_fcn(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, int dilation,
                    const ddp_step* steps, void* d_workspace, void* stream);
int ddp_sample_fcn(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, int dilation,
                   const ddp_step* steps, const float* d_x, const float* d_noise, const float* d_step_noise, float* d_out,
                   void* d_workspace, void* stream);

/* Measurement hook (bench.py roofline leg; not part of the reference surface, NOT thread-safe: one process-wide session;
 * two threads sampling with a session armed would interleave their records): arm HIP-event timing
 * around every launch of one GEMM call site, then read the summed duration and launch count.
 * tag: 1 xproj, 2 feat / step prologue, 3 value_proj, 4 sampling proj, 5 output_proj+LN, 6 FFN fc1, 7 FFN fc2+LN / the
 * layer kernel, 8 head conv / seg tail, 9 deformable gather, 10 last layer of a step + seg tail (one kernel); 255 = all of
 * them at once.  ddp_profile_end synchronises on
 * the recorded events and returns the sum over all records; ddp_profile_read then gives one call site's share
 * (DDP_E_BADCFG for an unknown tag or when no finished session exists). */
int ddp_profile_begin(int tag);
int ddp_profile_end(float* total_ms, int* launches);
int ddp_profile_read(int tag, float* total_ms, int* launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_MI355X_H */
