// ddp_api.hip - C-ABI entry points of libddp_mi355x.so and the K-step loop orchestration.
//
// One stream, no host synchronisation, no allocation: the caller hands over a workspace which is
// carved deterministically from `ddp_cfg` (constants first, then activations).  Layout in HBM:
// every activation is token-major fp32 (rows = tokens of all B*r maps back to back, 256 channels).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <initializer_list>

#include "ddp_internal.h"

namespace ddp {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return DDP_E_LAUNCH;
  }
  return DDP_OK;
}

// ---- optional event profiler of one GEMM call site (bench.py roofline leg) ----------------------
namespace {
constexpr int PROF_MAX = 2048;
constexpr int PROF_ALL = 255;        // ddp_profile_begin(255): every tagged call site at once (ddp_profile_read per tag)
struct Prof {
  int tag = -1;
  int n = 0;
  hipEvent_t ev[2 * PROF_MAX];
  unsigned char rec_tag[PROF_MAX];
  float ms[PROF_MAX];
  bool created = false;
  bool resolved = false;             // ddp_profile_end ran for the records in ms[] (cleared by ddp_profile_begin)
} g_prof;
}  // namespace

void prof_begin(int tag, hipStream_t st) {
  if ((tag != g_prof.tag && g_prof.tag != PROF_ALL) || g_prof.n >= PROF_MAX) return;
  (void)hipEventRecord(g_prof.ev[2 * g_prof.n], st);
}
void prof_end(int tag, hipStream_t st) {
  if ((tag != g_prof.tag && g_prof.tag != PROF_ALL) || g_prof.n >= PROF_MAX) return;
  (void)hipEventRecord(g_prof.ev[2 * g_prof.n + 1], st);
  g_prof.rec_tag[g_prof.n] = (unsigned char)tag;
  ++g_prof.n;
}

#define DDP_TRY(expr)            \
  do {                           \
    int _rc = (expr);            \
    if (_rc != DDP_OK) return _rc; \
  } while (0)

namespace {

inline size_t align64(size_t floats) { return (floats + 63) & ~size_t(63); }  // 256-byte granules

// The one workspace carver: consecutive regions of `count` elements of T, each rounded up to a 256-byte granule.  A null base
// carves sizes only - every take() returns nullptr and `off` ends at the byte count (the *_workspace queries).  With a base,
// take(0) is a non-null pointer of zero length: "carved but empty" and "not carved" (nullptr) stay different things.
struct Carver {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + 255) / 256 * 256;
    return p;
  }
};

// The caller-visible tail of a sampler workspace (ddp_sample and ddp_sample_fcn): the buffers the caller reads or writes directly,
// each present only with its flag (include/ddp_mi355x.h, at ddp_query_workspace)
struct CallerRegions {
  // DDP_FLAG_SCORE_PRIOR: the caller-written NCHW map (B, num_classes, h, w) and the token-major rows k_score_prior_rows writes:
  // (B * N, KP), KP = 64 * ceil(num_classes / 64), normalised, zero padded (the seg tails' and k_seg_update's addend)
  float *sprior_rows = nullptr, *sprior_map = nullptr;
  // DDP_FLAG_CLASS_PRIOR: the caller-written table (B, 256) and the per-image vectors k_class_prior writes: (B, 256) bias + prior rows
  // (the seg tails' accumulator start), then (B, 256) prior rows (k_seg_update's addend)
  float *cprior_rows = nullptr, *cprior_table = nullptr;
  // DDP_FLAG_PRIOR_START: the caller-written prior map (B, N) - seg uint8, depth fp32, bev uint32 - and the start map (B, r, Cm, h, w)
  // k_prior_start_* writes (without DDP_FLAG_SEEDED_NOISE; with it seed_noise is the start map, mixed in place)
  float* prior_start = nullptr;
  void* prior_map = nullptr;
  // DDP_FLAG_X0_HINTS: the caller-written hint map (B, N) - seg uint8, depth fp32 - and its per-row form (M0), written by k_hint_rows_*
  void *hint_rows = nullptr, *hint_map = nullptr;
  float* seed_noise = nullptr;   // DDP_FLAG_SEEDED_NOISE: (B, r, Cm, h, w) start noise of the call, written by k_noise_fill_nchw
  // DDP_FLAG_STEP_RECORD: the record (K, M) - seg uint8, depth fp32, bev uint32 - and the disagreement map (B, Nh)
  unsigned char* step_rec = nullptr;
  float* step_map = nullptr;
};

struct Layout : CallerRegions {
  // dims
  int B, r, K, L, Kc, Cx, Cm, h, w, hh, wh, N, Nh, R;
  size_t M0, M;   // tokens at (h,w) and at the head grid, over all B*r maps
  int ldl;        // row stride of logits / prob buffers
  // constants
  float *tin = nullptr, *u = nullptr, *hid = nullptr, *temb = nullptr, *film = nullptr, *aff = nullptr, *lut = nullptr,
        *wx = nullptr, *wm = nullptr, *wtap = nullptr;
  float *wcat[DDP_MAX_LAYERS] = {}, *bcat[DDP_MAX_LAYERS] = {}, *py[DDP_MAX_LAYERS] = {}, *px[DDP_MAX_LAYERS] = {};
  // activations
  float *xproj = nullptr, *mask = nullptr, *pred = nullptr, *feat0 = nullptr, *q = nullptr, *q1 = nullptr, *v = nullptr,
        *s = nullptr, *samp = nullptr, *hbuf = nullptr, *logits = nullptr, *prob = nullptr, *snoise = nullptr, *xtok = nullptr;
  // bf16x3 mode: split weights and split fragment-major activations
  int b3;
  unsigned char* x0_trace = nullptr;   // DDP_FLAG_RECORD_X0: (K, M) argmax class of every step (seg with DDP_FLAG_STEP_RECORD: == step_rec)
  bool fused_layer, fused_pro;   // bf16x3: persistent layer kernel / step-prologue kernel in use (cfg->flags)
  bool guess_zero;               // DDP_FLAG_GATHER_GUESS_ZERO
  SplitW wp_x, wp_m, wp_head, wp_v[DDP_MAX_LAYERS], wp_cat[DDP_MAX_LAYERS], wp_o[DDP_MAX_LAYERS], wp_f0[DDP_MAX_LAYERS],
      wp_f1[DDP_MAX_LAYERS];
  unsigned short *q_sb = nullptr, *q1_sb = nullptr, *s_sb = nullptr, *h_sb = nullptr,
                 *in_sb = nullptr;                      // in_sb: mask / x / feat staging (row-major producers)
  float* vpad = nullptr;                                // zero-padded value maps (R, hh+2, wh+2, 256) written by the layer kernel
  size_t vpad_floats = 0;
  unsigned char* wstream[DDP_MAX_LAYERS] = {};          // layer kernel: weight stream (stage images) per layer
  float* bias_ext[DDP_MAX_LAYERS] = {};                 //               fc1 bias | next value_proj bias | zeros
  unsigned char* pro_stream = nullptr;                  // step prologue: W_m (8 wide) + layer 0's value / sampling proj (11 tall)
  float* pro_bias = nullptr;                            //                layer 0's value_proj bias at [1024, 1280)
  float* ubuf = nullptr;                                // u = W_m . m_t, fp32 fragment-major (fused seg tails)
  float* tlut = nullptr;                                // seg: (Kc + 1, 256) = LUT . W_m^T; bev (<= 8 classes): (2^Kc, 256) = LUT64 . W_m^T
  float* lut64 = nullptr;                               // bev (<= 8 classes): the 2^Kc x0 vectors of a pixel
  float* wvs = nullptr;                                 // depth: W_v0 w_m (256) | W_cat0 w_m (96): the rank-1 terms of the GEMM-free step head
  float *xproj_f = nullptr, *rs0 = nullptr,             // depth chain (inside hbuf, unused by the bf16x3 engine otherwise): xproj fragment-major,
        *rvpad = nullptr;                               // W_cat0 xproj (M, 96), zero-padded map of W_v0 xproj + b_v0; nullptr: does not fit
  unsigned char* tail4_stream = nullptr;                // fused tail: conv_seg images + layer 0's 11 projection images
  unsigned char* head7_stream = nullptr;                // first step's head from NCHW (k_layer MODE 7): W_m 8 wide + W_x 8 wide + 11
  unsigned char* lt_stream = nullptr;                   // last layer + tail (k_layer MODE 6): 72 stages of layer L-1 + tail4_stream
  float* lt_bias = nullptr;                             //   fc1 bias of layer L-1 | layer 0's value_proj bias at [1024, 1280)
  float* tail4_bias = nullptr;                          //             conv_seg bias | layer 0's value_proj bias at [1024, 1280)
  unsigned char* tail_stream = nullptr;                 // seg tail: conv_seg stage images (2 per 64 classes)
  float* tail_bias = nullptr;                           //           conv_seg bias, zero padded
  // binned depth head (cfg->depth_n_bins > 0): conv_depth to n_bins channels + k_depth_bins
  int nbins, bins_ld, bins_guard;
  float *bins_tab = nullptr, *bins_bias = nullptr,      // bin centres, conv bias (256, zero padded),
        *bins_wpack = nullptr;                          // weights tap-major (256, 2304)
  unsigned short* bins_wsplit = nullptr;                // bf16x3: split planes of bins_wpack
  unsigned char* bins_stream = nullptr;                 // bf16x3: the 72 stage images of the implicit 3x3 GEMM
  float *bins_in = nullptr, *bins_logits = nullptr;     // fp32 engine: zero-bordered grid of the layer output; logits (see carve)
  // bev head variants (ABI 7).  seg3: conv_seg is 3x3 - it shares the bins_* buffers of the binned depth head (the same implicit
  // GEMM / nine shifted GEMMs, on the head grid).  prescale: the grid transform resamples the map prescaled to (hp, wp), which is
  // materialised in `pre` (R maps, row-major) by k_bev_prescale
  bool seg3 = false, prescale = false;
  int hp = 0, wp = 0;
  float pre_rscale = 1.f;
  float* pre = nullptr;
  size_t const_bytes;   // region A (model constants): a prefix of the workspace that does not depend on the geometry
  size_t total;
};

// floor(in * p) as F.interpolate computes its output size (double arithmetic on the given scale factor).  p is the FLOAT field: a
// caller whose factor is a double that float cannot hold (0.9: floor(10 * 0.9f) = 8, floor(10 * 0.9) = 9) must hand over a float
// that gives the sizes of its double (include/ddp_mi355x.h; ddp_amd.engine.check_bev_head does)
inline bool bev_prescaled(const ddp_cfg* c) { return c->bev_prescale != 0.f && c->bev_prescale != 1.f; }
inline double bev_prescaled_len(const ddp_cfg* c, int in_len) { return std::floor(double(in_len) * double(c->bev_prescale)); }

int validate(const ddp_cfg* c) {
  if (!c) {
    set_error("cfg is NULL");
    return DDP_E_NULL;
  }
  if (c->abi_version != DDP_ABI_VERSION) {
    set_error("abi_version %d != %d", c->abi_version, DDP_ABI_VERSION);
    return DDP_E_BADCFG;
  }
  if (c->task < 0 || c->task > 2) {
    set_error("unknown task %d", c->task);
    return DDP_E_BADCFG;
  }
  if (c->batch < 1 || c->randsteps < 1 || c->timesteps < 1 || c->timesteps > DDP_MAX_STEPS) {
    set_error("batch/randsteps/timesteps out of range (%d,%d,%d)", c->batch, c->randsteps, c->timesteps);
    return DDP_E_BADCFG;
  }
  if (c->num_layers < 1 || c->num_layers > DDP_MAX_LAYERS) {
    set_error("num_layers %d out of range", c->num_layers);
    return DDP_E_BADCFG;
  }
  if (c->h < 1 || c->w < 1 || c->head_h < 1 || c->head_w < 1) {
    set_error("bad spatial size");
    return DDP_E_BADCFG;
  }
  if (c->task != DDP_TASK_BEV && (c->head_h != c->h || c->head_w != c->w)) {
    set_error("head grid must equal (h,w) except for bev");
    return DDP_E_BADCFG;
  }
  if (c->feat_channels < 32 || c->feat_channels % 32) {
    set_error("feat_channels %d must be a positive multiple of 32", c->feat_channels);
    return DDP_E_BADCFG;
  }
  if (c->task != DDP_TASK_DEPTH && (c->num_classes < 1 || c->num_classes > 256)) {
    set_error("num_classes %d out of range [1,256]", c->num_classes);
    return DDP_E_BADCFG;
  }
  if (c->task == DDP_TASK_BEV && c->num_classes > 32 && (c->flags & DDP_FLAG_PRIOR_START)) {
    set_error("DDP_FLAG_PRIOR_START: a bev prior is one uint32 bit word per pixel (num_classes %d > 32)", c->num_classes);
    return DDP_E_BADCFG;
  }
  if (c->task == DDP_TASK_BEV && c->num_classes > 32) {
    set_error("bev supports at most 32 classes");
    return DDP_E_BADCFG;
  }
  if (c->flags & ~(DDP_FLAG_UNFUSED_LAYER | DDP_FLAG_UNFUSED_PROLOGUE | DDP_FLAG_RECORD_X0 | DDP_FLAG_GATHER_GUESS_ZERO |
                   DDP_FLAG_FORCE_X0 | DDP_FLAG_UNFUSED_TAIL | DDP_FLAG_SB_HEAD | DDP_FLAG_DEPTH_SCALE_UP | DDP_FLAG_DEPTH_NO_EPS |
                   DDP_FLAG_STEP_RECORD | DDP_FLAG_SEEDED_NOISE | DDP_FLAG_DDPM_CHAIN | DDP_FLAG_X0_HINTS |
                   DDP_FLAG_PRIOR_START | DDP_FLAG_CLASS_PRIOR | DDP_FLAG_SCORE_PRIOR)) {
    set_error("unknown flags 0x%x", c->flags);
    return DDP_E_BADCFG;
  }
  if ((c->flags & DDP_FLAG_SCORE_PRIOR) && c->task != DDP_TASK_SEG) {
    set_error("DDP_FLAG_SCORE_PRIOR exists for the segmentation sampler only (task %d: no depth or bev prior is built)", c->task);
    return DDP_E_BADCFG;
  }
  if ((c->flags & DDP_FLAG_CLASS_PRIOR) && c->task != DDP_TASK_SEG) {
    set_error("DDP_FLAG_CLASS_PRIOR exists for the segmentation sampler only (task %d: no depth or bev prior is built)", c->task);
    return DDP_E_BADCFG;
  }
  if (c->flags & DDP_FLAG_X0_HINTS) {
    if (c->task == DDP_TASK_BEV) {
      set_error("DDP_FLAG_X0_HINTS exists for the segmentation and depth samplers (task %d: the bev sampler takes no hints)", c->task);
      return DDP_E_BADCFG;
    }
    if (c->flags & DDP_FLAG_FORCE_X0) {
      set_error("DDP_FLAG_X0_HINTS cannot be combined with DDP_FLAG_FORCE_X0 (both supply the class the step feeds back)");
      return DDP_E_BADCFG;
    }
    if (c->task == DDP_TASK_SEG && c->num_classes > 255) {
      set_error("DDP_FLAG_X0_HINTS: num_classes %d leaves no uint8 value for a free pixel (<= 255 classes)", c->num_classes);
      return DDP_E_BADCFG;
    }
  }
  if ((c->flags & DDP_FLAG_DDPM_CHAIN) && (c->task != DDP_TASK_SEG || c->sampler != DDP_SAMPLER_DDPM)) {
    // (for any other task or sampler the bit is as unknown as an undefined one, and is reported that way)
    set_error("unknown flags 0x%x for task %d, sampler %d: DDP_FLAG_DDPM_CHAIN exists for the segmentation ddpm sampler only", c->flags,
              c->task, c->sampler);
    return DDP_E_BADCFG;
  }
  if ((c->flags & (DDP_FLAG_FORCE_X0 | DDP_FLAG_RECORD_X0)) && c->task != DDP_TASK_SEG) {
    set_error("DDP_FLAG_RECORD_X0 / DDP_FLAG_FORCE_X0 exist for the segmentation sampler only (task %d)", c->task);
    return DDP_E_BADCFG;
  }
  if ((c->flags & DDP_FLAG_STEP_RECORD) && (c->flags & DDP_FLAG_FORCE_X0)) {
    set_error("DDP_FLAG_STEP_RECORD cannot be combined with DDP_FLAG_FORCE_X0 (a test instrument with its own trace layout)");
    return DDP_E_BADCFG;
  }
  if (c->depth_n_bins != 0 && c->task != DDP_TASK_DEPTH) {
    set_error("depth_n_bins configures the depth head only (task %d)", c->task);
    return DDP_E_BADCFG;
  }
  if (c->depth_n_bins < 0 || c->depth_n_bins > DDP_MAX_DEPTH_BINS) {
    set_error("depth_n_bins %d out of range [0,%d]", c->depth_n_bins, DDP_MAX_DEPTH_BINS);
    return DDP_E_BADCFG;
  }
  if (c->depth_norm < DDP_DEPTH_NORM_LINEAR || c->depth_norm > DDP_DEPTH_NORM_SIGMOID || (c->depth_norm && !c->depth_n_bins)) {
    set_error("depth_norm %d: DDP_DEPTH_NORM_* of a binned depth head", c->depth_norm);
    return DDP_E_BADCFG;
  }
  if ((c->head_min_depth != 0.f || c->head_max_depth != 0.f) && c->task != DDP_TASK_DEPTH) {
    set_error("head_min_depth / head_max_depth configure the depth head only (task %d)", c->task);
    return DDP_E_BADCFG;
  }
  if ((c->flags & (DDP_FLAG_DEPTH_SCALE_UP | DDP_FLAG_DEPTH_NO_EPS)) && c->task != DDP_TASK_DEPTH) {
    set_error("DDP_FLAG_DEPTH_* configure the depth head only (task %d)", c->task);
    return DDP_E_BADCFG;
  }
  if ((c->bev_prescale != 0.f || c->bev_seg_kernel != 0) && c->task != DDP_TASK_BEV) {
    set_error("bev_prescale / bev_seg_kernel configure the bev head only (task %d)", c->task);
    return DDP_E_BADCFG;
  }
  if (c->bev_seg_kernel != 0 && c->bev_seg_kernel != 1 && c->bev_seg_kernel != 3) {
    set_error("bev_seg_kernel %d: conv_seg is 1x1 (0 / 1) or 3x3 (3)", c->bev_seg_kernel);
    return DDP_E_BADCFG;
  }
  if (!(c->bev_prescale >= 0.f) || !std::isfinite(c->bev_prescale)) {
    set_error("bev_prescale %g must be a positive factor (0 / 1: none)", double(c->bev_prescale));
    return DDP_E_BADCFG;
  }
  if (bev_prescaled(c)) {
    const double hp = bev_prescaled_len(c, c->h), wp = bev_prescaled_len(c, c->w);
    if (hp < 1.0 || wp < 1.0) {
      set_error("bev_prescale %g: prescaled map %.0f x %.0f is empty", double(c->bev_prescale), hp, wp);
      return DDP_E_BADCFG;
    }
    if (hp * wp > double(DDP_BEV_MAX_PRESCALE_AREA) * c->h * c->w ||
        double(c->batch) * c->randsteps * hp * wp > double(DDP_MAX_CALL_TOKENS)) {
      set_error("bev_prescale %g: prescaled map %.0f x %.0f exceeds %d x the map (or the per-call limit of 1.5e9 / 1024 prescaled tokens)",
                double(c->bev_prescale), hp, wp, DDP_BEV_MAX_PRESCALE_AREA);
      return DDP_E_BADCFG;
    }
  }
  if (c->gemm_mode != DDP_GEMM_F32_MFMA && c->gemm_mode != DDP_GEMM_BF16X3) {
    set_error("unknown gemm_mode %d", c->gemm_mode);
    return DDP_E_BADCFG;
  }
  if (c->sampler != DDP_SAMPLER_DDIM && !(c->sampler == DDP_SAMPLER_DDPM && c->task == DDP_TASK_SEG)) {
    set_error("sampler %d unsupported for task %d (the reference defines ddpm for seg only)", c->sampler, c->task);
    return DDP_E_BADCFG;
  }
  const double tokens = double(c->batch) * c->randsteps * double(c->head_h) * c->head_w;
  if (tokens > 1.5e9 / 1024) {  // keep int row*1024 offsets and 32-bit row counters safe
    set_error("problem too large for one call: %.0f tokens", tokens);
    return DDP_E_BADCFG;
  }
  return DDP_OK;
}

// bytes of the step record (include/ddp_mi355x.h): one element per (step, map, head-grid token)
inline size_t step_record_bytes(const ddp_cfg* c) {
  return size_t(c->timesteps) * c->batch * c->randsteps * c->head_h * c->head_w * (c->task == DDP_TASK_SEG ? 1 : 4);
}

// The tail of a sampler workspace, in its one fixed order (the ordered list of include/ddp_mi355x.h at ddp_query_workspace; the same
// table on the host side: ddp_amd.engine.caller_regions).  Every group exists only with its flag, so every offset in front of a group
// is the one of the cfg without that flag:
//   score prior    the private token-major rows, then the caller's NCHW map
//   class prior    the private per-image vectors, then the caller's table
//   prior start    the start map (only without DDP_FLAG_SEEDED_NOISE: with it the seeded-noise buffer is the start map), then the
//                  caller's prior map
//   x0 hints       the private row buffer, then the caller's map
//   seeded noise   the start noise of the call
//   step record    the record, then the disagreement map: the LAST two buffers
// ddp_sample_fcn refuses the first four flags (validate_fcn_loop): its tail is the last two groups.
void carve_caller_regions(const ddp_cfg* c, Carver& cv, CallerRegions* o) {
  const size_t B = c->batch, BN = B * c->h * c->w, M0 = BN * c->randsteps;
  const size_t Cm = c->task == DDP_TASK_DEPTH ? 1 : 256;      // channels of the noisy map
  const size_t px = c->task == DDP_TASK_SEG ? 1 : 4;          // bytes per pixel of a hint / prior map: uint8 classes, else fp32 / uint32
  if (c->flags & DDP_FLAG_SCORE_PRIOR) {
    o->sprior_rows = cv.take<float>(BN * size_t((c->num_classes + 63) / 64 * 64));
    o->sprior_map = cv.take<float>(BN * size_t(c->num_classes));
  }
  if (c->flags & DDP_FLAG_CLASS_PRIOR) {
    o->cprior_rows = cv.take<float>(2 * B * 256);
    o->cprior_table = cv.take<float>(B * 256);
  }
  if (c->flags & DDP_FLAG_PRIOR_START) {
    if (!(c->flags & DDP_FLAG_SEEDED_NOISE)) o->prior_start = cv.take<float>(M0 * Cm);
    o->prior_map = cv.take<unsigned char>(BN * px);
  }
  if (c->flags & DDP_FLAG_X0_HINTS) {
    o->hint_rows = cv.take<unsigned char>(M0 * px);
    o->hint_map = cv.take<unsigned char>(BN * px);
  }
  if (c->flags & DDP_FLAG_SEEDED_NOISE) o->seed_noise = cv.take<float>(M0 * Cm);
  if (c->flags & DDP_FLAG_STEP_RECORD) {
    o->step_rec = cv.take<unsigned char>(step_record_bytes(c));
    o->step_map = cv.take<float>(B * c->head_h * c->head_w);
  }
}

void carve(const ddp_cfg* c, char* base, Layout* o) {
  Carver cv{base};
  auto takeb = [&](size_t nbytes) { return cv.take<unsigned char>(nbytes); };
  o->B = c->batch;
  o->r = c->randsteps;
  o->K = c->timesteps;
  o->L = c->num_layers;
  o->Kc = c->task == DDP_TASK_DEPTH ? 1 : c->num_classes;
  o->Cx = c->feat_channels;
  o->Cm = c->task == DDP_TASK_DEPTH ? 1 : 256;
  o->h = c->h;
  o->w = c->w;
  o->hh = c->head_h;
  o->wh = c->head_w;
  o->N = c->h * c->w;
  o->Nh = c->head_h * c->head_w;
  o->R = c->batch * c->randsteps;
  o->M0 = size_t(o->R) * o->N;
  o->M = size_t(o->R) * o->Nh;
  o->ldl = c->task == DDP_TASK_SEG ? ((o->Kc + 31) / 32) * 32 : 32;
  // ---- region A: MODEL constants.  Sizes depend on (task, K, L, K_cls, Cx, gemm_mode) only - not on batch, r or the map
  // size - so this prefix of the workspace stays valid when only the geometry changes (ddp_prepare_geometry): the
  // reference's own test protocol is one image per call with a new (h, w) almost every call (tools/test.py:214-219)
  o->tin = cv.take<float>(DDP_MAX_STEPS);
  o->u = cv.take<float>(size_t(o->K) * DDP_SINU_FEATS);
  o->hid = cv.take<float>(size_t(o->K) * DDP_TIME_DIM);
  o->temb = cv.take<float>(size_t(o->K) * DDP_TIME_DIM);
  o->film = cv.take<float>(size_t(o->K) * o->L * 512);
  o->aff = cv.take<float>(size_t(o->K) * o->L * 512);   // norms.1 affine x FiLM per (step, layer)
  o->lut = cv.take<float>(size_t(o->Kc + 1) * 256);
  o->wx = cv.take<float>(size_t(256) * o->Cx);
  o->wm = cv.take<float>(size_t(256) * o->Cm);
  o->wtap = cv.take<float>(size_t(9) * 256);
  o->nbins = c->task == DDP_TASK_DEPTH ? c->depth_n_bins : 0;
  o->seg3 = c->task == DDP_TASK_BEV && c->bev_seg_kernel == 3;
  o->prescale = c->task == DDP_TASK_BEV && bev_prescaled(c);
  const bool conv3 = o->nbins || o->seg3;     // a 3x3 head convolution to more than one channel
  o->bins_tab = o->nbins ? cv.take<float>(DDP_MAX_DEPTH_BINS) : nullptr;
  o->bins_bias = conv3 ? cv.take<float>(256) : nullptr;
  o->bins_wpack = conv3 ? cv.take<float>(size_t(256) * 2304) : nullptr;
  for (int l = 0; l < DDP_MAX_LAYERS; ++l) {
    const bool on = l < o->L;
    o->wcat[l] = on ? cv.take<float>(96 * 256) : nullptr;
    o->bcat[l] = on ? cv.take<float>(96) : nullptr;
  }
  o->b3 = c->gemm_mode == DDP_GEMM_BF16X3;
  o->guess_zero = (c->flags & DDP_FLAG_GATHER_GUESS_ZERO) != 0;
  o->fused_layer = o->b3 && !(c->flags & DDP_FLAG_UNFUSED_LAYER);
  o->fused_pro = o->fused_layer && !(c->flags & DDP_FLAG_UNFUSED_PROLOGUE);
  const bool segp = c->task == DDP_TASK_SEG;
  if (o->b3) {
    // split weights: 3 bf16 planes per fp32 element = 6 bytes
    auto takew = [&](size_t rows, size_t K) {
      SplitW w;
      w.p = cv.take<unsigned short>(rows * K * 3);
      w.comp_stride = rows * K;
      return w;
    };
    const int head_rows = c->task == DDP_TASK_DEPTH ? 9 : o->Kc;
    o->wp_x = takew(256, o->Cx);
    o->wp_m = takew(256, 256);
    o->wp_head = takew(head_rows, 256);
    for (int l = 0; l < DDP_MAX_LAYERS; ++l) {
      if (l >= o->L) continue;
      o->wp_v[l] = takew(256, 256);
      o->wp_cat[l] = takew(96, 256);
      o->wp_o[l] = takew(256, 256);
      o->wp_f0[l] = takew(DDP_FFN, 256);
      o->wp_f1[l] = takew(256, DDP_FFN);
      o->wstream[l] = takeb(b3_layer_stream_bytes());
      o->bias_ext[l] = cv.take<float>(size_t(b3_layer_bias_floats()));
    }
    o->tail_stream = takeb(size_t(8) * 48 * 1024);
    o->tail_bias = cv.take<float>(size_t(b3_layer_bias_floats()));
    o->pro_stream = takeb(b3_prologue_stream_bytes());
    o->pro_bias = cv.take<float>(size_t(b3_layer_bias_floats()));
    o->tail4_stream = takeb(segp ? size_t(8 + 11) * 48 * 1024 : 0);
    o->tail4_bias = cv.take<float>(segp ? size_t(b3_layer_bias_floats()) : 0);
    o->head7_stream = (segp && o->Cx == 256) ? takeb(size_t(8 + 8 + 11) * 48 * 1024) : nullptr;
    // last layer + tail (k_layer MODE 6 / 8 / 9): seg 72 + 2 * chunks + 11 images, bev (<= 32 classes) and depth (9 taps) 72 + 2
    // (not for the 3x3 conv_seg of the bev head: its last layer is a plain layer, no tail stream is built or read)
    const bool lt = o->L >= 1 && (segp ? b3_layer_tail_supported(o->Kc) : o->Kc <= 32) && !o->seg3;
    o->lt_stream = lt ? takeb(size_t(segp ? 72 + 8 + 11 : 72 + 2) * 48 * 1024) : nullptr;
    o->lt_bias = lt ? cv.take<float>(size_t(b3_layer_bias_floats())) : nullptr;
    const bool bev_tab = c->task == DDP_TASK_BEV && o->Kc <= 8;
    o->tlut = cv.take<float>(segp ? size_t(o->Kc + 1) * 256 : bev_tab ? (size_t(1) << o->Kc) * 256 : 0);
    o->lut64 = bev_tab ? cv.take<float>((size_t(1) << o->Kc) * 256) : nullptr;
    o->wvs = c->task == DDP_TASK_DEPTH ? cv.take<float>(512) : nullptr;
    o->bins_wsplit = conv3 ? cv.take<unsigned short>(size_t(256) * 2304 * 3) : nullptr;
    o->bins_stream = conv3 ? takeb(size_t(72) * 48 * 1024) : nullptr;
  }
  o->const_bytes = cv.off;
  // ---- region B: everything that depends on the geometry (batch, r, map size): positional tables, activations
  for (int l = 0; l < DDP_MAX_LAYERS; ++l) {
    const bool on = l < o->L;
    o->py[l] = on ? cv.take<float>(size_t(o->hh) * 96) : nullptr;
    o->px[l] = on ? cv.take<float>(size_t(o->wh) * 96) : nullptr;
  }
  // (xproj in whole tiles: the first step's head may write it fragment-major)
  o->xproj = cv.take<float>((size_t(o->B) * o->N + 127) / 128 * 128 * 256);
  o->mask = cv.take<float>(o->M0 * (c->task == DDP_TASK_DEPTH ? 1 : 256));
  o->pred = cv.take<float>(c->task == DDP_TASK_DEPTH ? o->M0 : 0);
  o->feat0 = cv.take<float>(c->task == DDP_TASK_BEV ? o->M0 * 256 : 0);
  const size_t Mp = (o->M + 255) / 256 * 256;               // fragment-major buffers hold whole block tiles (128 / 256 tokens)
  o->q = cv.take<float>(Mp * 256);                          // fragment-major
  o->q1 = cv.take<float>(Mp * 256);                         // fragment-major
  o->v = cv.take<float>(o->M * 256);                        // row-major (gather taps want a head's 128 B contiguous)
  o->s = cv.take<float>(o->M * 256);                        // row-major
  o->samp = cv.take<float>(o->M * DDP_SAMP_STRIDE);
  size_t hb = Mp * DDP_FFN;                                 // fragment-major
  const size_t xt = size_t(o->B) * o->N * o->Cx;
  if (xt > hb) hb = xt;
  o->hbuf = cv.take<float>(hb);
  o->xtok = o->hbuf;  // x in token-major form is dead once xproj exists
  // (seg: the layer kernel's tails keep scores / probabilities fragment-major: whole 128-token TILES x whole 64-class chunks -
  // the wholly invalid waves of the last tile pre-load their groups' accumulators like every other wave)
  const size_t pfl = c->task == DDP_TASK_SEG ? (o->M + 127) / 128 * 128 * size_t((o->Kc + 63) / 64 * 64) : 0;
  o->logits = cv.take<float>(o->M * o->ldl > pfl ? o->M * o->ldl : pfl);
  o->prob = cv.take<float>(o->M * o->ldl > pfl ? o->M * o->ldl : pfl);
  o->snoise = cv.take<float>(c->sampler == DDP_SAMPLER_DDPM ? o->M0 * 256 : 0);
  // binned depth head: bf16x3 - the stream GEMM writes the logits fp32 fragment-major with 256 channels (rows padded to 256);
  // fp32 engine - the layer output on a zero-bordered grid (+ guard rows: the nine taps are row offsets of up to w + 3) and the
  // logits on that grid, rows of bins_ld floats
  // (3x3 conv_seg of the bev head: the same two buffers on the head grid, K_cls channels)
  o->bins_ld = ((o->seg3 ? o->Kc : o->nbins) + 3) / 4 * 4;
  o->bins_guard = o->wh + 3;
  if (conv3) {
    const size_t padded = size_t(o->R) * (o->hh + 2) * (o->wh + 2);
    if (o->b3) {
      o->bins_logits = cv.take<float>(Mp * 256);
    } else {
      o->bins_in = cv.take<float>((padded + 2 * size_t(o->bins_guard)) * 256);
      o->bins_logits = cv.take<float>(padded * o->bins_ld);
    }
  }
  // prescaled map: R row-major maps of (hp, wp) x 256 floats, whole 4-token blocks as k_bev_prescale writes them
  if (o->prescale) {
    o->hp = int(bev_prescaled_len(c, c->h));
    o->wp = int(bev_prescaled_len(c, c->w));
    o->pre_rscale = float(1.0 / double(c->bev_prescale));
    o->pre = cv.take<float>((size_t(o->R) * o->hp * o->wp + 3) / 4 * 4 * 256);
  }
  o->x0_trace = takeb((c->flags & (DDP_FLAG_RECORD_X0 | DDP_FLAG_FORCE_X0)) && c->task == DDP_TASK_SEG && !(c->flags & DDP_FLAG_STEP_RECORD)
                           ? (c->flags & DDP_FLAG_FORCE_X0 ? 2 : 1) * size_t(o->K) * o->M
                           : 0);
  if (o->b3) {
    auto takesb = [&](size_t rows, size_t C) {       // SB: 6 bytes per element, rows padded to 256
      const size_t rp = (rows + 255) / 256 * 256;
      return cv.take<unsigned short>(rp * C * 3);
    };
    // + one more zero row: a sample clamped to y = h reads (with weight 0) the row below the bottom border, which for the
    // last map would otherwise be whatever follows in the workspace (0 x NaN = NaN)
    o->vpad_floats = (size_t(o->R) * (o->hh + 2) + 1) * (o->wh + 2) * 256 + 256;
    o->vpad = cv.take<float>(o->vpad_floats);
    o->ubuf = cv.take<float>(segp ? (o->M + 255) / 256 * 256 * 256 : 0);
    o->q_sb = takesb(o->M, 256);
    o->q1_sb = takesb(o->M, 256);
    o->s_sb = takesb(o->M, 256);
    o->h_sb = takesb(o->M, DDP_FFN);
    // in_sb serves the noisy map / a layer input (max(M0, M) rows of 256) and x (B.N rows of Cx).  Both are written in whole 64-row
    // blocks and read in whole 256-row GEMM tiles, so the PADDED sizes decide: with r >= 2 and 256 < Cx <= 256 r the smaller
    // product can need the larger buffer (B.N = 100, r = 2, Cx = 512: 256 x 512 elements against 256 x 256)
    auto rp256 = [](size_t rows) { return (rows + 255) / 256 * 256; };
    size_t in_rows = o->M0 > o->M ? o->M0 : o->M, in_c = 256;
    if (rp256(size_t(o->B) * o->N) * o->Cx > rp256(in_rows) * in_c) {
      in_rows = size_t(o->B) * o->N;
      in_c = o->Cx;
    }
    o->in_sb = takesb(in_rows, in_c);
  }
  // depth chain: three loop-invariant tensors in the FFN scratch of the fp32 engine (Mp x 1024 floats, idle on the bf16x3 engine)
  if (o->b3 && c->task == DDP_TASK_DEPTH && o->r == 1) {
    const size_t need = Mp * 256 + align64(o->M * 96) + o->vpad_floats;
    if (need <= Mp * DDP_FFN && base) {                 // (a one-row map does not fit: its padded map is 3x the map - the GEMM head stays)
      o->xproj_f = o->hbuf;
      o->rs0 = o->hbuf + Mp * 256;
      o->rvpad = o->rs0 + align64(o->M * 96);
    }
  }
  // (seg with DDP_FLAG_STEP_RECORD and DDP_FLAG_RECORD_X0: one buffer serves both flags - the x0 trace moves into the record)
  carve_caller_regions(c, cv, o);
  if (o->step_rec && c->task == DDP_TASK_SEG) o->x0_trace = o->step_rec;
  o->total = cv.off;
}

// `o` given: the geometry of the grid RESAMPLING, whose source is the prescaled map when there is one
BevGeom bev_geom(const ddp_cfg* c, const Layout* o = nullptr) {
  BevGeom g;
  g.h = o && o->prescale ? o->hp : c->h;
  g.w = o && o->prescale ? o->wp : c->w;
  g.hh = c->head_h;
  g.wh = c->head_w;
  for (int a = 0; a < 2; ++a) {
    g.in_min[a] = c->bev_in_min[a];
    g.in_max[a] = c->bev_in_max[a];
    g.out_first[a] = c->bev_out_first[a];
    g.out_step[a] = c->bev_out_step[a];
  }
  return g;
}

// the out-parameter of a *_workspace query
int check_bytes(const size_t* bytes) {
  if (!bytes) {
    set_error("bytes is NULL");
    return DDP_E_NULL;
  }
  return DDP_OK;
}

int check_ptr(const void* p, const char* name) {
  if (!p) {
    set_error("%s is NULL", name);
    return DDP_E_NULL;
  }
  if (reinterpret_cast<uintptr_t>(p) & 15) {
    set_error("%s is not 16-byte aligned", name);
    return DDP_E_ALIGN;
  }
  return DDP_OK;
}

int check_weights(const ddp_cfg* c, const ddp_weights* w) {
  if (!w) {
    set_error("weights is NULL");
    return DDP_E_NULL;
  }
  DDP_TRY(check_ptr(w->transform_w, "transform_w"));
  DDP_TRY(check_ptr(w->transform_b, "transform_b"));
  DDP_TRY(check_ptr(w->head_w, "head_w"));
  DDP_TRY(check_ptr(w->head_b, "head_b"));
  if (c->task != DDP_TASK_DEPTH) DDP_TRY(check_ptr(w->embedding, "embedding"));
  if (c->task == DDP_TASK_DEPTH && c->depth_n_bins) DDP_TRY(check_ptr(w->depth_bins, "depth_bins"));
  for (int l = 0; l < c->num_layers; ++l) {
    const ddp_layer_weights& lw = w->layers[l];
    const void* ps[] = {lw.sampling_offsets_w, lw.sampling_offsets_b, lw.attention_weights_w, lw.attention_weights_b,
                        lw.value_proj_w, lw.value_proj_b, lw.output_proj_w, lw.output_proj_b, lw.ffn0_w, lw.ffn0_b,
                        lw.ffn1_w, lw.ffn1_b, lw.norm0_w, lw.norm0_b, lw.norm1_w, lw.norm1_b};
    for (const void* p : ps) DDP_TRY(check_ptr(p, "layer weight"));
  }
  return DDP_OK;
}

// time embedding + FiLM for S time inputs already on device at tin (segmentors/ddp.py:107-112,
// utils/transformer.py:275-278)
int time_embed_dev(const ddp_weights* w, int L, const float* tin, int S, float* u, float* hid, float* temb,
                   float* film, hipStream_t st) {
  DDP_TRY(launch_sinusoid(w->time_freq, tin, S, u, st));
  DDP_TRY(launch_matvec(w->time1_w, w->time1_b, u, hid, DDP_SINU_FEATS, DDP_TIME_DIM, S, DDP_SINU_FEATS,
                        DDP_TIME_DIM, 0, 1, st));
  DDP_TRY(launch_matvec(w->time3_w, w->time3_b, hid, temb, DDP_TIME_DIM, DDP_TIME_DIM, S, DDP_TIME_DIM,
                        DDP_TIME_DIM, 0, 0, st));
  for (int l = 0; l < L; ++l) {
    if (!w->layers[l].time_w) continue;
    DDP_TRY(launch_matvec(w->layers[l].time_w, w->layers[l].time_b, temb, film + size_t(l) * 512, DDP_TIME_DIM, 512,
                          S, DDP_TIME_DIM, L * 512, 2, 0, st));
  }
  return DDP_OK;
}

// norms.1 affine folded with the per-(step,layer) FiLM vectors
int fold_affine_dev(const ddp_weights* w, int L, int S, const float* film, float* aff, hipStream_t st) {
  for (int l = 0; l < L; ++l) {
    const ddp_layer_weights& lw = w->layers[l];
    for (int s = 0; s < S; ++s) {
      float* dst = aff + (size_t(s) * L + l) * 512;
      if (lw.time_w && film) {
        DDP_TRY(launch_fold_affine(lw.norm1_w, lw.norm1_b, film + (size_t(s) * L + l) * 512, dst, 1, st));
      } else {
        DDP_TRY(launch_pack_rows(lw.norm1_w, 1, lw.norm1_b, 1, dst, 256, st));
      }
    }
  }
  return DDP_OK;
}

// geometry-dependent constants (region B): separable positional tables of every layer (from the packed offset / attention
// projections of region A) and the zero border of the padded value maps
int prepare_geometry(const Layout& o, hipStream_t st) {
  for (int l = 0; l < o.L; ++l) DDP_TRY(launch_pos_tables(o.wcat[l], o.bcat[l], o.py[l], o.px[l], o.hh, o.wh, st));
  // border rows of the padded value maps: zero once, the layer kernel only ever writes the interior
  if (o.b3 && hipMemsetAsync(o.vpad, 0, o.vpad_floats * sizeof(float), st) != hipSuccess) {
    set_error("hipMemsetAsync(vpad) failed");
    return DDP_E_LAUNCH;
  }
  if (o.rvpad && hipMemsetAsync(o.rvpad, 0, o.vpad_floats * sizeof(float), st) != hipSuccess) {
    set_error("hipMemsetAsync(rvpad) failed");
    return DDP_E_LAUNCH;
  }
  return DDP_OK;
}

// a bias table of the layer kernel: b3_layer_bias_floats() zeros, then each segment copied in at its offset (src nullptr: stays zero)
struct BiasSeg {
  int at;
  const float* src;
  int n;
};
int bias_table(float* dst, std::initializer_list<BiasSeg> segs, const char* what, hipStream_t st) {
  bool ok = hipMemsetAsync(dst, 0, size_t(b3_layer_bias_floats()) * sizeof(float), st) == hipSuccess;
  for (const BiasSeg& s : segs)
    ok = ok && (!s.src || hipMemcpyAsync(dst + s.at, s.src, size_t(s.n) * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess);
  if (!ok) {
    set_error("%s: bias table copy failed", what);
    return DDP_E_LAUNCH;
  }
  return DDP_OK;
}

// layer l's value / sampling projections as 11 stage images from image `base` on: [Wv: 8 tall][Wcat: 2 tall + 1 split-K]
int build_proj_images(const Layout& o, int l, unsigned char* stream, int base, hipStream_t st) {
  DDP_TRY(launch_build_stages(o.wp_v[l].p, o.wp_v[l].comp_stride, 256, 256, 1, 4, 2, base, 0, 1, 2, stream, st));
  DDP_TRY(launch_build_stages(o.wp_cat[l].p, o.wp_cat[l].comp_stride, 256, 96, 1, 1, 2, base + 8, 0, 1, 2, stream, st));
  return launch_build_stages(o.wp_cat[l].p, o.wp_cat[l].comp_stride, 256, 96, 2, 1, 1, base + 10, 64, 0, 0, stream, st);
}

// model constants that do not depend on the schedule (region A)
int prepare_model(const ddp_cfg* c, const ddp_weights* w, const Layout& o, hipStream_t st) {
  DDP_TRY(launch_pack_cols(w->transform_w, o.Cx + o.Cm, 0, 256, o.Cx, o.wx, st));
  DDP_TRY(launch_pack_cols(w->transform_w, o.Cx + o.Cm, o.Cx, 256, o.Cm, o.wm, st));
  if (c->task == DDP_TASK_SEG) DDP_TRY(launch_build_lut(w->embedding, o.lut, o.Kc + 1, c->bit_scale, st));
  if (c->task == DDP_TASK_DEPTH) DDP_TRY(launch_pack_conv3x3(w->head_w, o.wtap, st));
  if (o.seg3) {
    // 3x3 conv_seg (K_cls,256,3,3): packed tap-major like the binned conv_depth below, zero rows beyond K_cls, bias zero-padded
    if (hipMemsetAsync(o.bins_wpack, 0, size_t(256) * 2304 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(o.bins_bias, 0, 256 * sizeof(float), st) != hipSuccess ||
        hipMemcpyAsync(o.bins_bias, w->head_b, size_t(o.Kc) * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("bev 3x3 conv_seg: weight copy failed");
      return DDP_E_LAUNCH;
    }
    DDP_TRY(launch_pack_conv3x3_scaled(w->head_w, nullptr, o.bins_wpack, o.Kc, 256, st));
    if (o.b3) {
      DDP_TRY(launch_split_weights(o.bins_wpack, 2304, 256, 2304, o.bins_wsplit, st));
      DDP_TRY(launch_build_stages(o.bins_wsplit, size_t(256) * 2304, 2304, 256, 0, 1, 72, 0, 2, 1, 0, o.bins_stream, st));
    }
  }
  if (o.nbins) {
    // binned depth head: conv_depth (n_bins,256,3,3) tap-major, output rows zero-padded to the stream GEMM's 256 columns; bias and
    // bin centres zero-padded likewise
    if (hipMemsetAsync(o.bins_wpack, 0, size_t(256) * 2304 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(o.bins_bias, 0, 256 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(o.bins_tab, 0, DDP_MAX_DEPTH_BINS * sizeof(float), st) != hipSuccess ||
        hipMemcpyAsync(o.bins_bias, w->head_b, size_t(o.nbins) * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(o.bins_tab, w->depth_bins, size_t(o.nbins) * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("depth bins: weight copy failed");
      return DDP_E_LAUNCH;
    }
    DDP_TRY(launch_pack_conv3x3_scaled(w->head_w, nullptr, o.bins_wpack, o.nbins, 256, st));
    if (o.b3) {   // the implicit 3x3 GEMM's 72 stage images (as FCNHeadWithTime's convolutions)
      DDP_TRY(launch_split_weights(o.bins_wpack, 2304, 256, 2304, o.bins_wsplit, st));
      DDP_TRY(launch_build_stages(o.bins_wsplit, size_t(256) * 2304, 2304, 256, 0, 1, 72, 0, 2, 1, 0, o.bins_stream, st));
    }
  }
  for (int l = 0; l < o.L; ++l) {
    const ddp_layer_weights& lw = w->layers[l];
    DDP_TRY(launch_pack_rows(lw.sampling_offsets_w, 64, lw.attention_weights_w, 32, o.wcat[l], 256, st));
    DDP_TRY(launch_pack_rows(lw.sampling_offsets_b, 64, lw.attention_weights_b, 32, o.bcat[l], 1, st));
  }
  if (o.b3) {
    auto wr = [](const SplitW& w) { return const_cast<unsigned short*>(w.p); };
    DDP_TRY(launch_split_weights(o.wx, o.Cx, 256, o.Cx, wr(o.wp_x), st));
    if (c->task != DDP_TASK_DEPTH) DDP_TRY(launch_split_weights(o.wm, 256, 256, 256, wr(o.wp_m), st));
    if (c->task == DDP_TASK_DEPTH) DDP_TRY(launch_split_weights(o.wtap, 256, 9, 256, wr(o.wp_head), st));
    else if (!o.seg3) DDP_TRY(launch_split_weights(w->head_w, 256, o.Kc, 256, wr(o.wp_head), st));
    for (int l = 0; l < o.L; ++l) {
      const ddp_layer_weights& lw = w->layers[l];
      DDP_TRY(launch_split_weights(lw.value_proj_w, 256, 256, 256, wr(o.wp_v[l]), st));
      DDP_TRY(launch_split_weights(o.wcat[l], 256, 96, 256, wr(o.wp_cat[l]), st));
      DDP_TRY(launch_split_weights(lw.output_proj_w, 256, 256, 256, wr(o.wp_o[l]), st));
      DDP_TRY(launch_split_weights(lw.ffn0_w, 256, DDP_FFN, 256, wr(o.wp_f0[l]), st));
      DDP_TRY(launch_split_weights(lw.ffn1_w, DDP_FFN, 256, DDP_FFN, wr(o.wp_f1[l]), st));
    }
    if (c->task == DDP_TASK_SEG) {
      // seg tail: conv_seg as tall stages of 64 classes, bias table; fused tail (k_layer MODE 4): [conv_seg: 2 tall per 64 classes]
      // [layer 0's Wv: 8 tall][Wcat: 2 tall + 1 split-K]
      const int nch = (o.Kc + 63) / 64;
      DDP_TRY(launch_build_stages(o.wp_head.p, o.wp_head.comp_stride, 256, o.Kc, 1, nch, 2, 0, 0, 1, 2, o.tail_stream, st));
      DDP_TRY(bias_table(o.tail_bias, {{0, w->head_b, o.Kc}}, "seg tail", st));
      DDP_TRY(launch_build_stages(o.wp_head.p, o.wp_head.comp_stride, 256, o.Kc, 1, nch, 2, 0, 0, 1, 2, o.tail4_stream, st));
      DDP_TRY(build_proj_images(o, 0, o.tail4_stream, 2 * nch, st));
      DDP_TRY(bias_table(o.tail4_bias, {{0, w->head_b, o.Kc}, {DDP_FFN, w->layers[0].value_proj_b, 256}}, "fused tail", st));
      // T = LUT . W_m^T: the noisy-map half of the concat-conv applied to each of the K + 1 possible x0 vectors (exact
      // fp32 products: the f32-input MFMA GEMM)
      DDP_TRY(launch_linear(o.lut, 256, false, o.wm, 256, nullptr, nullptr, 0, 0, 0, o.tlut, 256, o.Kc + 1, 256, 256, 0, st));
    }
    // step prologue: [W_m: 8 wide stages][layer 0's Wv: 8 tall][layer 0's Wcat: 2 tall + 1 split-K]
    // (depth has no W_m GEMM - one input channel - and uses images 8..18 only: k_layer MODE 3)
    if (c->task != DDP_TASK_DEPTH)
      DDP_TRY(launch_build_stages(o.wp_m.p, o.wp_m.comp_stride, 256, 256, 0, 1, 8, 0, 2, 1, 0, o.pro_stream, st));
    DDP_TRY(build_proj_images(o, 0, o.pro_stream, 8, st));
    DDP_TRY(bias_table(o.pro_bias, {{DDP_FFN, w->layers[0].value_proj_b, 256}}, "prologue", st));
    if (o.head7_stream) {               // first step's head from NCHW (k_layer MODE 7): [W_m: 8 wide][W_x: 8 wide][layer 0's Wv, Wcat as above]
      DDP_TRY(launch_build_stages(o.wp_m.p, o.wp_m.comp_stride, 256, 256, 0, 1, 8, 0, 2, 1, 0, o.head7_stream, st));
      DDP_TRY(launch_build_stages(o.wp_x.p, o.wp_x.comp_stride, 256, 256, 0, 1, 8, 8, 2, 1, 0, o.head7_stream, st));
      if (hipMemcpyAsync(o.head7_stream + size_t(16) * 48 * 1024, o.pro_stream + size_t(8) * 48 * 1024, size_t(11) * 48 * 1024,
                         hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("first-step head stream copy failed");
        return DDP_E_LAUNCH;
      }
    }
    // layer-kernel weight streams: [Wo: 8 wide stages][16 x (fc1 tall, tall, fc2 wide, wide)][next Wv: 8 tall][next Wcat: 2 tall + 1 split-K]
    for (int l = 0; l < o.L; ++l) {
      const ddp_layer_weights& lw = w->layers[l];
      unsigned char* sp = o.wstream[l];
      DDP_TRY(launch_build_stages(o.wp_o[l].p, o.wp_o[l].comp_stride, 256, 256, 0, 1, 8, 0, 2, 1, 0, sp, st));
      DDP_TRY(launch_build_stages(o.wp_f0[l].p, o.wp_f0[l].comp_stride, 256, DDP_FFN, 1, 16, 2, 8, 0, 1, 4, sp, st));
      DDP_TRY(launch_build_stages(o.wp_f1[l].p, o.wp_f1[l].comp_stride, DDP_FFN, 256, 0, 1, 32, 10, 4, 1, 0, sp, st));
      DDP_TRY(bias_table(o.bias_ext[l], {{0, lw.ffn0_b, DDP_FFN}}, "layer", st));
      if (l + 1 < o.L) {
        DDP_TRY(build_proj_images(o, l + 1, sp, 72, st));
        if (hipMemcpyAsync(o.bias_ext[l] + DDP_FFN, w->layers[l + 1].value_proj_b, 256 * sizeof(float), hipMemcpyDeviceToDevice, st) !=
            hipSuccess) {
          set_error("bias table copy failed");
          return DDP_E_LAUNCH;
        }
      }
    }
    if (o.lt_stream && c->task != DDP_TASK_SEG && !o.seg3) {
      // last layer + bev / depth tail (k_layer MODE 8 / 9): [layer L-1: 72 stages][the head convolution: 2 tall stages of <= 32 rows]
      // (conv_seg of the bev head; the nine taps of the 3x3 conv_depth as nine output rows).  Bias table: fc1's; tail_bias: conv_seg's
      // (depth: zeros - conv_depth's bias is added once per pixel by k_depth_update).
      const size_t sb = size_t(48) * 1024;
      const int rows = c->task == DDP_TASK_DEPTH ? 9 : o.Kc;
      DDP_TRY(launch_build_stages(o.wp_head.p, o.wp_head.comp_stride, 256, rows, 1, 1, 2, 0, 0, 1, 2, o.tail_stream, st));
      DDP_TRY(bias_table(o.tail_bias, {{0, c->task == DDP_TASK_BEV ? w->head_b : nullptr, o.Kc}}, "head tail", st));
      if (hipMemcpyAsync(o.lt_stream, o.wstream[o.L - 1], 72 * sb, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(o.lt_stream + 72 * sb, o.tail_stream, 2 * sb, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("layer + tail stream copy failed");
        return DDP_E_LAUNCH;
      }
      DDP_TRY(bias_table(o.lt_bias, {{0, w->layers[o.L - 1].ffn0_b, DDP_FFN}}, "layer + tail", st));
    }
    if (o.wvs) {
      // depth chain: the rank-1 terms of the GEMM-free step head, W_v0 w_m and W_cat0 w_m (fp32 dot products)
      DDP_TRY(launch_matvec(w->layers[0].value_proj_w, nullptr, o.wm, o.wvs, 256, 256, 1, 256, 256, 0, 0, st));
      DDP_TRY(launch_matvec(o.wcat[0], nullptr, o.wm, o.wvs + 256, 256, 96, 1, 256, 96, 0, 0, st));
    }
    if (o.lut64) {
      // bev u chain: the 2^K x0 vectors of a pixel and their images under W_m (exact fp32 products, as the seg table)
      DDP_TRY(launch_build_bev_lut(w->embedding, o.lut64, o.Kc, c->bit_scale, st));
      DDP_TRY(launch_linear(o.lut64, 256, false, o.wm, 256, nullptr, nullptr, 0, 0, 0, o.tlut, 256, 1 << o.Kc, 256, 256, 0, st));
    }
    if (o.lt_stream && c->task == DDP_TASK_SEG) {
      // last layer + tail (k_layer MODE 6): the images do not depend on the step, so ONE concatenated stream serves every step -
      // [layer L-1: Wo 8 wide, 16 x (fc1 2 tall, fc2 2 wide)][conv_seg 2 tall per 64 classes][layer 0's Wv 8 tall][Wcat 2 tall +
      // 1 split-K]; after the last step the kernel wraps behind conv_seg.  Bias table: fc1's | layer 0's value_proj bias.
      const int nch = (o.Kc + 63) / 64;
      const size_t sb = size_t(48) * 1024;
      if (hipMemcpyAsync(o.lt_stream, o.wstream[o.L - 1], 72 * sb, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(o.lt_stream + 72 * sb, o.tail4_stream, size_t(2 * nch + 11) * sb, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        set_error("layer + tail stream copy failed");
        return DDP_E_LAUNCH;
      }
      DDP_TRY(bias_table(o.lt_bias, {{0, w->layers[o.L - 1].ffn0_b, DDP_FFN}, {DDP_FFN, w->layers[0].value_proj_b, 256}}, "layer + tail",
                         st));
    }
  }
  return DDP_OK;
}

// publish a row-major (M,256) activation as the encoder input: fp32 fragment-major q, or SB in bf16x3 mode
int publish_q(const Layout& o, const float* row_major, hipStream_t st) {
  if (o.b3 && !o.fused_layer) return launch_row_to_sb(row_major, 256, o.q_sb, int(o.M), 256, st);
  return launch_row_to_blk(row_major, o.q, int(o.M), st);     // the layer kernels (and the fp32 engine) take q as fp32 fragments
}

// the 3x3 head convolution (padding 1, bias) of the encoder output on the head grid into o.bins_logits -> (layout, ld) as
// DepthBinsArgs / BevSeg3Args read it.  bf16x3: the implicit 3x3 GEMM of the stream engine (k_layer MODE 5, 72 stages, bias in the
// epilogue, no activation) on the fp32 fragment-major layer output; fp32 engine: the exact-product GEMM as nine shifted GEMMs over
// the zero-bordered grid, accumulated in place.
int conv3x3_head(const Layout& o, int n_out, int* layout, int* ld, hipStream_t st) {
  const int M = int(o.M);
  if (o.b3) {
    if (!o.fused_layer) {     // the tile-GEMM layers leave their output as SB only
      DDP_TRY(launch_sb_to_row(o.q_sb, o.s, M, 256, st));
      DDP_TRY(launch_row_to_blk(o.s, o.q, M, st));
    }
    SgemmProblem pr{};
    pr.A = o.q;
    pr.out = o.bins_logits;
    pr.stream = o.bins_stream;
    pr.M = M;
    pr.ns = 72;
    pr.conv_h = o.hh;
    pr.conv_w = o.wh;
    pr.bias = o.bins_bias;
    prof_begin(TAG_HEAD, st);
    DDP_TRY(launch_b3_sgemm(&pr, 1, 0, 1, st));
    prof_end(TAG_HEAD, st);
    *layout = 0;
    *ld = 256;
  } else {
    DDP_TRY(launch_blk_to_pad(o.q, o.bins_in, o.R, o.hh, o.wh, o.bins_guard, st));
    const int rows = o.R * (o.hh + 2) * (o.wh + 2);
    for (int t = 0; t < 9; ++t) {
      const int off = (t / 3 - 1) * (o.wh + 2) + (t % 3 - 1);
      DDP_TRY(launch_linear(o.bins_in + size_t(o.bins_guard + off) * 256, 256, false, o.bins_wpack + t * 256, 2304,
                            t == 0 ? o.bins_bias : nullptr, t == 0 ? nullptr : o.bins_logits, o.bins_ld, 0, 0, o.bins_logits,
                            o.bins_ld, rows, n_out, 256, 0, st));
    }
    *layout = 1;
    *ld = o.bins_ld;
  }
  return DDP_OK;
}

// binned depth head (decode_head.py:233-250) on the encoder output: conv_depth to n_bins channels (conv3x3_head), then
// k_depth_bins -> the metric prediction `pred` (M)
int depth_bins_head(const ddp_cfg* c, const Layout& o, float* pred, hipStream_t st) {
  DepthBinsArgs a;
  a.bins = o.bins_tab;
  a.n_bins = o.nbins;
  a.norm = c->depth_norm;
  a.pred = pred;
  a.R = o.R;
  a.h = o.h;
  a.w = o.w;
  a.logits = o.bins_logits;
  DDP_TRY(conv3x3_head(o, o.nbins, &a.layout, &a.ld, st));
  return launch_depth_bins(a, st);
}

// the 3x3 conv_seg of the bev head on the encoder output (fp32 fragment-major o.q), then k_bev_seg3: the step's probabilities set /
// accumulated in o.prob; `code` (u chain, K_cls <= 8): the step's x0 code bytes; `logits_out`: rows of 32 for k_bev_update
int bev_seg3_head(const ddp_cfg* c, const Layout& o, bool first, unsigned char* code, float* logits_out, hipStream_t st) {
  BevSeg3Args a{};
  a.logits = o.bins_logits;
  DDP_TRY(conv3x3_head(o, o.Kc, &a.layout, &a.ld, st));
  a.num_classes = o.Kc;
  a.prob = o.prob;
  a.first = first;
  a.code = code;
  a.logits_out = logits_out;
  a.threshold = c->threshold;
  a.R = o.R;
  a.hh = o.hh;
  a.wh = o.wh;
  prof_begin(TAG_HEAD, st);          // (the route's witness: a second TAG_HEAD record per step behind the convolution's)
  const int rc = launch_bev_seg3(a, st);
  prof_end(TAG_HEAD, st);
  return rc;
}

// eps of the regression head's depth_pred: the HEAD's depth range (decode_head.py:258-266; 0 / 0 = the depther's)
float depth_head_eps(const ddp_cfg* c) {
  const bool own = c->head_min_depth != 0.f || c->head_max_depth != 0.f;
  const float lo = own ? c->head_min_depth : c->min_depth, hi = own ? c->head_max_depth : c->max_depth;
  const bool su = (c->flags & DDP_FLAG_DEPTH_SCALE_UP) != 0;
  return (c->flags & DDP_FLAG_DEPTH_NO_EPS) ? (su ? 1.0f : 0.0f) : (su ? hi : lo);
}

// layer 0's value / sampling projections of the fragment-major Q (k_layer MODE 3 on the step prologue's 11 projection images), value
// map to v_out.  The depth step head also sets the concat-conv fields (res, wm, dvec) and the fused update (upd).
L0ProjLaunch l0proj_launch(const Layout& o, float* Q, int M, float* v_out) {
  L0ProjLaunch pj{};
  pj.Q = Q;
  pj.stream = o.pro_stream + size_t(8) * 48 * 1024;
  pj.bias_ext = o.pro_bias;
  pj.M = M;
  pj.v_out = v_out;
  pj.samp_out = o.samp;
  pj.py = o.py[0];
  pj.px = o.px[0];
  pj.n_tok = o.Nh;
  pj.w = o.wh;
  return pj;
}

// k_depth_update (decode_head.py:252-262): taps == nullptr when pred already holds the binned head's prediction
DepthUpdateArgs depth_update_args(const ddp_cfg* c, const ddp_weights* w, const Layout& o, const float* taps, float* depth_t,
                                  float* pred, const ddp_step& stp) {
  DepthUpdateArgs a{};
  a.taps = taps;
  a.bias_ptr = w->head_b;
  a.depth_t = depth_t;
  a.pred = pred;
  a.B_r = o.R;
  a.h = o.h;
  a.w = o.w;
  a.min_depth = c->min_depth;
  a.max_depth = c->max_depth;
  a.bit_scale = c->bit_scale;
  a.scale_up = (c->flags & DDP_FLAG_DEPTH_SCALE_UP) ? 1 : 0;
  a.eps_depth = depth_head_eps(c);
  a.st = stp;
  a.hint = static_cast<const float*>(o.hint_rows);   // (nullptr without DDP_FLAG_X0_HINTS)
  return a;
}

// k_bev_update on the head GEMM's logits: probabilities set (first) or accumulated; mask == nullptr: no DDIM update
BevUpdateArgs bev_update_args(const ddp_cfg* c, const ddp_weights* w, const Layout& o, float* mask, bool first, const ddp_step& stp) {
  BevUpdateArgs a{};
  a.logits = o.logits;
  a.num_classes = o.Kc;
  a.emb = w->embedding;
  a.mask = mask;
  a.prob = o.prob;
  a.first = first;
  a.R = o.R;
  a.g = bev_geom(c);
  a.threshold = c->threshold;
  a.bit_scale = c->bit_scale;
  a.st = stp;
  return a;
}

// k_seg_update without DDPM step noise or x0 trace (the sampler adds them where it has them)
SegUpdateArgs seg_update_args(const float* logits, int ldl, int num_classes, const float* lut, float* mask, float* prob, int prob_mode,
                              int sampler, const ddp_step& stp, int rows) {
  SegUpdateArgs a{};
  a.logits = logits;
  a.ldl = ldl;
  a.num_classes = num_classes;
  a.lut = lut;
  a.mask = mask;
  a.prob = prob;
  a.prob_mode = prob_mode;
  a.sampler = sampler;
  a.st = stp;
  a.rows = rows;
  return a;
}

// the x0 trace of seg step s.  FORCE_X0: [0] = the caller's decisions (read), [1] = the step's own argmax (written); RECORD_X0
// alone: [0] written; STEP_RECORD: the same (K, M) record, in the step-record buffer
// DDP_FLAG_X0_HINTS: the hint rows take the place of the forced decisions - the same buffer at every step, with the keep-the-argmax
// reading of a value >= num_classes - and the record is the one of the cfg without the flag (the model's own argmax)
struct X0Trace {
  unsigned char* idx = nullptr;
  const unsigned char* force = nullptr;
  int keep = 0;
};
X0Trace x0_trace_of(const ddp_cfg* c, const Layout& o, int s) {
  X0Trace t;
  if (c->flags & DDP_FLAG_X0_HINTS) {
    t.force = static_cast<const unsigned char*>(o.hint_rows);
    t.keep = 1;
    if (c->flags & (DDP_FLAG_RECORD_X0 | DDP_FLAG_STEP_RECORD)) t.idx = o.x0_trace + size_t(s) * o.M;
    return t;
  }
  if (c->flags & DDP_FLAG_FORCE_X0) {
    t.force = o.x0_trace + size_t(s) * o.M;
    t.idx = o.x0_trace + size_t(o.K + s) * o.M;
  } else if (c->flags & (DDP_FLAG_RECORD_X0 | DDP_FLAG_STEP_RECORD)) {
    t.idx = o.x0_trace + size_t(s) * o.M;
  }
  return t;
}

// the head convolution as a GEMM of the encoder output into o.logits: conv_seg (seg: rows of ldl, bev: of 32) or the nine taps of
// the 3x3 conv_depth (rows of 32, no bias: k_depth_update adds it once per pixel)
int head_gemm(const ddp_cfg* c, const ddp_weights* w, const Layout& o, hipStream_t st) {
  const bool depth = c->task == DDP_TASK_DEPTH;
  const int M = int(o.M), ld = c->task == DDP_TASK_SEG ? o.ldl : 32, n = depth ? 9 : o.Kc;
  const float* bias = depth ? nullptr : w->head_b;
  if (o.b3) return launch_b3_linear(o.q_sb, o.wp_head, bias, nullptr, 0, 0, 0, o.logits, ld, M, n, 256, st, TAG_HEAD);
  return launch_linear(o.q, 256, true, depth ? o.wtap : w->head_w, 256, bias, nullptr, 0, 0, 0, o.logits, ld, M, n, 256, 0, st,
                       TAG_HEAD);
}

// DetrTransformerEncoder over the fragment-major q (in/out); aff (L,512) = norms.1 affine x FiLM
// `tail` (seg, u chain): the step's tail is fused into the LAST layer's kernel (k_layer MODE 6) - the caller launches no tail
int encoder_forward(const ddp_weights* w, const Layout& o, const float* aff, hipStream_t st, bool l0_projected = false,
                    bool sb_out = true, const TailLaunch* tail = nullptr, bool depth_chain = false) {
  const int M = int(o.M);
  if (o.b3) {
    // same dataflow on the bf16 matrix cores: q / q1 travel only as SB (operands AND residuals: the three pieces
    // of an element sum to its fp32 value exactly)
    const bool fused = o.fused_layer;
    for (int l = 0; l < o.L; ++l) {
      const ddp_layer_weights& lw = w->layers[l];
      // later layers: emitted by the previous layer kernel; layer 0: by the step prologue kernel when that ran
      bool own_proj = !fused || (l == 0 && !l0_projected);
      if (own_proj && fused) {
        // layer 0 of a path without a fused step head (bev after its grid resampling, ddp_head_forward): the value /
        // sampling projections of the SB q as ONE launch of the layer kernel's P3 (k_layer MODE 3), padded value map out
        DDP_TRY(launch_b3_l0proj(l0proj_launch(o, o.q, M, o.vpad), st));
        own_proj = false;
      }
      if (own_proj) {
        DDP_TRY(launch_b3_linear(o.q_sb, o.wp_v[l], lw.value_proj_b, nullptr, 0, 0, 0, o.v, 256, M, 256, 256, st, TAG_VALUE));
        DDP_TRY(launch_b3_linear_samp(o.q_sb, o.wp_cat[l], o.py[l], o.px[l], o.Nh, o.wh, o.samp, M, st));
      }
      // a row-major GEMM leaves a plain value map; the layer / prologue kernels write it zero-padded
      // (the LDS gather feeds the layer kernel only: its output is fp32 in the accumulator layout - o.q1 is free on this path)
      if (own_proj) DDP_TRY(launch_msda_gather_sb(o.v, o.samp, o.s_sb, M, o.Nh, o.hh, o.wh, st));
      else DDP_TRY(launch_msda_gather_sb_pad(o.vpad, o.samp, o.s_sb, DDP_S_F32 ? o.q1 : nullptr, M, o.Nh, o.hh, o.wh, o.py[l], o.px[l],
                                             o.guess_zero, st));
      const float* a = aff + size_t(l) * 512;
      if (fused) {
        // output_proj + LN0 + FFN + LN1 + FiLM + the next layer's value / sampling projections: one persistent kernel
        LayerLaunch ll;
        ll.S = o.s_sb;
        ll.Sf = DDP_S_F32 ? o.q1 : nullptr;
        ll.Q = o.q;
        ll.Q_sb = (sb_out && l + 1 == o.L) ? o.q_sb : nullptr;      // a head GEMM after the encoder reads SB
        ll.stream = o.wstream[l];
        ll.bias_ext = o.bias_ext[l];
        ll.bo = lw.output_proj_b;
        ll.ga0 = lw.norm0_w;
        ll.be0 = lw.norm0_b;
        ll.b2 = lw.ffn1_b;
        ll.ga1 = a;
        ll.be1 = a + 256;
        ll.M = M;
        ll.has_next = l + 1 < o.L;
        ll.v_out = o.vpad;
        ll.samp_out = o.samp;
        ll.py = ll.has_next ? o.py[l + 1] : nullptr;
        ll.px = ll.has_next ? o.px[l + 1] : nullptr;
        ll.n_tok = o.Nh;
        ll.w = o.wh;
        // depth chain: q of the step never exists - layer 0 forms its residual from xproj and the noisy depth (k_layer MODE 10)
        ll.res_f = (depth_chain && l == 0) ? o.xproj_f : nullptr;
        ll.wm = o.wm;
        ll.dvec = o.mask;
        if (tail && l + 1 == o.L) DDP_TRY(launch_b3_layer_tail(ll, *tail, o.lt_stream, o.lt_bias, o.tail_bias, st));
        else DDP_TRY(launch_b3_layer(ll, st));
      } else {
        DDP_TRY(launch_b3_linear_res_ln(o.s_sb, o.wp_o[l], lw.output_proj_b, nullptr, o.q_sb, lw.norm0_w, lw.norm0_b, nullptr,
                                        o.q1_sb, M, 256, st, TAG_OUTPROJ_LN));
        DDP_TRY(launch_b3_linear_sb(o.q1_sb, o.wp_f0[l], lw.ffn0_b, nullptr, 0, 0, 0, o.h_sb, nullptr, M, DDP_FFN, 256, 1, st,
                                    TAG_FC1));
        DDP_TRY(launch_b3_linear_res_ln(o.h_sb, o.wp_f1[l], lw.ffn1_b, nullptr, o.q1_sb, a, a + 256, nullptr, o.q_sb, M,
                                        DDP_FFN, st, TAG_FC2_LN));
      }
    }
    return DDP_OK;
  }
  for (int l = 0; l < o.L; ++l) {
    const ddp_layer_weights& lw = w->layers[l];
    // value / sampling projections (multi_scale_deform_attn.py:313-328)
    DDP_TRY(launch_linear(o.q, 256, true, lw.value_proj_w, 256, lw.value_proj_b, nullptr, 0, 0, 0, o.v, 256, M, 256, 256, 0,
                          st, TAG_VALUE));
    DDP_TRY(launch_linear_samp(o.q, o.wcat[l], o.py[l], o.px[l], o.Nh, o.wh, o.samp, M, st));
    // bilinear gather + weighted sum (:94-151)
    DDP_TRY(launch_msda_gather(o.v, o.samp, o.s, M, o.Nh, o.hh, o.wh, st));
    // output_proj + identity, LayerNorm (:352-358; utils/transformer.py:390-392)
    DDP_TRY(launch_linear_res_ln_blk(o.s, 256, false, lw.output_proj_w, 256, lw.output_proj_b, o.q, lw.norm0_w, lw.norm0_b,
                                     o.q1, M, 256, st));
    // FFN + identity, LayerNorm, FiLM (mmcv FFN :269-280; utils/transformer.py:413-417)
    DDP_TRY(launch_linear_blk(o.q1, 256, true, lw.ffn0_w, 256, lw.ffn0_b, nullptr, 0, 0, 0, o.hbuf, M, DDP_FFN, 256, 1, st));
    const float* a = aff + size_t(l) * 512;
    DDP_TRY(launch_linear_res_ln_blk(o.hbuf, DDP_FFN, true, lw.ffn1_w, DDP_FFN, lw.ffn1_b, o.q1, a, a + 256, o.q, M, DDP_FFN,
                                     st));
  }
  return DDP_OK;
}

// Which launches a ddp_sample call runs, resolved once from (cfg, Layout).  The conditions lean on facts established elsewhere:
// validate() makes the head grid equal (h, w) for seg and depth; fused_pro implies fused_layer implies b3; carve gives
// head7_stream, lt_stream, lut64 and rvpad only to the configs whose path can use them.
struct Plan {
  // seg + DDIM, one noisy map per image, 256 feature channels (head7_stream): the first step's head reads the caller's NCHW x and
  // start noise directly (k_layer MODE 7) and writes xproj itself - no NCHW -> SB conversions, no x-projection GEMM
  bool head7 = false;
  // seg + DDIM on the layer kernel: conv_seg, argmax, softmax accumulation, x0 LUT and the DDIM update run as the "tail" mode of
  // the layer kernel, which leaves m_{t_next} as the SB operand of the next step's concat-conv
  bool seg_tail = false;
  // seg tail + step prologue: the noisy map enters the loop only through u = W_m . m_t and its update is affine in (m_t, x0) with
  // x0 one of K + 1 table rows, so steps 1 .. K-1 run NO concat-conv GEMM and keep no 256-channel map: the tail of step s updates
  // u (u' = ua u + uc (W_m . LUT)[argmax]) and is at the same time the head of step s + 1 (q = W_x x + b + u', layer 0's
  // projections): k_layer MODE 4.  Step 0 starts from the noise with the step-prologue kernel, the last step's tail has nothing
  // to update.
  bool u_chain = false;
  // u chain: the step's tail runs inside the LAST layer's kernel (k_layer MODE 6) - the layer output never leaves the registers
  bool lt_fused = false;
  // seg + DDPM with DDP_FLAG_DDPM_CHAIN on the fused prologue path: head7 / seg_tail / u_chain / lt_fused under the ddim sampler's
  // conditions.  The ddpm update is u' = ua' u + uc' T[argmax] + std (W_m eps) with ua' = ((1 - c) / alpha) alpha', uc' = c alpha'
  // (ddp.py:274-283 under W_m): a noise-adding step runs the pre-pass U <- ua' U + std (E W_m^T) (k_u_noise) in front of its tail,
  // which then runs with (ua, uc) = (1, uc'); a step without noise runs the tail with (ua', uc'); the last step updates nothing
  bool ddpm_chain = false;
  // depth (regression head) on the fused path: the step's last layer runs with the nine taps of conv_depth as its tail (k_layer
  // MODE 9) - no head GEMM, no SB copy of the layer output - and the step's update runs in front of the next step's head.  (The
  // binned head takes the route of DDP_FLAG_UNFUSED_TAIL: MODE 3 step head, a plain last layer, conv_depth + k_depth_bins,
  // k_depth_update.)
  bool depth_lt = false;
  // depth chain (one noisy map per image - rvpad fits -, >= 2 layers): the step head without a GEMM.  Loop invariant, once per
  // sample: xproj fragment-major (layer 0's residual operand), rvpad = W_v0 xproj + b_v0 as a padded map (layer 0's projection
  // kernel run on xproj itself), rs0 = W_cat0 xproj; per step k_depth_head adds the rank-1 terms in the noisy depth (and runs the
  // previous step's update)
  bool depth_chain = false;
  // bev (<= 8 classes: lut64) on the fused path: the last layer carries conv_seg as its tail (k_layer MODE 8), and the u chain runs:
  // the grid transform and the concat-conv are linear, so resample(W_x x + b) is hoisted out of the loop (rx, row-major in o.s: the
  // fused layers never touch that buffer), the noisy map is carried as u = W_m m (o.feat0, row-major at the map size) and follows
  // the DDIM update through the 2^K-row table T = LUT64 . W_m^T - per step: u update, q = rx + resample(u), layer 0's projections;
  // no GEMM at the map size after u_0
  bool bev_chain = false;
  // bev with the 3x3 conv_seg (cfg->bev_seg_kernel == 3): nine taps x K_cls columns do not fit the two tall stages of the MODE 8 tail, so
  // the last layer runs as a plain layer and conv_seg follows as the implicit 3x3 GEMM (the fp32 engine: nine shifted GEMMs) +
  // k_bev_seg3.  With bev_chain the u chain is kept around it (k_bev_seg3 writes the codes); otherwise k_bev_seg3 feeds k_bev_update
  bool bev_seg3 = false;
};

Plan plan_of(const ddp_cfg* c, const Layout& o) {
  const bool seg_ddim = c->task == DDP_TASK_SEG && c->sampler == DDP_SAMPLER_DDIM;
  // the step's last layer with the head convolution as its tail (k_layer MODE 6 / 8 / 9)
  const bool lt = o.fused_pro && o.lt_stream && !(c->flags & DDP_FLAG_UNFUSED_TAIL);
  Plan p;
  p.ddpm_chain = c->task == DDP_TASK_SEG && c->sampler == DDP_SAMPLER_DDPM && (c->flags & DDP_FLAG_DDPM_CHAIN) && o.fused_pro;
  const bool seg_chain = seg_ddim || p.ddpm_chain;
  p.head7 = seg_chain && o.fused_pro && o.r == 1 && o.head7_stream && !(c->flags & DDP_FLAG_SB_HEAD) && !((size_t(o.M) * 256) >> 32);
  p.seg_tail = seg_chain && o.fused_layer;
  p.u_chain = p.seg_tail && o.fused_pro;
  p.lt_fused = p.u_chain && lt;
  p.depth_lt = c->task == DDP_TASK_DEPTH && lt && !o.nbins;
  p.depth_chain = p.depth_lt && o.rvpad && o.L >= 2;
  // (the 1x1 head needs the last layer + tail stream; the 3x3 head keeps the chain around a plain last layer and has none)
  p.bev_chain = c->task == DDP_TASK_BEV && o.lut64 && (o.seg3 ? o.fused_pro && !(c->flags & DDP_FLAG_UNFUSED_TAIL) : lt);
  p.bev_seg3 = o.seg3;
  return p;
}

// The launches DDP_FLAG_STEP_RECORD adds carry the profiler tag no launch of ddp_sample otherwise uses (TAG_GENERIC), so the launch
// records count them: tests/test_step_record_gpu.py asserts the figures the header states.  Usage: prof_begin(TAG_GENERIC, st) in
// front of the launch, `return recorded(launch_...(...), st)` behind it
inline int recorded(int rc, hipStream_t st) {
  prof_end(TAG_GENERIC, st);
  return rc;
}

// DDP_FLAG_STEP_RECORD: the disagreement map from the finished record and the output the sampler just wrote (one launch, last)
// DDP_FLAG_SEEDED_NOISE: d_noise is the device key; the start noise of the call goes to `buf` (B images of `per_image` floats, NCHW),
// which every consumer then reads in place of the caller's tensor (one launch, first)
int seeded_start_noise(const uint32_t* key, float* buf, int B, size_t per_image, hipStream_t st) {
  prof_begin(TAG_GENERIC, st);
  return recorded(launch_noise_fill_nchw(key, buf, B, per_image, st), st);
}

// (`threshold` is read for bev only; ddp_sample passes cfg->threshold, the FCN loop 0)
int step_disagreement(const ddp_cfg* c, const CallerRegions& o, float threshold, const float* d_out, hipStream_t st) {
  if (!o.step_rec) return DDP_OK;
  prof_begin(TAG_GENERIC, st);
  StepDisagreementArgs a{};
  a.rec = o.step_rec;
  a.out = d_out;
  a.map = o.step_map;
  a.task = c->task;
  a.B = c->batch;
  a.r = c->randsteps;
  a.K = c->timesteps;
  a.N = c->head_h * c->head_w;
  a.num_classes = c->task == DDP_TASK_DEPTH ? 1 : c->num_classes;
  a.threshold = threshold;
  return recorded(launch_step_disagreement(a, st), st);
}

// DDPM: the noise added after step s, token-major (B * r * N, 256) in `snoise`.  DDP_FLAG_SEEDED_NOISE (key): generated that way - no
// NCHW tensor, no transpose; else the transpose of slice s of the caller's (K, B, r, 256, h, w) tensor
int stage_step_noise(const uint32_t* key, const float* d_step_noise, float* snoise, int B, int r, int N, int s, hipStream_t st) {
  if (key) {
    prof_begin(TAG_GENERIC, st);
    return recorded(launch_noise_fill_tok(key, snoise, B, r, N, s, st), st);
  }
  return launch_nchw_to_tok(d_step_noise + size_t(s) * B * r * N * 256, snoise, B * r, 256, N, st);
}

// the segmentation sampler after the xproj hoist: noise staging, K steps, reduction
int sample_seg(const ddp_cfg* c, const ddp_weights* w, const ddp_step* steps, const Plan& p, const Layout& o, const float* d_x,
               const float* d_noise, const float* d_step_noise, const uint32_t* key, float* d_out, hipStream_t st) {
  const int M = int(o.M), M0 = int(o.M0);
  if (p.head7) {
    // (the first step's head reads d_noise itself)
  } else if (p.seg_tail) {
    DDP_TRY(launch_nchw_to_sb(d_noise, o.in_sb, o.R, 256, o.N, st));    // the noisy map only ever exists as SB on this path
  } else {
    DDP_TRY(launch_nchw_to_tok(d_noise, o.mask, o.R, 256, o.N, st));
  }
  for (int s = 0; s < o.K; ++s) {
    const ddp_step& sp = steps[s];
    const float* aff = o.aff + size_t(s) * o.L * 512;
    // feat = transform(cat[x, mask_t])
    if (o.b3 && !p.seg_tail) DDP_TRY(launch_row_to_sb(o.mask, 256, o.in_sb, M0, 256, st));
    if (p.u_chain && s > 0) {
      // the previous step's fused tail already wrote q (SB) and layer 0's value map / sampling table
    } else if (o.fused_pro) {
      // q = W_m m_t + xproj -> SB, layer 0's value / sampling projections: one persistent kernel
      PrologueLaunch pl{};
      pl.mask_sb = o.in_sb;
      pl.Q = o.q;
      pl.stream = o.pro_stream;
      pl.bias_ext = o.pro_bias;
      pl.res = o.xproj;
      pl.res_rn = o.r > 1 ? o.r * o.N : 0;
      pl.ubuf = p.u_chain && o.K > 1 ? o.ubuf : nullptr;
      pl.M = M0;
      pl.v_out = o.vpad;
      pl.samp_out = o.samp;
      pl.py = o.py[0];
      pl.px = o.px[0];
      pl.n_tok = o.Nh;
      pl.w = o.wh;
      if (p.head7) {
        pl.mask_sb = nullptr;
        pl.res_frag = 1;
        pl.stream = o.head7_stream;
        DDP_TRY(launch_b3_head_nchw(pl, d_noise, d_x, w->transform_b, st));
      } else {
        DDP_TRY(launch_b3_prologue(pl, st));
      }
    } else if (o.b3) {
      // separate concat-conv GEMM: SB for the tile-GEMM layers, and fp32 fragments for the layer kernels
      DDP_TRY(launch_b3_linear_sb(o.in_sb, o.wp_m, nullptr, o.xproj, 256, o.r * o.N, o.N, o.q_sb, o.fused_layer ? o.q : nullptr, M0,
                                  256, 256, 0, st, TAG_FEAT));
    } else {
      DDP_TRY(launch_linear_blk(o.mask, 256, false, o.wm, 256, nullptr, o.xproj, 256, o.r * o.N, o.N, o.q, M0, 256, 256, 0, st));
    }
    const X0Trace x0 = x0_trace_of(c, o, s);
    TailLaunch tl{};
    if (p.seg_tail) {
      tl.Q = o.q;
      tl.stream = o.tail_stream;
      tl.bias_ext = o.tail_bias;
      tl.lut = o.lut;
      // accumulation: softmax summed over the steps; otherwise the last step's scores are the output
      tl.prob = c->accumulation ? o.prob : o.logits;
      tl.prob_mode = c->accumulation ? (s == 0 ? 1 : 2) : (s == o.K - 1 ? 3 : 0);
      tl.mask_sb = p.u_chain ? nullptr : o.in_sb;
      tl.fuse_next = p.u_chain && s + 1 < o.K;
      if (tl.fuse_next) {
        tl.stream = o.tail4_stream;
        tl.bias_ext = o.tail4_bias;
        tl.ubuf = o.ubuf;
        tl.tlut = o.tlut;
        tl.res = o.xproj;
        tl.res_rn = o.r > 1 ? o.r * o.N : 0;
        // written fragment-major by the first step's head (k_layer MODE 7): one coalesced 1-KiB load per (t, g) in the tail instead of
        // 32 rows x 32 B (same box: head 0.62 -> 0.59 ms, tail -0.006 ms, +0.15 % on the batch; profiles/r05h_ab_xproj_frag.txt)
        tl.res_frag = p.head7 ? 1 : 0;
        tl.v_out = o.vpad;
        tl.samp_out = o.samp;
        tl.py = o.py[0];
        tl.px = o.px[0];
        tl.n_tok = o.Nh;
        tl.w = o.wh;
      }
      tl.x0_force = x0.force;
      tl.x0_keep = x0.keep;
      tl.x0_idx = x0.idx;
      tl.cp_bias = o.cprior_rows;                        // (nullptr without DDP_FLAG_CLASS_PRIOR)
      tl.cp_rn = o.r * o.N;
      tl.sp_rows = o.sprior_rows;                        // (nullptr without DDP_FLAG_SCORE_PRIOR)
      tl.sp_n = o.N;
      tl.M = M;
      tl.num_classes = o.Kc;
      tl.ldl = o.ldl;
      tl.alpha = sp.alpha;
      tl.sigma = sp.sigma;
      tl.alpha_next = sp.alpha_next;
      tl.sigma_next = sp.sigma_next;
      if (p.ddpm_chain && tl.fuse_next) {
        // fp32, in the reference's grouping (ddp.py:277: mask_t * (1 - c) / alpha, then * alpha_next)
        const float ua = (1.0f - sp.ddpm_c) / sp.alpha * sp.alpha_next, uc = sp.ddpm_c * sp.alpha_next;
        const bool noisy = sp.ddpm_add_noise != 0;
        if (noisy) {
          // the step's noise token-major, then U <- ua' U + std (E W_m^T): u_s is complete (step 0's head / the previous tail wrote
          // it) and this step's tail, inside the last layer's kernel or behind it, has not run yet
          DDP_TRY(stage_step_noise(key, d_step_noise, o.snoise, o.B, o.r, o.N, s, st));
          prof_begin(TAG_GENERIC, st);
          DDP_TRY(recorded(launch_u_noise(o.ubuf, o.snoise, o.wm, M0, ua, sp.ddpm_std, st), st));
        }
        // the tail derives ua = sigma_next / max(sigma, 1e-8), uc = alpha_next - alpha ua: these four give (ua, uc) back exactly
        tl.alpha = 0.0f;
        tl.sigma = 1.0f;
        tl.sigma_next = noisy ? 1.0f : ua;
        tl.alpha_next = uc;
      }
    }
    // layer 0's projections come from the step head on the prologue path; the tail reads the fp32 layer output, a head GEMM its SB copy
    DDP_TRY(encoder_forward(w, o, aff, st, /*l0_projected=*/o.fused_pro, /*sb_out=*/!p.seg_tail, p.lt_fused ? &tl : nullptr));
    if (p.seg_tail) {
      if (!p.lt_fused) DDP_TRY(launch_b3_tail(tl, st));
      continue;
    }
    DDP_TRY(head_gemm(c, w, o, st));
    SegUpdateArgs a = seg_update_args(o.logits, o.ldl, o.Kc, o.lut, o.mask, o.prob, c->accumulation ? (s == 0 ? 1 : 2) : 0, c->sampler,
                                      sp, M);
    a.x0_force = x0.force;
    a.x0_keep = x0.keep;
    a.x0_idx = x0.idx;
    a.cp_delta = o.cprior_rows ? o.cprior_rows + size_t(o.B) * 256 : nullptr;
    a.cp_rn = o.r * o.N;
    a.sp_rows = o.sprior_rows;
    a.sp_n = o.N;
    a.sp_kp = (o.Kc + 63) / 64 * 64;
    if (c->sampler == DDP_SAMPLER_DDPM && sp.ddpm_add_noise) {
      DDP_TRY(stage_step_noise(key, d_step_noise, o.snoise, o.B, o.r, o.N, s, st));
      a.step_noise = o.snoise;
    }
    DDP_TRY(launch_seg_update(a, st));
  }
  // reduction over (steps x r) and token-major -> NCHW (ddp.py:243-245); the layer kernel's tails leave the scores fragment-major
  const int frag_nch = p.seg_tail ? (o.Kc + 63) / 64 : 0;
  if (c->accumulation) DDP_TRY(launch_finalize_nchw(o.prob, o.ldl, d_out, o.B, o.r, o.Nh, o.Kc, float(o.r * o.K), st, frag_nch));
  else DDP_TRY(launch_finalize_nchw(o.logits, o.ldl, d_out, o.B, o.r, o.Nh, o.Kc, float(o.r), st, frag_nch));
  return step_disagreement(c, o, c->threshold, d_out, st);
}

// the depth sampler after the xproj hoist: noise staging, loop invariants of the chain, K steps, mean over r
int sample_depth(const ddp_cfg* c, const ddp_weights* w, const ddp_step* steps, const Plan& p, const Layout& o, const float* d_noise,
                 float* d_out, hipStream_t st) {
  const int M0 = int(o.M0);
  if (hipMemcpyAsync(o.mask, d_noise, size_t(M0) * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("noise copy failed");
    return DDP_E_LAUNCH;
  }
  DepthHeadArgs ha{};
  if (p.depth_chain) {
    DDP_TRY(launch_row_to_blk(o.xproj, o.xproj_f, M0, st));
    // (its sample table, that of a zero depth, is overwritten by the first step's head)
    DDP_TRY(launch_b3_l0proj(l0proj_launch(o, o.xproj_f, M0, o.rvpad), st));
    DDP_TRY(launch_row_to_sb(o.xproj, 256, o.in_sb, M0, 256, st));
    DDP_TRY(launch_b3_linear(o.in_sb, o.wp_cat[0], nullptr, nullptr, 0, 0, 0, o.rs0, 96, M0, 96, 256, st, TAG_SAMP));
    ha.rvpad = o.rvpad;
    ha.rs = o.rs0;
    ha.wv = o.wvs;
    ha.ws = o.wvs + 256;
    ha.py = o.py[0];
    ha.px = o.px[0];
    ha.dvec = o.mask;
    ha.v_out = o.vpad;
    ha.samp_out = o.samp;
    ha.R = o.R;
    ha.h = o.h;
    ha.w = o.w;
  }
  // the last layer's tail (depth_lt): the nine per-tap dot products of conv_depth, rows of 32, which k_depth_update sums
  TailLaunch tl{};
  tl.Q = o.q;
  tl.M = int(o.M);
  tl.num_classes = 9;
  tl.kind = 2;
  tl.prob = o.logits;
  tl.prob_mode = 3;
  tl.threshold = c->threshold;
  tl.ldl = 32;
  auto update_args = [&](const ddp_step& stp) { return depth_update_args(c, w, o, o.nbins ? nullptr : o.logits, o.mask, o.pred, stp); };
  // DDP_FLAG_STEP_RECORD: the step's metric prediction goes to its slice of the record instead of o.pred (the same kernels write
  // it, the mean over r reads the last slice)
  float* const rec = reinterpret_cast<float*>(o.step_rec);
  float* pred = o.pred;
  for (int s = 0; s < o.K; ++s) {
    const float* aff = o.aff + size_t(s) * o.L * 512;
    if (rec) pred = rec + size_t(s) * o.M;
    // fused step boundary: the PREVIOUS step's DDIM update (from the taps its last layer's tail left) runs in front of this head
    DepthUpdateArgs prev;
    const DepthUpdateArgs* upd = nullptr;
    if (p.depth_lt && s > 0) {
      prev = update_args(steps[s - 1]);
      upd = &prev;
    }
    if (p.depth_chain) {
      ha.upd = upd;
      DDP_TRY(launch_depth_head(ha, st));
    } else if (o.fused_pro) {
      // down conv over cat[x, depth_t] (depther/ddp.py:236-237) = hoisted x half + ONE depth column: q is formed inside
      // the layer-0 projection kernel (k_layer MODE 3): no feat / SB-conversion / VALUE / SAMP launches
      L0ProjLaunch pj = l0proj_launch(o, o.q, M0, o.vpad);
      pj.res = o.xproj;
      pj.res_rn = o.r > 1 ? o.r * o.N : 0;
      pj.wm = o.wm;
      pj.dvec = o.mask;
      pj.upd = upd;
      DDP_TRY(launch_b3_l0proj(pj, st));
    } else {
      DDP_TRY(launch_feat_depth(o.xproj, o.wm, o.mask, o.s, o.B, o.r, o.N, st));
      DDP_TRY(publish_q(o, o.s, st));
    }
    // the step head projects layer 0 on the fused path; the fused tail and the binned head read the fp32 layer output, a head GEMM SB
    DDP_TRY(encoder_forward(w, o, aff, st, /*l0_projected=*/o.fused_pro, /*sb_out=*/!(p.depth_lt || o.nbins), p.depth_lt ? &tl : nullptr,
                            p.depth_chain));
    if (p.depth_lt) {
      // (the nine taps were written by the last layer's tail: k_layer MODE 9)
    } else if (o.nbins) {
      DDP_TRY(depth_bins_head(c, o, pred, st));
    } else {
      DDP_TRY(head_gemm(c, w, o, st));
    }
    // the update of every step but the last runs inside the next step's head (k_layer MODE 3) on the fused path; the last step's
    // (and every step's on the other paths) here: it also leaves the metric depth prediction the output is made of
    if (!(p.depth_lt && s + 1 < o.K)) {
      DepthUpdateArgs ua = update_args(steps[s]);
      ua.pred = pred;
      DDP_TRY(launch_depth_update(ua, st));
    } else if (rec) {
      // (fused boundary: the next step's head forms this prediction in registers and keeps only the updated depth - the record
      // takes it from the same taps by k_depth_update's head-only form, which leaves the noisy depth alone)
      DepthUpdateArgs ua = update_args(steps[s]);
      ua.pred = pred;
      ua.depth_t = nullptr;
      prof_begin(TAG_GENERIC, st);
      DDP_TRY(recorded(launch_depth_update(ua, st), st));
    }
  }
  DDP_TRY(launch_mean_r(pred, d_out, o.B, o.r, o.N, st));
  return step_disagreement(c, o, c->threshold, d_out, st);
}

// the BEV sampler after the xproj hoist: noise staging (u_0 on the chain), K steps, reduction
int sample_bev(const ddp_cfg* c, const ddp_weights* w, const ddp_step* steps, const Plan& p, const Layout& o, const float* d_noise,
               float* d_out, hipStream_t st) {
  const int M0 = int(o.M0);
  // geom: the map (h, w) and the head grid - the x0 feedback; rs: the grid resampling, whose source is the prescaled map when
  // cfg->bev_prescale is set.  The prescale is linear, so the u chain survives: resample(prescale(W_x x + b + u)) = rx' +
  // resample(prescale(u)), with u kept at the map size (the nearest-resize of the thresholded maps goes to (h, w))
  const BevGeom geom = bev_geom(c), rs = bev_geom(c, &o);
  const BevPrescale ps{o.h, o.w, o.hp, o.wp, o.pre_rscale};
  // the source of the grid resampling for a row-major map `src` of `maps` maps
  auto prescaled = [&](const float* src, int maps, const float** out) {
    *out = src;
    if (!o.prescale) return int(DDP_OK);
    *out = o.pre;
    return launch_bev_prescale(src, o.pre, maps, ps, st);
  };
  const float* rsrc = nullptr;
  unsigned char* code = reinterpret_cast<unsigned char*>(o.logits);            // (M) the step's x0 code per head-grid token
  if (p.bev_chain) {
    DDP_TRY(prescaled(o.xproj, o.B, &rsrc));
    DDP_TRY(launch_bev_resample(rsrc, o.s, o.B, rs, st));                       // rx = resample(W_x x + b), B maps
    DDP_TRY(launch_nchw_to_sb(d_noise, o.in_sb, o.R, 256, o.N, st));
    DDP_TRY(launch_b3_linear(o.in_sb, o.wp_m, nullptr, nullptr, 0, 0, 0, o.feat0, 256, M0, 256, 256, st, TAG_FEAT));   // u_0 = W_m . noise
  } else {
    DDP_TRY(launch_nchw_to_tok(d_noise, o.mask, o.R, 256, o.N, st));
  }
  // the last layer's tail (bev_chain): conv_seg + sigmoid, the probabilities accumulated and the step's x0 codes written
  TailLaunch tl{};
  tl.Q = o.q;
  tl.M = int(o.M);
  tl.num_classes = o.Kc;
  tl.kind = 1;
  tl.prob = o.prob;
  tl.threshold = c->threshold;
  tl.x0_idx = code;
  tl.ldl = 32;
  // DDP_FLAG_STEP_RECORD: after the step's head, its decisions as bit words - from the code byte on the u chain, else from the
  // raw logits k_bev_update thresholds (both on the head grid, in front of the nearest resize to the map)
  auto record = [&](int s) {
    if (!o.step_rec) return int(DDP_OK);
    prof_begin(TAG_GENERIC, st);
    return recorded(launch_bev_record(p.bev_chain ? code : nullptr, o.logits, reinterpret_cast<unsigned*>(o.step_rec) + size_t(s) * o.M,
                                      o.Kc, c->threshold, int(o.M), st), st);
  };
  for (int s = 0; s < o.K; ++s) {
    const ddp_step& sp = steps[s];
    const float* aff = o.aff + size_t(s) * o.L * 512;
    if (p.bev_chain) {
      if (s > 0) {
        // m' = alpha' x0 + sigma' (m - alpha x0) / max(sigma, 1e-8) (fusion_models/ddp.py:296-297) under W_m, with the PREVIOUS step's scalars
        const ddp_step& pp = steps[s - 1];
        const float ua = pp.sigma_next / (pp.sigma > 1e-8f ? pp.sigma : 1e-8f);
        DDP_TRY(launch_bev_u_update(o.feat0, code, o.tlut, o.R, geom, ua, pp.alpha_next - pp.alpha * ua, st));
      }
      DDP_TRY(prescaled(o.feat0, o.R, &rsrc));
      DDP_TRY(launch_bev_q(rsrc, o.s, o.q, o.R, o.r, rs, st));
    } else {
      // feat = transform(cat[x, mask_t]) on the map, then the grid transform to the head grid
      if (o.b3) {
        DDP_TRY(launch_row_to_sb(o.mask, 256, o.in_sb, M0, 256, st));
        DDP_TRY(launch_b3_linear(o.in_sb, o.wp_m, nullptr, o.xproj, 256, o.r * o.N, o.N, o.feat0, 256, M0, 256, 256, st, TAG_XPROJ));
      } else {
        DDP_TRY(launch_linear(o.mask, 256, false, o.wm, 256, nullptr, o.xproj, 256, o.r * o.N, o.N, o.feat0, 256, M0, 256, 256, 0, st));
      }
      DDP_TRY(prescaled(o.feat0, o.R, &rsrc));
      DDP_TRY(launch_bev_resample(rsrc, o.s, o.R, rs, st));
      DDP_TRY(publish_q(o, o.s, st));
    }
    tl.prob_mode = s == 0 ? 1 : 2;
    // (the 3x3 conv_seg reads the fp32 layer output of a plain last layer)
    DDP_TRY(encoder_forward(w, o, aff, st, /*l0_projected=*/false, /*sb_out=*/!p.bev_chain && !p.bev_seg3,
                            p.bev_chain && !p.bev_seg3 ? &tl : nullptr));
    if (p.bev_seg3) {
      DDP_TRY(bev_seg3_head(c, o, s == 0, p.bev_chain ? code : nullptr, p.bev_chain ? nullptr : o.logits, st));
      DDP_TRY(record(s));
      if (p.bev_chain) continue;
      BevUpdateArgs ua = bev_update_args(c, w, o, o.mask, s == 0, sp);
      ua.prob = nullptr;             // (k_bev_seg3 accumulated the probabilities)
      DDP_TRY(launch_bev_update(ua, st));
      continue;
    }
    if (p.bev_chain) {             // (the next step's head updates u from the codes the tail wrote)
      DDP_TRY(record(s));
      continue;
    }
    DDP_TRY(head_gemm(c, w, o, st));
    DDP_TRY(record(s));
    DDP_TRY(launch_bev_update(bev_update_args(c, w, o, o.mask, s == 0, sp), st));
  }
  DDP_TRY(launch_finalize_nchw(o.prob, 32, d_out, o.B, o.r, o.Nh, o.Kc, float(o.r * o.K), st));
  return step_disagreement(c, o, c->threshold, d_out, st);
}

}  // namespace
}  // namespace ddp

using namespace ddp;

extern "C" {

const char* ddp_last_error(void) { return g_err; }
int ddp_abi_version(void) { return DDP_ABI_VERSION; }

int ddp_profile_begin(int tag) {
  if ((tag < 0 || tag >= TAG_COUNT) && tag != PROF_ALL) {
    set_error("profile: unknown tag %d", tag);
    return DDP_E_BADCFG;
  }
  if (!g_prof.created) {
    for (int i = 0; i < 2 * PROF_MAX; ++i)
      if (hipEventCreate(&g_prof.ev[i]) != hipSuccess) {
        set_error("hipEventCreate failed");
        return DDP_E_LAUNCH;
      }
    g_prof.created = true;
  }
  g_prof.n = 0;
  g_prof.tag = tag;
  g_prof.resolved = false;
  return DDP_OK;
}

int ddp_profile_end(float* total_ms, int* launches) {
  const int n = g_prof.n;
  g_prof.tag = -1;
  float tot = 0.f;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) {
      set_error("hipEventSynchronize failed");
      return DDP_E_LAUNCH;
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]);
    g_prof.ms[i] = ms;
    tot += ms;
  }
  g_prof.resolved = true;
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
  return DDP_OK;
}

int ddp_profile_read(int tag, float* total_ms, int* launches) {
  // after ddp_profile_end: the share of one call site in the records of the last session
  if (tag < 0 || tag >= TAG_COUNT) {
    set_error("profile: unknown tag %d", tag);
    return DDP_E_BADCFG;
  }
  if (!g_prof.resolved) {
    set_error("profile: no finished session (call ddp_profile_end first)");
    return DDP_E_BADCFG;
  }
  float tot = 0.f;
  int cnt = 0;
  for (int i = 0; i < g_prof.n; ++i)
    if (g_prof.rec_tag[i] == tag) {
      tot += g_prof.ms[i];
      ++cnt;
    }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  return DDP_OK;
}

int ddp_query_workspace(const ddp_cfg* cfg, size_t* bytes) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_bytes(bytes));
  Layout o;
  carve(cfg, nullptr, &o);
  *bytes = o.total;
  return DDP_OK;
}

int ddp_prepare(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_step* steps, void* d_workspace,
                void* stream) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_weights(cfg, weights));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  if (!steps) {
    set_error("steps is NULL");
    return DDP_E_NULL;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  Layout o;
  carve(cfg, static_cast<char*>(d_workspace), &o);
  DDP_TRY(prepare_model(cfg, weights, o, st));
  DDP_TRY(prepare_geometry(o, st));
  float tin[DDP_MAX_STEPS];
  for (int s = 0; s < o.K; ++s) tin[s] = steps[s].time_in;
  DDP_TRY(launch_write_floats(tin, o.K, o.tin, st));
  DDP_TRY(time_embed_dev(weights, o.L, o.tin, o.K, o.u, o.hid, o.temb, o.film, st));
  DDP_TRY(fold_affine_dev(weights, o.L, o.K, o.film, o.aff, st));
  return DDP_OK;
}

int ddp_query_const_workspace(const ddp_cfg* cfg, size_t* bytes) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_bytes(bytes));
  Layout o;
  carve(cfg, nullptr, &o);
  *bytes = o.const_bytes;
  return DDP_OK;
}

int ddp_prepare_geometry(const ddp_cfg* cfg, void* d_workspace, void* stream) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  Layout o;
  carve(cfg, static_cast<char*>(d_workspace), &o);
  return prepare_geometry(o, static_cast<hipStream_t>(stream));
}

int ddp_sample(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_step* steps, const float* d_x,
               const float* d_noise, const float* d_step_noise, float* d_out, void* d_workspace, void* stream) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_weights(cfg, weights));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  DDP_TRY(check_ptr(d_x, "x"));
  DDP_TRY(check_ptr(d_noise, "noise"));
  DDP_TRY(check_ptr(d_out, "out"));
  if (!steps) {
    set_error("steps is NULL");
    return DDP_E_NULL;
  }
  const bool seeded = (cfg->flags & DDP_FLAG_SEEDED_NOISE) != 0;
  if (cfg->sampler == DDP_SAMPLER_DDPM && !seeded) DDP_TRY(check_ptr(d_step_noise, "step_noise"));
  hipStream_t st = static_cast<hipStream_t>(stream);
  Layout o;
  carve(cfg, static_cast<char*>(d_workspace), &o);
  const Plan p = plan_of(cfg, o);
  // DDP_FLAG_X0_HINTS: the caller's map as read NOW (a captured graph replays this launch on the buffer's current content) -> rows
  if (o.hint_rows) {
    prof_begin(TAG_GENERIC, st);
    DDP_TRY(recorded(launch_hint_rows(o.hint_map, o.hint_rows, cfg->task, o.B, o.r, o.N, o.Kc, st), st));
  }
  // DDP_FLAG_CLASS_PRIOR: the caller's table as read NOW -> the per-image bias / prior rows of the seg decision kernels
  if (o.cprior_rows) {
    prof_begin(TAG_GENERIC, st);
    DDP_TRY(recorded(launch_class_prior(o.cprior_table, weights->head_b, o.cprior_rows, o.cprior_rows + size_t(o.B) * 256, o.B, o.Kc, st),
                     st));
  }
  // DDP_FLAG_SCORE_PRIOR: the caller's NCHW map as read NOW -> the token-major prior rows of the seg decision kernels
  if (o.sprior_rows) {
    prof_begin(TAG_GENERIC, st);
    DDP_TRY(recorded(launch_score_prior_rows(o.sprior_map, o.sprior_rows, o.B, o.Kc, o.N, st), st));
  }
  const uint32_t* key = nullptr;
  if (seeded) {
    key = reinterpret_cast<const uint32_t*>(d_noise);
    DDP_TRY(seeded_start_noise(key, o.seed_noise, o.B, size_t(o.r) * o.Cm * o.N, st));
    d_noise = o.seed_noise;
  }
  // DDP_FLAG_PRIOR_START: the loop's first read comes from alpha(t_start) x0(prior) + sigma(t_start) eps, eps = what d_noise is by
  // now.  The prior is read from device memory when the kernel runs (a captured graph replays this launch on the buffer's current
  // content); the seeded-noise buffer is mixed in place
  if (o.prior_map) {
    PriorStartArgs pa;
    pa.prior = o.prior_map;
    pa.table = cfg->task == DDP_TASK_SEG ? o.lut : weights->embedding;
    pa.eps = d_noise;
    pa.out = seeded ? o.seed_noise : o.prior_start;
    pa.task = cfg->task;
    pa.B = o.B;
    pa.r = o.r;
    pa.N = o.N;
    pa.num_classes = o.Kc;
    pa.alpha = steps[0].alpha;
    pa.sigma = steps[0].sigma;
    pa.bit_scale = cfg->bit_scale;
    pa.min_depth = cfg->min_depth;
    pa.max_depth = cfg->max_depth;
    prof_begin(TAG_GENERIC, st);
    DDP_TRY(recorded(launch_prior_start(pa, st), st));
    d_noise = pa.out;
  }
  // loop-invariant half of the concat-conv: xproj = W_x x + b  (ddp.py:223-224 with the x columns hoisted)
  if (p.head7) {
    // (inside the first step's head)
  } else if (o.b3) {
    DDP_TRY(launch_nchw_to_sb(d_x, o.in_sb, o.B, o.Cx, o.N, st));       // NCHW -> split fragments in one pass
    DDP_TRY(launch_b3_linear(o.in_sb, o.wp_x, weights->transform_b, nullptr, 0, 0, 0, o.xproj, 256, o.B * o.N, 256, o.Cx, st,
                             TAG_XPROJ));
  } else {
    DDP_TRY(launch_nchw_to_tok(d_x, o.xtok, o.B, o.Cx, o.N, st));
    DDP_TRY(launch_linear(o.xtok, o.Cx, false, o.wx, o.Cx, weights->transform_b, nullptr, 0, 0, 0, o.xproj, 256, o.B * o.N,
                          256, o.Cx, 0, st, TAG_XPROJ));
  }
  if (cfg->task == DDP_TASK_SEG) return sample_seg(cfg, weights, steps, p, o, d_x, d_noise, d_step_noise, key, d_out, st);
  if (cfg->task == DDP_TASK_DEPTH) return sample_depth(cfg, weights, steps, p, o, d_noise, d_out, st);
  return sample_bev(cfg, weights, steps, p, o, d_noise, d_out, st);
}

int ddp_x0_trace(const ddp_cfg* cfg, void* d_workspace, const unsigned char** d_idx) {
  DDP_TRY(validate(cfg));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  const bool step_rec = d_idx && (cfg->flags & DDP_FLAG_STEP_RECORD);
  if (!step_rec && (!d_idx || !(cfg->flags & (DDP_FLAG_RECORD_X0 | DDP_FLAG_FORCE_X0)) || cfg->task != DDP_TASK_SEG)) {
    set_error("x0_trace: needs a segmentation cfg with DDP_FLAG_RECORD_X0 or DDP_FLAG_FORCE_X0");
    return DDP_E_BADCFG;
  }
  Layout o;
  carve(cfg, static_cast<char*>(d_workspace), &o);
  *d_idx = step_rec ? o.step_rec : o.x0_trace;
  return DDP_OK;
}

int ddp_head_forward(const ddp_cfg* cfg, const ddp_weights* weights, const float* d_feat, const float* d_temb,
                     float* d_out, void* d_workspace, void* stream) {
  // one decoder pass has no x0 feedback and no start map: DDP_FLAG_X0_HINTS, DDP_FLAG_PRIOR_START, DDP_FLAG_CLASS_PRIOR and
  // DDP_FLAG_SCORE_PRIOR are ignored (the buffers they carve lie behind everything used here)
  ddp_cfg no_hints;
  if (cfg && (cfg->flags & (DDP_FLAG_X0_HINTS | DDP_FLAG_PRIOR_START | DDP_FLAG_CLASS_PRIOR | DDP_FLAG_SCORE_PRIOR))) {
    no_hints = *cfg;
    no_hints.flags &= ~(DDP_FLAG_X0_HINTS | DDP_FLAG_PRIOR_START | DDP_FLAG_CLASS_PRIOR | DDP_FLAG_SCORE_PRIOR);
    cfg = &no_hints;
  }
  DDP_TRY(validate(cfg));
  DDP_TRY(check_weights(cfg, weights));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  DDP_TRY(check_ptr(d_feat, "feat"));
  DDP_TRY(check_ptr(d_out, "out"));
  hipStream_t st = static_cast<hipStream_t>(stream);
  Layout o;
  carve(cfg, static_cast<char*>(d_workspace), &o);
  DDP_TRY(prepare_model(cfg, weights, o, st));
  DDP_TRY(prepare_geometry(o, st));
  const float* film = nullptr;
  if (d_temb) {
    for (int l = 0; l < o.L; ++l) {
      if (!weights->layers[l].time_w) continue;
      DDP_TRY(launch_matvec(weights->layers[l].time_w, weights->layers[l].time_b, d_temb, o.film + size_t(l) * 512,
                            DDP_TIME_DIM, 512, 1, DDP_TIME_DIM, o.L * 512, 2, 0, st));
    }
    film = o.film;
  }
  DDP_TRY(fold_affine_dev(weights, o.L, 1, film, o.aff, st));
  if (cfg->task == DDP_TASK_BEV) {
    DDP_TRY(launch_nchw_to_tok(d_feat, o.feat0, o.R, 256, o.N, st));
    const float* rsrc = o.feat0;
    if (o.prescale) {
      DDP_TRY(launch_bev_prescale(o.feat0, o.pre, o.R, BevPrescale{o.h, o.w, o.hp, o.wp, o.pre_rscale}, st));
      rsrc = o.pre;
    }
    DDP_TRY(launch_bev_resample(rsrc, o.s, o.R, bev_geom(cfg, &o), st));
  } else {
    DDP_TRY(launch_nchw_to_tok(d_feat, o.s, o.R, 256, o.N, st));      // row-major staging in `s`
  }
  DDP_TRY(publish_q(o, o.s, st));
  DDP_TRY(encoder_forward(weights, o, o.aff, st));
  // outputs (R,K,h,w) or, for depth, (R,1,h,w) == (R*N)
  if (cfg->task == DDP_TASK_DEPTH && o.nbins) return depth_bins_head(cfg, o, d_out, st);
  if (o.seg3) {
    DDP_TRY(bev_seg3_head(cfg, o, true, nullptr, nullptr, st));
    return launch_finalize_nchw(o.prob, 32, d_out, o.R, 1, o.Nh, o.Kc, 1.0f, st);
  }
  DDP_TRY(head_gemm(cfg, weights, o, st));
  if (cfg->task == DDP_TASK_SEG) return launch_finalize_nchw(o.logits, o.ldl, d_out, o.R, 1, o.Nh, o.Kc, 1.0f, st);
  if (cfg->task == DDP_TASK_DEPTH) return launch_depth_update(depth_update_args(cfg, weights, o, o.logits, nullptr, d_out, ddp_step{}), st);
  DDP_TRY(launch_bev_update(bev_update_args(cfg, weights, o, nullptr, true, ddp_step{}), st));
  return launch_finalize_nchw(o.prob, 32, d_out, o.R, 1, o.Nh, o.Kc, 1.0f, st);
}

int ddp_msda_forward(const float* d_value, const float* d_samp, float* d_out, int rows, int h, int w, void* stream) {
  DDP_TRY(check_ptr(d_value, "value"));
  DDP_TRY(check_ptr(d_samp, "samp"));
  DDP_TRY(check_ptr(d_out, "out"));
  if (rows < 0 || h < 1 || w < 1 || rows % (h * w)) {
    set_error("msda: rows=%d must be a multiple of h*w=%d", rows, h * w);
    return DDP_E_BADCFG;
  }
  return launch_msda_gather(d_value, d_samp, d_out, rows, h * w, h, w, static_cast<hipStream_t>(stream));
}

namespace {
struct MsdaLdsLayout {
  float *vpad, *samp_hm, *tab_y, *tab_x;
  unsigned short* out_sb;
  size_t vpad_floats, bytes;
};
int msda_lds_layout(int rows, int h, int w, char* base, MsdaLdsLayout* o) {
  if (rows < 1 || h < 1 || w < 1 || rows % (h * w)) {
    set_error("msda_lds: rows=%d must be a positive multiple of h*w=%d", rows, h * w);
    return DDP_E_BADCFG;
  }
  Carver cv{base};
  const size_t R = size_t(rows) / (size_t(h) * w);
  o->vpad_floats = (R * (h + 2) + 1) * (w + 2) * 256 + 256;      // + one zero row below the last map, as in the sampler's workspace
  o->vpad = cv.take<float>(o->vpad_floats);
  o->samp_hm = cv.take<float>(size_t(rows) * DDP_SAMP_STRIDE);
  o->tab_y = cv.take<float>(size_t(h) * 96);
  o->tab_x = cv.take<float>(size_t(w) * 96);
  o->out_sb = cv.take<unsigned short>((size_t(rows) + 255) / 256 * 256 * 256 * 3);
  o->bytes = cv.off;
  return DDP_OK;
}
}  // namespace

int ddp_msda_forward_lds_workspace(int rows, int h, int w, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  MsdaLdsLayout o;
  DDP_TRY(msda_lds_layout(rows, h, w, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

int ddp_msda_forward_lds(const float* d_value, const float* d_samp, const float* d_guess, float* d_out, int rows, int h, int w,
                         void* d_workspace, void* stream) {
  DDP_TRY(check_ptr(d_value, "value"));
  DDP_TRY(check_ptr(d_samp, "samp"));
  DDP_TRY(check_ptr(d_out, "out"));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  MsdaLdsLayout o;
  DDP_TRY(msda_lds_layout(rows, h, w, static_cast<char*>(d_workspace), &o));
  hipStream_t st = static_cast<hipStream_t>(stream);
  DDP_TRY(launch_msda_lds_adapters_in(d_value, d_samp, d_guess, o.vpad, o.vpad_floats, o.samp_hm, o.tab_y, o.tab_x, rows, h * w, h, w,
                                      st));
  // the kernel of the sampling loop, launched exactly as encoder_forward launches it
#if DDP_S_F32
  float* out_blk = reinterpret_cast<float*>(o.out_sb);            // (the SB slot is 1.5x the size of the fp32 fragments)
  DDP_TRY(launch_msda_gather_sb_pad(o.vpad, o.samp_hm, nullptr, out_blk, rows, h * w, h, w, o.tab_y, o.tab_x, d_guess ? 0 : 1, st));
  return launch_blk_to_row(out_blk, d_out, rows, st);
#else
  DDP_TRY(launch_msda_gather_sb_pad(o.vpad, o.samp_hm, o.out_sb, nullptr, rows, h * w, h, w, o.tab_y, o.tab_x, d_guess ? 0 : 1, st));
  return launch_sb_to_row(o.out_sb, d_out, rows, 256, st);
#endif
}

int ddp_linear(const float* d_a, const float* d_w, const float* d_bias, float* d_out, int m, int n, int k, int gelu,
               void* stream) {
  DDP_TRY(check_ptr(d_a, "a"));
  DDP_TRY(check_ptr(d_w, "w"));
  DDP_TRY(check_ptr(d_out, "out"));
  if (n % 4) {
    set_error("linear: n=%d must be a multiple of 4 (row stride of out)", n);
    return DDP_E_BADCFG;
  }
  return launch_linear(d_a, k, false, d_w, k, d_bias, nullptr, 0, 0, 0, d_out, n, m, n, k, gelu,
                       static_cast<hipStream_t>(stream));
}

namespace {
struct LinB3Layout {
  unsigned short *a_sb, *wsplit;
  size_t bytes;
};
int linb3_layout(int m, int n, int k, char* base, LinB3Layout* o) {
  if (m < 1 || n < 1 || k < 32 || k % 32 || n % 4) {
    set_error("linear_b3: m=%d n=%d k=%d (k must be a positive multiple of 32, n of 4)", m, n, k);
    return DDP_E_BADCFG;
  }
  const size_t mp = (size_t(m) + 255) / 256 * 256;
  Carver cv{base};
  o->a_sb = cv.take<unsigned short>(mp * k * 3);
  o->wsplit = cv.take<unsigned short>(size_t(3) * n * k);
  o->bytes = cv.off;
  return DDP_OK;
}
}  // namespace

int ddp_linear_b3_workspace(int m, int n, int k, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  LinB3Layout o;
  DDP_TRY(linb3_layout(m, n, k, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

int ddp_linear_b3(const float* d_a, const float* d_w, const float* d_bias, float* d_out, int m, int n, int k,
                  void* d_workspace, void* stream) {
  DDP_TRY(check_ptr(d_a, "a"));
  DDP_TRY(check_ptr(d_w, "w"));
  DDP_TRY(check_ptr(d_out, "out"));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  LinB3Layout o;
  DDP_TRY(linb3_layout(m, n, k, static_cast<char*>(d_workspace), &o));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // operands -> exact 3-way bf16 splits (activations as SB fragments, weights K-permuted), then the tile GEMM
  DDP_TRY(launch_row_to_sb(d_a, k, o.a_sb, m, k, st));
  DDP_TRY(launch_split_weights(d_w, k, n, k, o.wsplit, st));
  SplitW w;
  w.p = o.wsplit;
  w.comp_stride = size_t(n) * k;
  return launch_b3_linear(o.a_sb, w, d_bias, nullptr, 0, 0, 0, d_out, n, m, n, k, st, TAG_GENERIC);
}

int ddp_time_embed(const ddp_weights* weights, int num_layers, const float* time_in_host, int s, float* d_temb,
                   float* d_film, float* d_scratch, void* stream) {
  if (!weights || !time_in_host || s < 1 || s > DDP_MAX_STEPS || num_layers < 0 || num_layers > DDP_MAX_LAYERS) {
    set_error("time_embed: bad arguments");
    return DDP_E_BADCFG;
  }
  DDP_TRY(check_ptr(d_temb, "temb"));
  DDP_TRY(check_ptr(d_scratch, "scratch"));
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* tin = d_scratch;
  float* u = d_scratch + 64;
  float* hid = u + align64(size_t(s) * DDP_SINU_FEATS);
  DDP_TRY(launch_write_floats(time_in_host, s, tin, st));
  return time_embed_dev(weights, d_film ? num_layers : 0, tin, s, u, hid, d_temb, d_film, st);
}

int ddp_ddim_update_seg(const float* d_logits, int ld_logits, int num_classes, const float* d_lut, float* d_mask,
                        int rows, const ddp_step* step, void* stream) {
  DDP_TRY(check_ptr(d_logits, "logits"));
  DDP_TRY(check_ptr(d_lut, "lut"));
  DDP_TRY(check_ptr(d_mask, "mask"));
  if (!step || num_classes < 1 || num_classes > 256) {
    set_error("ddim_update_seg: bad arguments");
    return DDP_E_BADCFG;
  }
  return launch_seg_update(seg_update_args(d_logits, ld_logits, num_classes, d_lut, d_mask, nullptr, 0, DDP_SAMPLER_DDIM, *step, rows),
                           static_cast<hipStream_t>(stream));
}

int ddp_seg_x0_project(const float* d_scores, int batch, int num_classes, int n_pix, const float* d_embedding, float bit_scale,
                       float* d_x0, void* stream) {
  DDP_TRY(check_ptr(d_scores, "scores"));
  DDP_TRY(check_ptr(d_embedding, "embedding"));
  DDP_TRY(check_ptr(d_x0, "x0"));
  if (batch < 1 || num_classes < 1 || n_pix < 1) {
    set_error("seg_x0_project: bad sizes (batch %d classes %d pixels %d)", batch, num_classes, n_pix);
    return DDP_E_BADCFG;
  }
  return launch_seg_x0_nchw(d_scores, d_embedding, d_x0, batch, num_classes, n_pix, bit_scale, static_cast<hipStream_t>(stream));
}

int ddp_seg_postprocess(const float* d_scores, int batch, int num_classes, int h, int w, int img_h, int img_w, int crop_h,
                        int crop_w, int out_h, int out_w, int align_corners, int flip, unsigned char* d_seg, void* stream) {
  DDP_TRY(check_ptr(d_scores, "scores"));
  if (!d_seg) {
    set_error("seg is NULL");
    return DDP_E_NULL;
  }
  if (batch < 1 || num_classes < 1 || num_classes > 256 || h < 1 || w < 1 || img_h < 1 || img_w < 1 || crop_h < 1 ||
      crop_w < 1 || crop_h > img_h || crop_w > img_w || out_h < 1 || out_w < 1 || flip < 0 || flip > 2) {
    set_error("seg_postprocess: bad geometry (B %d K %d map %dx%d image %dx%d crop %dx%d out %dx%d flip %d)", batch,
              num_classes, h, w, img_h, img_w, crop_h, crop_w, out_h, out_w, flip);
    return DDP_E_BADCFG;
  }
  SegPostArgs a;
  a.logits = d_scores;
  a.B = batch;
  a.K = num_classes;
  a.h = h;
  a.w = w;
  a.H = img_h;
  a.W = img_w;
  a.ch = crop_h;
  a.cw = crop_w;
  a.oh = out_h;
  a.ow = out_w;
  a.align = align_corners ? 1 : 0;
  a.flip = flip;
  a.seg = d_seg;
  return launch_seg_postprocess(a, static_cast<hipStream_t>(stream));
}

int ddp_seg_aug_postprocess(const ddp_seg_aug* augs, int n_aug, int batch, int num_classes, int out_h, int out_w,
                            int align_corners, unsigned char* d_seg, float* d_prob, void* stream) {
  if (!augs || !d_seg) {
    set_error("seg_aug_postprocess: augs / seg is NULL");
    return DDP_E_NULL;
  }
  if (n_aug < 1 || n_aug > DDP_MAX_AUGS || batch < 1 || num_classes < 1 || num_classes > 256 || out_h < 1 || out_w < 1) {
    set_error("seg_aug_postprocess: bad arguments (n_aug %d B %d K %d out %dx%d)", n_aug, batch, num_classes, out_h, out_w);
    return DDP_E_BADCFG;
  }
  for (int i = 0; i < n_aug; ++i) {
    const ddp_seg_aug& g = augs[i];
    DDP_TRY(check_ptr(g.d_scores, "aug scores"));
    if (g.h < 1 || g.w < 1 || g.img_h < 1 || g.img_w < 1 || g.crop_h < 1 || g.crop_w < 1 || g.crop_h > g.img_h ||
        g.crop_w > g.img_w || g.flip < 0 || g.flip > 2) {
      set_error("seg_aug_postprocess: augmentation %d: bad geometry (map %dx%d image %dx%d crop %dx%d flip %d)", i, g.h, g.w,
                g.img_h, g.img_w, g.crop_h, g.crop_w, g.flip);
      return DDP_E_BADCFG;
    }
  }
  if (d_prob) DDP_TRY(check_ptr(d_prob, "prob"));
  return launch_seg_aug_postprocess(augs, n_aug, batch, num_classes, out_h, out_w, align_corners ? 1 : 0, d_seg, d_prob,
                                    static_cast<hipStream_t>(stream));
}

int ddp_seg_slide_postprocess(const float* const* d_scores, const int* win_y1, const int* win_x1, int n_rows, int n_cols, int batch,
                              int num_classes, int h, int w, int crop_h, int crop_w, int img_h, int img_w, int keep_h, int keep_w,
                              int out_h, int out_w, int align_corners, int flip, int prob_mode, unsigned char* d_seg, float* d_prob,
                              void* stream) {
  if (!d_scores || !win_y1 || !win_x1 || (!d_seg && !d_prob)) {
    set_error("seg_slide_postprocess: scores / window origins / both outputs NULL");
    return DDP_E_NULL;
  }
  if (n_rows < 1 || n_cols < 1 || n_rows * n_cols > DDP_MAX_WINDOWS || batch < 1 || num_classes < 1 || num_classes > 256 || h < 1 ||
      w < 1 || crop_h < 1 || crop_w < 1 || crop_h > img_h || crop_w > img_w || keep_h < 1 || keep_w < 1 || keep_h > img_h ||
      keep_w > img_w || out_h < 1 || out_w < 1 || flip < 0 || flip > 2 || prob_mode < 0 || prob_mode > 2 || (prob_mode && !d_prob)) {
    set_error("seg_slide_postprocess: bad geometry (%dx%d windows of %dx%d on %dx%d, B %d K %d map %dx%d keep %dx%d out %dx%d flip %d "
              "prob_mode %d)", n_rows, n_cols, crop_h, crop_w, img_h, img_w, batch, num_classes, h, w, keep_h, keep_w, out_h, out_w, flip,
              prob_mode);
    return DDP_E_BADCFG;
  }
  // every image pixel covered, by at most 4 window rows / columns (the kernel keeps that many per tap in registers)
  for (int axis = 0; axis < 2; ++axis) {
    const int* o = axis ? win_x1 : win_y1;
    const int n = axis ? n_cols : n_rows, crop = axis ? crop_w : crop_h, size = axis ? img_w : img_h;
    int covered = 0;
    for (int i = 0; i < n; ++i) {
      if (o[i] < 0 || o[i] + crop > size || (i > 0 && o[i] < o[i - 1]) || o[i] > covered) {
        set_error("seg_slide_postprocess: window origins along axis %d must be ascending, inside the image and leave no gap", axis);
        return DDP_E_BADCFG;
      }
      covered = o[i] + crop;
      if (i >= 4 && o[i - 4] + crop > o[i]) {
        set_error("seg_slide_postprocess: more than 4 windows overlap along axis %d (stride < crop / 4)", axis);
        return DDP_E_BADCFG;
      }
    }
    if (covered < size) {
      set_error("seg_slide_postprocess: the windows do not cover the image along axis %d", axis);
      return DDP_E_BADCFG;
    }
  }
  for (int i = 0; i < n_rows * n_cols; ++i) DDP_TRY(check_ptr(d_scores[i], "window scores"));
  if (d_prob) DDP_TRY(check_ptr(d_prob, "prob"));
  return launch_seg_slide_postprocess(d_scores, win_y1, win_x1, n_rows, n_cols, batch, num_classes, h, w, crop_h, crop_w, img_h, img_w,
                                      keep_h, keep_w, out_h, out_w, align_corners ? 1 : 0, flip, prob_mode, d_seg, d_prob,
                                      static_cast<hipStream_t>(stream));
}

int ddp_depth_postprocess(const ddp_depth_aug* augs, int n_aug, int batch, int out_h, int out_w, int align_corners,
                          float min_depth, float max_depth, float* d_out, void* stream) {
  if (!augs) {
    set_error("depth_postprocess: augs is NULL");
    return DDP_E_NULL;
  }
  DDP_TRY(check_ptr(d_out, "out"));
  if (n_aug < 1 || n_aug > DDP_MAX_AUGS || batch < 1 || out_h < 1 || out_w < 1 || !(min_depth <= max_depth)) {
    set_error("depth_postprocess: bad arguments (n_aug %d B %d out %dx%d depth range [%g, %g])", n_aug, batch, out_h, out_w,
              double(min_depth), double(max_depth));
    return DDP_E_BADCFG;
  }
  for (int i = 0; i < n_aug; ++i) {
    const ddp_depth_aug& g = augs[i];
    DDP_TRY(check_ptr(g.d_depth, "aug depth"));
    if (g.h < 1 || g.w < 1 || g.flip < 0 || g.flip > 2) {
      set_error("depth_postprocess: augmentation %d: bad geometry (map %dx%d flip %d)", i, g.h, g.w, g.flip);
      return DDP_E_BADCFG;
    }
  }
  return launch_depth_aug_postprocess(augs, n_aug, batch, out_h, out_w, align_corners ? 1 : 0, min_depth, max_depth, d_out,
                                      static_cast<hipStream_t>(stream));
}

namespace {
struct MsmLayout {
  // weight region first (independent of batch and map sizes: DDP_NECK_WEIGHTS_READY)
  unsigned short* wsplit;
  unsigned char* stream[4];   // per level: its 256 x 256 block of the 1x1 conv as 8 wide stage images
  // activations
  float* a[4];                // level inputs, fp32 fragment-major
  float* y[4];                // per-level conv outputs at the level's own resolution (y[0]: the merged map)
  double* partial;
  float* stats;
  size_t wbytes, abytes, bytes;
};
// weights are carved from wbase, activations from abase (nullptr: sizes only); o->wbytes / o->abytes = the two region sizes
static int msm_layout(int batch, const int* lh, const int* lw, char* wbase, char* abase, MsmLayout* o) {
  if (batch < 1 || !lh || !lw) {
    set_error("neck_msm: bad arguments");
    return DDP_E_BADCFG;
  }
  for (int l = 0; l < 4; ++l)
    if (lh[l] < 1 || lw[l] < 1) {
      set_error("neck_msm: level %d has size %dx%d", l, lh[l], lw[l]);
      return DDP_E_BADCFG;
    }
  Carver wv{wbase}, av{abase};
  o->wsplit = wv.take<unsigned short>(size_t(3) * 256 * 256);
  for (int l = 0; l < 4; ++l) o->stream[l] = wv.take<unsigned char>(size_t(8) * b3_stage_bytes());
  o->wbytes = wv.off;
  for (int l = 0; l < 4; ++l) {
    const size_t M = size_t(batch) * lh[l] * lw[l], Mp = (M + 255) / 256 * 256;
    o->a[l] = av.take<float>(Mp * 256);
    o->y[l] = av.take<float>(Mp * 256);
  }
  const size_t chunks = (size_t(lh[0]) * lw[0] + 31) / 32;   // (32-token chunks: the merging kernel writes the statistics itself)
  o->partial = av.take<double>(size_t(batch) * chunks * 64);
  o->stats = av.take<float>(size_t(batch) * 64);
  o->abytes = av.off;
  o->bytes = o->wbytes + o->abytes;
  return DDP_OK;
}
}  // namespace

int ddp_neck_msm_workspace(int batch, const int* level_h, const int* level_w, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  MsmLayout o;
  DDP_TRY(msm_layout(batch, level_h, level_w, nullptr, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

namespace {
// the merging itself on fp32 fragment-major level inputs a[0..3] (see ddp_neck_msm)
// (a_nchw: the level inputs are the caller's NCHW tensors, read in place by the stream GEMM - no layout conversion)
int msm_core(const float* const* a_blk, const int* level_h, const int* level_w, int batch, const float* d_conv_w, const float* d_gn_w,
             const float* d_gn_b, int align_corners, int flags, float* d_out, const MsmLayout& o, hipStream_t st, bool a_nchw = false) {
  const int N = level_h[0] * level_w[0];
  if (!(flags & DDP_NECK_WEIGHTS_READY))
    for (int l = 0; l < 4; ++l) {
      DDP_TRY(launch_split_weights(d_conv_w + 256 * l, 1024, 256, 256, o.wsplit, st));
      DDP_TRY(launch_build_stages(o.wsplit, size_t(256) * 256, 256, 256, 0, 1, 8, 0, 2, 1, 0, o.stream[l], st));
    }
  SgemmProblem pr[4];
  for (int l = 0; l < 4; ++l) {
    pr[l].A = a_blk[l];
    pr[l].out = o.y[l];
    pr[l].stream = o.stream[l];
    pr[l].M = batch * level_h[l] * level_w[l];
    pr[l].ns = 8;
    pr[l].conv_h = pr[l].conv_w = 0;
    pr[l].bias = nullptr;
    pr[l].gn_partial = nullptr;                            // (GroupNorm acts on the SUM of the resized level outputs)
    pr[l].gn_N = 0;
    pr[l].nchw_N = a_nchw ? level_h[l] * level_w[l] : 0;
  }
  DDP_TRY(launch_b3_sgemm(pr, 4, 0, 0, st));               // all four levels in one persistent launch
  const float* yl[3] = {o.y[1], o.y[2], o.y[3]};
  DDP_TRY(launch_msm_sum_blk(o.y[0], yl, level_h + 1, level_w + 1, batch, level_h[0], level_w[0], align_corners ? 1 : 0, st, o.partial));
  if (N % 32 == 0) DDP_TRY(launch_gn_final32(o.partial, o.stats, batch, N, 1e-5f, st));      // (statistics fused into the merging kernel)
  else DDP_TRY(launch_gn_stats_blk(o.y[0], o.partial, o.stats, batch, N, 1e-5f, st));
  return launch_gn_apply_nchw_blk(o.y[0], o.stats, d_gn_w, d_gn_b, d_out, batch, N, st);
}
}  // namespace

int ddp_neck_msm(const float* const* d_levels, const int* level_h, const int* level_w, int batch, const float* d_conv_w,
                 const float* d_gn_w, const float* d_gn_b, int align_corners, int flags, float* d_out, void* d_workspace,
                 void* stream) {
  if (!d_levels) {
    set_error("levels is NULL");
    return DDP_E_NULL;
  }
  for (int l = 0; l < 4; ++l) DDP_TRY(check_ptr(d_levels[l], "level"));
  DDP_TRY(check_ptr(d_conv_w, "conv weight"));
  DDP_TRY(check_ptr(d_gn_w, "gn weight"));
  DDP_TRY(check_ptr(d_gn_b, "gn bias"));
  DDP_TRY(check_ptr(d_out, "out"));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  if (flags & ~DDP_NECK_WEIGHTS_READY) {
    set_error("neck_msm: unknown flags 0x%x", flags);
    return DDP_E_BADCFG;
  }
  MsmLayout o;
  DDP_TRY(msm_layout(batch, level_h, level_w, nullptr, nullptr, &o));
  DDP_TRY(msm_layout(batch, level_h, level_w, static_cast<char*>(d_workspace), static_cast<char*>(d_workspace) + o.wbytes, &o));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // The 1x1 conv over the concatenation of the four resized levels is linear: it equals the sum over the levels of the
  // bilinear resize of (that level's 256-column block of the weight applied at the level's OWN resolution).  Levels 1..3 are
  // 4x / 16x / 64x smaller than level 0, so the contraction shrinks from 4 to 1.33 level-0 maps and the 1024-channel
  // concatenation (6 KiB per token as a split operand) is never built.
  return msm_core(d_levels, level_h, level_w, batch, d_conv_w, d_gn_w, d_gn_b, align_corners, flags, d_out, o, st, true);
}

namespace {
struct FpnLayout {
  // weight region first (sizes depend on the level channels only: DDP_NECK_WEIGHTS_READY)
  float* wpack;
  unsigned short* wsplit;
  unsigned char* lat_stream[4];   // lateral 1x1 conv: C_l / 32 wide stage images
  unsigned char* out_stream[4];   // 3x3 output conv: 72 stage images (tap, 32-channel block)
  // activations, fp32 fragment-major
  float* a[4];                    // level inputs (C_l channels)
  float* y[4];                    // lateral conv output, later the 3x3 conv output
  float* lat[4];                  // laterals after GroupNorm + top-down add
  double* partial[4];             // per level: GroupNorm partial sums (chunks of 32 tokens when fused into the GEMM, else 256)
  float* stats[4];
  size_t wbytes, abytes, bytes;
};
// weights are carved from wbase, activations from abase (nullptr: sizes only); o->wbytes / o->abytes = the two region sizes
static int fpn_layout(const ddp_fpn_level* lv, int batch, char* wbase, char* abase, FpnLayout* o) {
  if (!lv || batch < 1) {
    set_error("neck_fpn: bad arguments");
    return DDP_E_BADCFG;
  }
  Carver wv{wbase}, av{abase};
  size_t max_w = 2304;
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = lv[l];
    if (v.h < 1 || v.w < 1 || v.in_channels < 64 || v.in_channels % 32 || v.in_channels > 4096) {
      set_error("neck_fpn: level %d: %d channels, %dx%d (channels must be a multiple of 32 in [64, 4096])", l, v.in_channels, v.h, v.w);
      return DDP_E_BADCFG;
    }
    if (size_t(v.in_channels) > max_w) max_w = v.in_channels;
  }
  o->wpack = wv.take<float>(size_t(256) * max_w);
  o->wsplit = wv.take<unsigned short>(size_t(3) * 256 * max_w);
  for (int l = 0; l < 4; ++l) {
    o->lat_stream[l] = wv.take<unsigned char>(size_t(lv[l].in_channels / 32) * b3_stage_bytes());
    o->out_stream[l] = wv.take<unsigned char>(size_t(72) * b3_stage_bytes());
  }
  o->wbytes = wv.off;
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = lv[l];
    const size_t M = size_t(batch) * v.h * v.w, Mp = (M + 255) / 256 * 256;
    o->a[l] = av.take<float>(Mp * v.in_channels);
    o->y[l] = av.take<float>(Mp * 256);
    o->lat[l] = av.take<float>(Mp * 256);
    o->stats[l] = av.take<float>(size_t(batch) * 64);
    o->partial[l] = av.take<double>(size_t(batch) * ((size_t(v.h) * v.w + 31) / 32) * 64);
  }
  o->abytes = av.off;
  o->bytes = o->wbytes + o->abytes;
  return DDP_OK;
}
}  // namespace

int ddp_neck_fpn_workspace(const ddp_fpn_level* levels, int batch, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  FpnLayout o;
  DDP_TRY(fpn_layout(levels, batch, nullptr, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

namespace {
// d_out != nullptr: the four outputs as NCHW tensors; else they stay fp32 fragment-major in o.lat[l] (consumed by msm_core)
int fpn_core(const ddp_fpn_level* levels, int batch, const float* const* d_in, float* const* d_out, int flags, const FpnLayout& o,
             hipStream_t st) {
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = levels[l];
    DDP_TRY(check_ptr(d_in[l], "level input"));
    if (d_out) DDP_TRY(check_ptr(d_out[l], "level output"));
    DDP_TRY(check_ptr(v.lat_w, "lateral weight"));
    DDP_TRY(check_ptr(v.out_w, "fpn conv weight"));
  }
  // weights -> stage images of the stream GEMM (once per set of weights: DDP_NECK_WEIGHTS_READY skips this)
  if (!(flags & DDP_NECK_WEIGHTS_READY))
    for (int l = 0; l < 4; ++l) {
      const ddp_fpn_level& v = levels[l];
      const int C = v.in_channels;
      DDP_TRY(launch_split_weights(v.lat_w, C, 256, C, o.wsplit, st));
      DDP_TRY(launch_build_stages(o.wsplit, size_t(256) * C, C, 256, 0, 1, C / 32, 0, 2, 1, 0, o.lat_stream[l], st));
      DDP_TRY(launch_pack_conv3x3_scaled(v.out_w, nullptr, o.wpack, 256, 256, st));
      DDP_TRY(launch_split_weights(o.wpack, 2304, 256, 2304, o.wsplit, st));
      DDP_TRY(launch_build_stages(o.wsplit, size_t(256) * 2304, 2304, 256, 0, 1, 72, 0, 2, 1, 0, o.out_stream[l], st));
    }
  // laterals (fpn.py:167-171): 1x1 conv of all four levels in ONE persistent launch of the stream GEMM (k_layer MODE 5; the
  // coarse levels have few tiles of many stages: longest tiles first), GroupNorm statistics per level
  SgemmProblem pr[4];
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = levels[3 - l];
    pr[l].A = d_in[3 - l];                                  // the backbone's NCHW level, read in place (k_layer MODE 5, nchw_N)
    pr[l].nchw_N = v.h * v.w;
    pr[l].out = o.y[3 - l];
    pr[l].stream = o.lat_stream[3 - l];
    pr[l].M = batch * v.h * v.w;
    pr[l].ns = v.in_channels / 32;
    pr[l].conv_h = pr[l].conv_w = 0;
    pr[l].bias = nullptr;
    // GroupNorm partial sums in the GEMM epilogue when a wave's 32 tokens cannot straddle two images
    pr[l].gn_N = v.h * v.w;
    pr[l].gn_partial = (v.h * v.w) % 32 == 0 ? o.partial[3 - l] : nullptr;
  }
  DDP_TRY(launch_b3_sgemm(pr, 4, 0, 0, st));
  // GroupNorm + top-down path (:173-185): lat_l = GN(y_l) + nearest_up(lat_{l+1}), coarsest level first, one kernel per level
  // (the statistics of all four levels are finalised by ONE launch when the GEMM epilogue wrote every level's partial sums)
  bool all32 = true;
  int Nl[4];
  for (int l = 0; l < 4; ++l) {
    Nl[l] = levels[l].h * levels[l].w;
    all32 = all32 && Nl[l] % 32 == 0;
  }
  if (all32) DDP_TRY(launch_gn_final32_multi(o.partial, o.stats, Nl, 4, batch, 1e-5f, st));
  for (int l = 3; l >= 0; --l) {
    const ddp_fpn_level& v = levels[l];
    if (all32) {
    } else if ((v.h * v.w) % 32 == 0) DDP_TRY(launch_gn_final32(o.partial[l], o.stats[l], batch, v.h * v.w, 1e-5f, st));
    else DDP_TRY(launch_gn_stats_blk(o.y[l], o.partial[l], o.stats[l], batch, v.h * v.w, 1e-5f, st));
    DDP_TRY(launch_gn_apply_add_blk(o.y[l], o.stats[l], v.lat_gn_w, v.lat_gn_b, l < 3 ? o.lat[l + 1] : nullptr, o.lat[l], batch, v.h,
                                    v.w, l < 3 ? levels[l + 1].h : 1, l < 3 ? levels[l + 1].w : 1, st));
  }
  // outputs (:189-191): 3x3 conv as an implicit GEMM (72 stage images = (tap, 32-channel block); the A fragments of a stage
  // are the fp32 quads of the token shifted by the tap, zero padding), all four levels in one launch, then GroupNorm
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = levels[l];
    pr[l].A = o.lat[l];
    pr[l].out = o.y[l];
    pr[l].stream = o.out_stream[l];
    pr[l].M = batch * v.h * v.w;
    pr[l].ns = 72;
    pr[l].conv_h = v.h;
    pr[l].conv_w = v.w;
    pr[l].nchw_N = 0;
    pr[l].gn_N = v.h * v.w;
    pr[l].gn_partial = (v.h * v.w) % 32 == 0 ? o.partial[l] : nullptr;
  }
  DDP_TRY(launch_b3_sgemm(pr, 4, 0, 1, st));
  if (all32) DDP_TRY(launch_gn_final32_multi(o.partial, o.stats, Nl, 4, batch, 1e-5f, st));
  for (int l = 0; l < 4; ++l) {
    const ddp_fpn_level& v = levels[l];
    if (all32) {
    } else if ((v.h * v.w) % 32 == 0) DDP_TRY(launch_gn_final32(o.partial[l], o.stats[l], batch, v.h * v.w, 1e-5f, st));
    else DDP_TRY(launch_gn_stats_blk(o.y[l], o.partial[l], o.stats[l], batch, v.h * v.w, 1e-5f, st));
    if (d_out) DDP_TRY(launch_gn_apply_nchw_blk(o.y[l], o.stats[l], v.out_gn_w, v.out_gn_b, d_out[l], batch, v.h * v.w, st));
    else       // (the laterals are dead once the convolution has run: their buffers take the normalised outputs)
      DDP_TRY(launch_gn_apply_add_blk(o.y[l], o.stats[l], v.out_gn_w, v.out_gn_b, nullptr, o.lat[l], batch, v.h, v.w, 1, 1, st));
  }
  return DDP_OK;
}
}  // namespace

int ddp_neck_fpn(const ddp_fpn_level* levels, int batch, const float* const* d_in, float* const* d_out, int flags, void* d_workspace,
                 void* stream) {
  if (!d_in || !d_out) {
    set_error("neck_fpn: in / out is NULL");
    return DDP_E_NULL;
  }
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  if (flags & ~DDP_NECK_WEIGHTS_READY) {
    set_error("neck_fpn: unknown flags 0x%x", flags);
    return DDP_E_BADCFG;
  }
  FpnLayout o;
  DDP_TRY(fpn_layout(levels, batch, nullptr, nullptr, &o));
  DDP_TRY(fpn_layout(levels, batch, static_cast<char*>(d_workspace), static_cast<char*>(d_workspace) + o.wbytes, &o));
  return fpn_core(levels, batch, d_in, d_out, flags, o, static_cast<hipStream_t>(stream));
}

// FPN followed by MultiStageMerging, as every DDP config chains them (configs/ade/ddp_swin_t_2x8_512x512_160k_ade20k.py neck list):
// the four FPN outputs stay fp32 fragment-major and feed the merging directly - their NCHW form (one write by FPN, one read
// and re-layout by the merging per level) is never produced.
int ddp_neck_fpn_msm_workspace(const ddp_fpn_level* levels, int batch, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  FpnLayout f;
  DDP_TRY(fpn_layout(levels, batch, nullptr, nullptr, &f));
  int lh[4], lw[4];
  for (int l = 0; l < 4; ++l) {
    lh[l] = levels[l].h;
    lw[l] = levels[l].w;
  }
  MsmLayout m;
  DDP_TRY(msm_layout(batch, lh, lw, nullptr, nullptr, &m));
  *bytes = f.bytes + m.bytes;
  return DDP_OK;
}

int ddp_neck_fpn_msm(const ddp_fpn_level* levels, int batch, const float* const* d_in, const float* d_msm_conv_w,
                     const float* d_msm_gn_w, const float* d_msm_gn_b, int align_corners, int flags, float* d_out, void* d_workspace,
                     void* stream) {
  if (!d_in) {
    set_error("neck_fpn_msm: in is NULL");
    return DDP_E_NULL;
  }
  DDP_TRY(check_ptr(d_msm_conv_w, "msm conv weight"));
  DDP_TRY(check_ptr(d_msm_gn_w, "msm gn weight"));
  DDP_TRY(check_ptr(d_msm_gn_b, "msm gn bias"));
  DDP_TRY(check_ptr(d_out, "out"));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  if (flags & ~DDP_NECK_WEIGHTS_READY) {
    set_error("neck_fpn_msm: unknown flags 0x%x", flags);
    return DDP_E_BADCFG;
  }
  // workspace = [FPN weights | MSM weights | FPN activations | MSM activations]: both weight regions at offsets that do not
  // depend on the geometry (DDP_NECK_WEIGHTS_READY survives a change of batch / map size)
  FpnLayout f;
  DDP_TRY(fpn_layout(levels, batch, nullptr, nullptr, &f));
  int lh[4], lw[4];
  for (int l = 0; l < 4; ++l) {
    lh[l] = levels[l].h;
    lw[l] = levels[l].w;
  }
  MsmLayout m;
  DDP_TRY(msm_layout(batch, lh, lw, nullptr, nullptr, &m));
  char* wsb = static_cast<char*>(d_workspace);
  const size_t fw = f.wbytes, mw = m.wbytes, fa = f.abytes;
  DDP_TRY(fpn_layout(levels, batch, wsb, wsb + fw + mw, &f));
  DDP_TRY(msm_layout(batch, lh, lw, wsb + fw, wsb + fw + mw + fa, &m));
  hipStream_t st = static_cast<hipStream_t>(stream);
  DDP_TRY(fpn_core(levels, batch, d_in, nullptr, flags, f, st));
  return msm_core(f.lat, lh, lw, batch, d_msm_conv_w, d_msm_gn_w, d_msm_gn_b, align_corners, flags, d_out, m, st);
}

namespace {
struct FcnLayout {
  float *x0, *xb0, *xb1, *wpack, *film, *aff, *logits, *cls_bias;
  unsigned short *a_sb, *wsplit;
  unsigned char* stream;     // stage images of the GEMM being run (72 for a 3x3 conv, 8 for conv_seg)
  int ldl;
  size_t bytes;
};
static int fcn_layout(int maps, int h, int w, int K, char* base, FcnLayout* o) {
  if (maps < 1 || h < 1 || w < 1 || K < 1 || K > 256) {
    set_error("fcn_head: bad geometry (maps %d map %dx%d classes %d)", maps, h, w, K);
    return DDP_E_BADCFG;
  }
  Carver cv{base};
  const size_t M = size_t(maps) * h * w, Mp = (M + 255) / 256 * 256;
  o->ldl = (K + 31) / 32 * 32;
  o->x0 = cv.take<float>(Mp * 256);                    // row-major input (the sampler's concat-conv writes it)
  o->xb0 = cv.take<float>(Mp * 256);                    // fp32 fragment-major activations, ping / pong
  o->xb1 = cv.take<float>(Mp * 256);
  o->a_sb = cv.take<unsigned short>(Mp * 256 * 3);      // (SB staging of the sampler's concat-conv input)
  o->wpack = cv.take<float>(size_t(256) * 2304);
  o->wsplit = cv.take<unsigned short>(size_t(3) * 256 * 2304);
  o->stream = cv.take<unsigned char>(size_t(72) * b3_stage_bytes());
  o->film = cv.take<float>(512);
  o->aff = cv.take<float>(512);
  o->cls_bias = cv.take<float>(256);
  o->logits = cv.take<float>(Mp * o->ldl);
  o->bytes = cv.off;
  return DDP_OK;
}
}  // namespace

int ddp_fcn_head_workspace(int maps, int h, int w, int num_classes, size_t* bytes) {
  DDP_TRY(check_bytes(bytes));
  FcnLayout o;
  DDP_TRY(fcn_layout(maps, h, w, num_classes, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

namespace {
// constants of one head evaluation that depend on (weights, time embedding) only: per conv the 72 stage images of the scaled
// 3x3 weights and the shift vector, conv_seg's 8 images and its padded bias
struct FcnPrepared {
  const unsigned char* conv_stream[8];
  const float* conv_shift[8];
  const unsigned char* cls_stream;
  const float* cls_bias;
};
// one ConvWithTimeModule (fcn_head_with_time.py:205-225): FiLM vector from the time embedding, eval BatchNorm x FiLM folded
// into (scale, shift), the scale folded into the 3x3 weights, those split and laid out as the 72 stage images of the stream
// GEMM.  scratch = o.{film, aff, wpack, wsplit}
int fcn_conv_prepare(const ddp_fcn_conv& c, int i, const float* d_temb, const FcnLayout& o, unsigned char* stream_dst,
                     float* shift_dst, hipStream_t st) {
  DDP_TRY(check_ptr(c.conv_w, "conv weight"));
  if (c.bn_w && (!c.bn_b || !c.bn_mean || !c.bn_var)) {
    set_error("fcn_head: conv %d has an incomplete norm", i);
    return DDP_E_NULL;
  }
  const float* film = nullptr;
  if (d_temb && c.time_w) {      // (:216-221) SiLU -> Linear(1024, 512) -> (scale | shift)
    DDP_TRY(launch_matvec(c.time_w, c.time_b, d_temb, o.film, DDP_TIME_DIM, 512, 1, DDP_TIME_DIM, 512, 2, 0, st));
    film = o.film;
  }
  DDP_TRY(launch_fcn_fold(c.bn_w, c.bn_b, c.bn_mean, c.bn_var, c.bn_eps, c.conv_b, film, o.aff, shift_dst, st));
  DDP_TRY(launch_pack_conv3x3_scaled(c.conv_w, o.aff, o.wpack, 256, 256, st));
  DDP_TRY(launch_split_weights(o.wpack, 2304, 256, 2304, o.wsplit, st));
  return launch_build_stages(o.wsplit, size_t(256) * 2304, 2304, 256, 0, 1, 72, 0, 2, 1, 0, stream_dst, st);
}
// bn_w and bn_b set, both running statistics NULL: a GroupNorm(32, 256) convolution (include/ddp_mi355x.h, ddp_fcn_conv)
inline bool fcn_conv_is_gn(const ddp_fcn_conv& c) { return c.bn_w && c.bn_b && !c.bn_mean && !c.bn_var; }
// GroupNorm scratch of one head evaluation, inside FcnLayout::a_sb (dead while the head's convolutions run: nothing of the
// head reads it and the sampler stages its concat-conv input in its own in_sb): the fp64 partial sums first - 16 B per token
// on the fused route, 512 B per 256-token chunk of a map otherwise, either way <= 512 Mp bytes - then {mean, rstd} per
// (map, group), 256 B per map <= 256 Mp bytes; the region holds 1536 Mp bytes
struct FcnGnScratch {
  double* partial;
  float* stats;
};
FcnGnScratch fcn_gn_scratch(const FcnLayout& o, int M) {
  const size_t Mp = (size_t(M) + 255) / 256 * 256;
  char* base = reinterpret_cast<char*>(o.a_sb);
  return {reinterpret_cast<double*>(base), reinterpret_cast<float*>(base + Mp * 512)};
}
// the weight-side constants of a GroupNorm conv: the stage images of the PLAIN 3x3 weights and the accumulator bias (conv
// bias or zeros) - neither depends on the time embedding.  scratch = o.{wpack, wsplit}
int fcn_gn_conv_prepare(const ddp_fcn_conv& c, const FcnLayout& o, unsigned char* stream_dst, float* bias_dst, hipStream_t st) {
  DDP_TRY(check_ptr(c.conv_w, "conv weight"));
  DDP_TRY(launch_pack_conv3x3_scaled(c.conv_w, nullptr, o.wpack, 256, 256, st));
  DDP_TRY(launch_split_weights(o.wpack, 2304, 256, 2304, o.wsplit, st));
  DDP_TRY(launch_build_stages(o.wsplit, size_t(256) * 2304, 2304, 256, 0, 1, 72, 0, 2, 1, 0, stream_dst, st));
  const hipError_t e = c.conv_b ? hipMemcpyAsync(bias_dst, c.conv_b, 256 * sizeof(float), hipMemcpyDeviceToDevice, st)
                                : hipMemsetAsync(bias_dst, 0, 256 * sizeof(float), st);
  if (e != hipSuccess) {
    set_error("fcn_head: GroupNorm conv bias copy failed");
    return DDP_E_LAUNCH;
  }
  return DDP_OK;
}
// conv_seg (cls_seg; dropout is the identity in eval mode): 1x1, the class rows zero-padded to the GEMM's 256 outputs
int fcn_cls_prepare(const float* d_cls_w, const float* d_cls_b, int num_classes, const FcnLayout& o, unsigned char* stream_dst,
                    float* bias_dst, hipStream_t st) {
  DDP_TRY(launch_split_weights(d_cls_w, 256, num_classes, 256, o.wsplit, st));
  DDP_TRY(launch_build_stages(o.wsplit, size_t(num_classes) * 256, 256, num_classes, 0, 1, 8, 0, 2, 1, 0, stream_dst, st));
  if (hipMemsetAsync(bias_dst, 0, 256 * sizeof(float), st) != hipSuccess ||
      (d_cls_b && hipMemcpyAsync(bias_dst, d_cls_b, size_t(num_classes) * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)) {
    set_error("fcn_head: conv_seg bias copy failed");
    return DDP_E_LAUNCH;
  }
  return DDP_OK;
}

// FCNHeadWithTime on token-major rows: o.x0 (M,256) in -> o.logits (M, ldl) (fcn_head_with_time.py:285-305, eval mode).  Inside,
// the activations are fp32 fragment-major and every convolution runs on the persistent stream GEMM (k_layer MODE 5): the 3x3
// ones as implicit GEMMs of 72 stages with the folded norm x FiLM shift as bias and ReLU in the epilogue, conv_seg as 8 stages.
// `prep`: the weight-side constants built beforehand (the sampler loop: ddp_prepare_fcn); NULL: the time embedding is a
// run-time input (ddp_fcn_head_forward) and they are built here, one conv at a time through the workspace's single stream
// buffer (conv i's images are consumed - stream order - before conv i + 1's are written).
// A GroupNorm conv (fcn_conv_is_gn) cannot fold its norm into the weights - the statistics are of the activations: plain GEMM with
// the statistics fused into its epilogue where h * w % 32 == 0, then k_gn_film_relu_blk in place (ddp_fcn_gn.hip).
int fcn_head_tokens(const ddp_fcn_conv* convs, int num_convs, int dilation, const float* d_cls_w, const float* d_cls_b,
                    int num_classes, const float* d_temb, int maps, int h, int w, const FcnLayout& o, hipStream_t st,
                    const FcnPrepared* prep = nullptr) {
  const int N = h * w, M = maps * N;
  DDP_TRY(launch_row_to_blk(o.x0, o.xb0, M, st));
  float* cur = o.xb0;
  float* nxt = o.xb1;
  SgemmProblem pr;
  pr.gn_partial = nullptr;
  pr.gn_N = 0;
  pr.nchw_N = 0;
  pr.M = M;
  for (int i = 0; i < num_convs; ++i) {
    const bool gn = fcn_conv_is_gn(convs[i]);
    if (!prep) {
      if (gn) DDP_TRY(fcn_gn_conv_prepare(convs[i], o, o.stream, o.aff + 256, st));
      else DDP_TRY(fcn_conv_prepare(convs[i], i, d_temb, o, o.stream, o.aff + 256, st));
    }
    pr.A = cur;
    pr.out = nxt;
    pr.stream = prep ? prep->conv_stream[i] : o.stream;
    pr.ns = 72;
    pr.conv_h = h;
    pr.conv_w = w;
    pr.bias = prep ? prep->conv_shift[i] : o.aff + 256;
    if (gn) {
      // GroupNorm: plain convolution (+ bias, inside the accumulators the fused statistics are formed from) -> statistics per
      // map -> one in-place pass norm x FiLM + ReLU.  The FiLM vector is evaluated here, also in the sampler loop: it needs
      // 512 floats per (step, conv), conv_shifts holds 256.
      const float* film = nullptr;
      if (d_temb && convs[i].time_w) {
        DDP_TRY(launch_matvec(convs[i].time_w, convs[i].time_b, d_temb, o.film, DDP_TIME_DIM, 512, 1, DDP_TIME_DIM, 512, 2, 0, st));
        film = o.film;
      }
      const FcnGnScratch gs = fcn_gn_scratch(o, M);
      const bool fused = N % 32 == 0;
      pr.gn_partial = fused ? gs.partial : nullptr;
      pr.gn_N = fused ? N : 0;
      DDP_TRY(launch_b3_sgemm(&pr, 1, 0, dilation, st));
      pr.gn_partial = nullptr;
      pr.gn_N = 0;
      if (fused) DDP_TRY(launch_gn_final32(gs.partial, gs.stats, maps, N, convs[i].bn_eps, st));
      else DDP_TRY(launch_gn_stats_blk(nxt, gs.partial, gs.stats, maps, N, convs[i].bn_eps, st));
      DDP_TRY(launch_gn_film_relu_blk(nxt, gs.stats, convs[i].bn_w, convs[i].bn_b, film, maps, N, st));
    } else {
      DDP_TRY(launch_b3_sgemm(&pr, 1, 2, dilation, st));
    }
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (!prep) DDP_TRY(fcn_cls_prepare(d_cls_w, d_cls_b, num_classes, o, o.stream, o.cls_bias, st));
  pr.A = cur;
  pr.out = nxt;
  pr.stream = prep ? prep->cls_stream : o.stream;
  pr.ns = 8;
  pr.conv_h = pr.conv_w = 0;
  pr.bias = prep ? prep->cls_bias : o.cls_bias;
  DDP_TRY(launch_b3_sgemm(&pr, 1, 0, 0, st));
  return launch_blk_to_row(nxt, o.logits, M, st, o.ldl, o.ldl);
}

// sampler loop around the FCN head: the head's own workspace first, then the loop's buffers, then the caller-visible tail
// (the step-record and seeded-noise groups of carve_caller_regions)
struct FcnLoopLayout : CallerRegions {
  FcnLayout head;
  float *tin, *u, *hid, *temb, *lut, *wx, *wm, *xtok, *xproj, *mask, *prob, *snoise;
  unsigned short *wx_split, *wm_split, *in_sb;
  // what ddp_prepare_fcn leaves behind for ddp_sample_fcn (besides temb, lut, wx_split, wm_split): per (step, conv) the stage
  // images of the FiLM-scaled 3x3 weights and the shift vector; conv_seg's images and padded bias
  unsigned char *conv_streams, *cls_stream;
  float *conv_shifts, *cls_bias;
  size_t bytes;
};
int fcn_loop_layout(const ddp_cfg* c, int num_convs, char* base, FcnLoopLayout* o) {
  const int R = c->batch * c->randsteps, N = c->h * c->w, Kc = c->num_classes, Cx = c->feat_channels;
  DDP_TRY(fcn_layout(R, c->h, c->w, Kc, base, &o->head));
  Carver cv{base, o->head.bytes};
  const size_t M = size_t(R) * N, Mp = (M + 255) / 256 * 256, MB = size_t(c->batch) * N, MBp = (MB + 255) / 256 * 256;
  o->tin = cv.take<float>(DDP_MAX_STEPS);
  o->u = cv.take<float>(size_t(c->timesteps) * DDP_SINU_FEATS);
  o->hid = cv.take<float>(size_t(c->timesteps) * DDP_TIME_DIM);
  o->temb = cv.take<float>(size_t(c->timesteps) * DDP_TIME_DIM);
  o->lut = cv.take<float>(size_t(Kc + 1) * 256);
  o->wx = cv.take<float>(size_t(256) * Cx);
  o->wm = cv.take<float>(size_t(256) * 256);
  o->wx_split = cv.take<unsigned short>(size_t(3) * 256 * Cx);
  o->wm_split = cv.take<unsigned short>(size_t(3) * 256 * 256);
  o->xtok = cv.take<float>(MB * Cx);
  o->xproj = cv.take<float>(MB * 256);
  o->mask = cv.take<float>(M * 256);
  o->prob = cv.take<float>(M * o->head.ldl);
  o->snoise = cv.take<float>(c->sampler == DDP_SAMPLER_DDPM ? M * 256 : 0);
  const size_t sb_a = MBp * Cx, sb_b = Mp * 256;
  o->in_sb = cv.take<unsigned short>((sb_a > sb_b ? sb_a : sb_b) * 3);
  const size_t per_conv = size_t(72) * b3_stage_bytes();
  o->conv_streams = cv.take<unsigned char>(size_t(c->timesteps) * num_convs * per_conv);
  o->conv_shifts = cv.take<float>(size_t(c->timesteps) * (num_convs > 0 ? num_convs : 1) * 256);
  o->cls_stream = cv.take<unsigned char>(size_t(8) * b3_stage_bytes());
  o->cls_bias = cv.take<float>(256);
  carve_caller_regions(c, cv, o);
  o->bytes = cv.off;
  return DDP_OK;
}
// a GroupNorm conv's images and bias do not depend on the step: its slot of step 0 serves every step (its other slots stay unused)
FcnPrepared fcn_prepared_of(const FcnLoopLayout& o, const ddp_fcn_conv* convs, int num_convs, int step) {
  FcnPrepared p;
  const size_t per_conv = size_t(72) * b3_stage_bytes();
  for (int i = 0; i < 8; ++i) {
    const bool live = i < num_convs;
    const size_t slot = live ? size_t(fcn_conv_is_gn(convs[i]) ? 0 : step) * num_convs + i : 0;
    p.conv_stream[i] = live ? o.conv_streams + slot * per_conv : nullptr;
    p.conv_shift[i] = live ? o.conv_shifts + slot * 256 : nullptr;
  }
  p.cls_stream = o.cls_stream;
  p.cls_bias = o.cls_bias;
  return p;
}
int validate_fcn_loop(const ddp_cfg* cfg, int num_convs, int dilation) {
  if (!cfg) {
    set_error("cfg is NULL");
    return DDP_E_NULL;
  }
  ddp_cfg c = *cfg;
  c.num_layers = 1;                       // the encoder depth is meaningless here
  c.flags &= ~DDP_FLAG_FCN_PREPARED;      // this loop's own flag (ddp_sample rejects it)
  DDP_TRY(validate(&c));
  if (cfg->task != DDP_TASK_SEG || cfg->head_h != cfg->h || cfg->head_w != cfg->w) {
    set_error("sample_fcn: segmentation only (FCNHeadWithTime is a segmentation head)");
    return DDP_E_BADCFG;
  }
  if (cfg->flags & DDP_FLAG_DDPM_CHAIN) {
    set_error("sample_fcn: DDP_FLAG_DDPM_CHAIN is a route of ddp_sample (the FCN loop has no u chain)");
    return DDP_E_BADCFG;
  }
  if (cfg->flags & DDP_FLAG_X0_HINTS) {
    set_error("sample_fcn: DDP_FLAG_X0_HINTS is built for ddp_sample only (the FCN loop takes no hints)");
    return DDP_E_BADCFG;
  }
  if (cfg->flags & DDP_FLAG_PRIOR_START) {
    set_error("sample_fcn: DDP_FLAG_PRIOR_START is built for ddp_sample only (the FCN loop starts from noise)");
    return DDP_E_BADCFG;
  }
  if (cfg->flags & DDP_FLAG_CLASS_PRIOR) {
    set_error("sample_fcn: DDP_FLAG_CLASS_PRIOR is built for ddp_sample only (the FCN loop takes no class prior)");
    return DDP_E_BADCFG;
  }
  if (cfg->flags & DDP_FLAG_SCORE_PRIOR) {
    set_error("sample_fcn: DDP_FLAG_SCORE_PRIOR is built for ddp_sample only (the FCN loop takes no score prior)");
    return DDP_E_BADCFG;
  }
  if (num_convs < 0 || num_convs > 8 || dilation < 1) {
    set_error("sample_fcn: num_convs %d / dilation %d out of range", num_convs, dilation);
    return DDP_E_BADCFG;
  }
  return DDP_OK;
}
}  // namespace

int ddp_fcn_head_forward(const ddp_fcn_conv* convs, int num_convs, int dilation, const float* d_cls_w, const float* d_cls_b,
                         int num_classes, const float* d_feat, const float* d_temb, int maps, int h, int w, float* d_out,
                         void* d_workspace, void* stream) {
  if (num_convs < 0 || num_convs > 8 || dilation < 1 || (num_convs > 0 && !convs)) {
    set_error("fcn_head: num_convs %d / dilation %d out of range", num_convs, dilation);
    return DDP_E_BADCFG;
  }
  DDP_TRY(check_ptr(d_cls_w, "conv_seg weight"));
  DDP_TRY(check_ptr(d_feat, "feat"));
  DDP_TRY(check_ptr(d_out, "out"));
  DDP_TRY(check_ptr(d_workspace, "workspace"));
  FcnLayout o;
  DDP_TRY(fcn_layout(maps, h, w, num_classes, static_cast<char*>(d_workspace), &o));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = h * w;
  DDP_TRY(launch_nchw_to_tok(d_feat, o.x0, maps, 256, N, st));
  DDP_TRY(fcn_head_tokens(convs, num_convs, dilation, d_cls_w, d_cls_b, num_classes, d_temb, maps, h, w, o, st));
  return launch_finalize_nchw(o.logits, o.ldl, d_out, maps, 1, N, num_classes, 1.0f, st);
}

int ddp_sample_fcn_workspace(const ddp_cfg* cfg, int num_convs, int dilation, size_t* bytes) {
  DDP_TRY(validate_fcn_loop(cfg, num_convs, dilation));
  DDP_TRY(check_bytes(bytes));
  FcnLoopLayout o;
  DDP_TRY(fcn_loop_layout(cfg, num_convs, nullptr, &o));
  *bytes = o.bytes;
  return DDP_OK;
}

namespace {
int check_fcn_loop_args(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, int dilation,
                        const ddp_step* steps, const void* d_workspace) {
  DDP_TRY(validate_fcn_loop(cfg, num_convs, dilation));
  if (!weights || !steps || (num_convs > 0 && !convs)) {
    set_error("sample_fcn: weights / steps / convs is NULL");
    return DDP_E_NULL;
  }
  DDP_TRY(check_ptr(weights->transform_w, "transform_w"));
  DDP_TRY(check_ptr(weights->transform_b, "transform_b"));
  DDP_TRY(check_ptr(weights->embedding, "embedding"));
  DDP_TRY(check_ptr(weights->head_w, "conv_seg weight"));
  DDP_TRY(check_ptr(weights->time1_w, "time_mlp.1"));
  DDP_TRY(check_ptr(weights->time3_w, "time_mlp.3"));
  return check_ptr(d_workspace, "workspace");
}
int prepare_fcn(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, const ddp_step* steps,
                const FcnLoopLayout& o, hipStream_t st) {
  const int K = cfg->timesteps, Kc = cfg->num_classes, Cx = cfg->feat_channels;
  // time embeddings of every step, x0 LUT, the two column blocks of the concat-conv
  float tin[DDP_MAX_STEPS];
  for (int s = 0; s < K; ++s) tin[s] = steps[s].time_in;
  DDP_TRY(launch_write_floats(tin, K, o.tin, st));
  DDP_TRY(time_embed_dev(weights, 0, o.tin, K, o.u, o.hid, o.temb, nullptr, st));
  DDP_TRY(launch_build_lut(weights->embedding, o.lut, Kc + 1, cfg->bit_scale, st));
  DDP_TRY(launch_pack_cols(weights->transform_w, Cx + 256, 0, 256, Cx, o.wx, st));
  DDP_TRY(launch_pack_cols(weights->transform_w, Cx + 256, Cx, 256, 256, o.wm, st));
  DDP_TRY(launch_split_weights(o.wx, Cx, 256, Cx, o.wx_split, st));
  DDP_TRY(launch_split_weights(o.wm, 256, 256, 256, o.wm_split, st));
  // the head's weight-side constants: one set of scaled-weight images per (step, conv) - the FiLM scale depends on the step
  const size_t per_conv = size_t(72) * b3_stage_bytes();
  // (a GroupNorm conv: plain weights, one set for every step in its slot of step 0; its FiLM vector is evaluated in the loop)
  for (int s = 0; s < K; ++s)
    for (int i = 0; i < num_convs; ++i) {
      unsigned char* images = o.conv_streams + (size_t(s) * num_convs + i) * per_conv;
      float* shift = o.conv_shifts + (size_t(s) * num_convs + i) * 256;
      if (!fcn_conv_is_gn(convs[i])) DDP_TRY(fcn_conv_prepare(convs[i], i, o.temb + size_t(s) * DDP_TIME_DIM, o.head, images, shift, st));
      else if (s == 0) DDP_TRY(fcn_gn_conv_prepare(convs[i], o.head, images, shift, st));
    }
  return fcn_cls_prepare(weights->head_w, weights->head_b, Kc, o.head, o.cls_stream, o.cls_bias, st);
}
}  // namespace

int ddp_prepare_fcn(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, int dilation,
                    const ddp_step* steps, void* d_workspace, void* stream) {
  DDP_TRY(check_fcn_loop_args(cfg, weights, convs, num_convs, dilation, steps, d_workspace));
  FcnLoopLayout o;
  DDP_TRY(fcn_loop_layout(cfg, num_convs, static_cast<char*>(d_workspace), &o));
  return prepare_fcn(cfg, weights, convs, num_convs, steps, o, static_cast<hipStream_t>(stream));
}

int ddp_sample_fcn(const ddp_cfg* cfg, const ddp_weights* weights, const ddp_fcn_conv* convs, int num_convs, int dilation,
                   const ddp_step* steps, const float* d_x, const float* d_noise, const float* d_step_noise, float* d_out,
                   void* d_workspace, void* stream) {
  DDP_TRY(check_fcn_loop_args(cfg, weights, convs, num_convs, dilation, steps, d_workspace));
  DDP_TRY(check_ptr(d_x, "x"));
  DDP_TRY(check_ptr(d_noise, "noise"));
  DDP_TRY(check_ptr(d_out, "out"));
  const bool seeded = (cfg->flags & DDP_FLAG_SEEDED_NOISE) != 0;
  if (cfg->sampler == DDP_SAMPLER_DDPM && !seeded) DDP_TRY(check_ptr(d_step_noise, "step_noise"));
  hipStream_t st = static_cast<hipStream_t>(stream);
  FcnLoopLayout o;
  DDP_TRY(fcn_loop_layout(cfg, num_convs, static_cast<char*>(d_workspace), &o));
  const int B = cfg->batch, r = cfg->randsteps, K = cfg->timesteps, Kc = cfg->num_classes, Cx = cfg->feat_channels;
  const int N = cfg->h * cfg->w, R = B * r, M = R * N;
  if (!(cfg->flags & DDP_FLAG_FCN_PREPARED)) DDP_TRY(prepare_fcn(cfg, weights, convs, num_convs, steps, o, st));
  SplitW wpx, wpm;
  wpx.p = o.wx_split;
  wpx.comp_stride = size_t(256) * Cx;
  wpm.p = o.wm_split;
  wpm.comp_stride = size_t(256) * 256;
  // loop-invariant half of the concat-conv (ddp.py:223-224 with the x columns hoisted), start noise -> token-major
  DDP_TRY(launch_nchw_to_tok(d_x, o.xtok, B, Cx, N, st));
  DDP_TRY(launch_row_to_sb(o.xtok, Cx, o.in_sb, B * N, Cx, st));
  DDP_TRY(launch_b3_linear(o.in_sb, wpx, weights->transform_b, nullptr, 0, 0, 0, o.xproj, 256, B * N, 256, Cx, st, TAG_XPROJ));
  const uint32_t* key = nullptr;
  if (seeded) {
    key = reinterpret_cast<const uint32_t*>(d_noise);
    DDP_TRY(seeded_start_noise(key, o.seed_noise, B, size_t(r) * 256 * N, st));
    d_noise = o.seed_noise;
  }
  DDP_TRY(launch_nchw_to_tok(d_noise, o.mask, R, 256, N, st));
  for (int s = 0; s < K; ++s) {
    const ddp_step& sp = steps[s];
    // feat = transform(cat[x, mask_t]) -> the head's token-major input
    DDP_TRY(launch_row_to_sb(o.mask, 256, o.in_sb, M, 256, st));
    DDP_TRY(launch_b3_linear(o.in_sb, wpm, nullptr, o.xproj, 256, r * N, N, o.head.x0, 256, M, 256, 256, st, TAG_XPROJ));
    const FcnPrepared prep = fcn_prepared_of(o, convs, num_convs, s);
    DDP_TRY(fcn_head_tokens(convs, num_convs, dilation, weights->head_w, weights->head_b, Kc, o.temb + size_t(s) * DDP_TIME_DIM, R,
                            cfg->h, cfg->w, o.head, st, &prep));
    SegUpdateArgs a = seg_update_args(o.head.logits, o.head.ldl, Kc, o.lut, o.mask, o.prob, cfg->accumulation ? (s == 0 ? 1 : 2) : 0,
                                      cfg->sampler, sp, M);
    if (cfg->sampler == DDP_SAMPLER_DDPM && sp.ddpm_add_noise) {
      DDP_TRY(stage_step_noise(key, d_step_noise, o.snoise, B, r, N, s, st));
      a.step_noise = o.snoise;
    }
    a.x0_idx = o.step_rec ? o.step_rec + size_t(s) * M : nullptr;
    DDP_TRY(launch_seg_update(a, st));
  }
  if (cfg->accumulation) DDP_TRY(launch_finalize_nchw(o.prob, o.head.ldl, d_out, B, r, N, Kc, float(r * K), st));
  else DDP_TRY(launch_finalize_nchw(o.head.logits, o.head.ldl, d_out, B, r, N, Kc, float(r), st));
  return step_disagreement(cfg, o, 0.f, d_out, st);
}

}  // extern "C"
