"""The configuration sweep shared by tests/test_config_space_gpu.py (GPU: every case against the CPU oracle) and
tests/test_config_space_host.py (CPU: workspace queries, refusals, fp32-vs-fp64 conditioning of the oracle on every case).

``ddp_sample`` picks its kernels from the configuration (``carve()`` / ``plan_of()`` in csrc/ddp_api.hip); the reference-made
fixtures reach only a few of those regions (BEV with 6 classes, seg / depth with 256 feature channels, depth maps of >= 5 rows,
L <= 6, K <= 20, DDPM at B = 1, r = 1).  A case here is a plain dict: a model (task, classes, layers, feature width, seed), a
geometry (B, h, w, r; BEV: the head grid), a schedule and the sampler's options.  Weights and inputs come from
``ddp_amd.utils.synthetic`` ('init' profile), the expectation from ``oracle.ddp_oracle`` - no fixture file is involved.

Sizes: B = 2 or 3 and token counts that are no multiple of 32 (groups and tiles straddle images), except where the case is
about a degenerate size (1 x 1, one row, one column).

``path``: the route the case was written for on the bf16x3 engine with default flags, stated here by hand from reading
``sample_seg`` / ``sample_depth`` / ``sample_bev`` - the GPU test checks it against the library's own launch records:
  seg_head7     first step's head straight from the caller's NCHW tensors (256 feature channels, r = 1), u chain, last layer + tail
  seg_prologue  x-projection GEMM + step-prologue kernel in front of the same chain (Cx != 256 or r > 1)
  depth_chain   GEMM-free step head from the loop invariants (r = 1, L >= 2, the padded map fits the FFN scratch)
  depth_lt      layer-0 projection kernel as the step head (r > 1, L = 1, or the map does not fit), last layer + conv_depth taps
  depth_bins    binned head: layer-0 projection kernel, plain last layer, conv_depth as a stream GEMM
  bev_chain     <= 8 classes: u chain through the 2^Kc-row table, last layer + conv_seg tail
  bev_separate  9 .. 32 classes: concat-conv GEMM, head GEMM and k_bev_update on the 256-channel map per step
A one-row map is NOT by itself a fallback: 1 x 37 and 1 x 1 fit (Mp rounds the token count up to 256, which leaves room for the
3-row padded map) and run the chain; 1 x 127 with B = 2 (254 tokens) is the size that does not."""
import ctypes as C

import torch

from ddp_amd import _lib, schedule
from ddp_amd.utils import synthetic
from golden_util import max_rel
from oracle import ddp_oracle as O
from support import REL  # noqa: F401  (the bar of every parity test against the fp32 reference)

COND = REL / 20         # the fp32 oracle must sit this close to its own fp64 evaluation for REL to apply unchanged
BEV_FUSED_UNFUSED = 5e-5   # tests/test_hip_parity.py::test_fused_and_unfused_step_boundary_depth_bev (the same regrouping)

CASES = {}


def _add(name, family, task, **kw):
    c = dict(name=name, family=family, task=task, B=2, r=1, K=3, L=3, Cx=256, td=1, seed=len(CASES) + 700)
    if task == 'seg':
        c.update(Kc=19, bit_scale=0.01, accumulation=True, sampler='ddim')
    elif task == 'depth':
        c.update(Kc=1, K=4, bit_scale=0.1, min_depth=1e-3, max_depth=80.0, scale_up=False, use_eps=True, n_bins=0, norm='linear')
    else:
        c.update(Kc=6, bit_scale=0.01, threshold=0.5, grid=(7, 9))      # grid: head grid = (h + 7, w + 9)
    c.update(kw)
    assert name not in CASES
    CASES[name] = c


# ---- BEV class count: the u chain (<= 8 classes: code byte + 2^Kc-row table) and the separate kernels (9 .. 32) ----------------
for _kc in (1, 2, 3, 7, 8, 9, 16, 31, 32):
    for _r in (1, 2):
        _add(f'bev_kc{_kc}_r{_r}', 'bev_classes', 'bev', Kc=_kc, r=_r, h=12, w=20, path='bev_chain' if _kc <= 8 else 'bev_separate')
for _kc, _p in ((5, 'bev_chain'), (12, 'bev_separate')):
    for _th in (0.3, 0.7):
        _add(f'bev_kc{_kc}_th{_th}', 'bev_classes', 'bev', Kc=_kc, r=1, h=12, w=20, threshold=_th, path=_p)
    _add(f'bev_kc{_kc}_td2', 'bev_classes', 'bev', Kc=_kc, r=2, h=12, w=20, td=2, K=4, path=_p)
    _add(f'bev_kc{_kc}_small_grid', 'bev_classes', 'bev', Kc=_kc, r=1, h=13, w=21, grid=(-4, -6), B=3, path=_p)   # head grid 9 x 15

# ---- feature width: no head7 stream, x-projection of depth Cx, in_sb / hbuf sized by B.N.Cx -------------------------------------
# 9 x 14 = 126 tokens, B = 2: Mp = 256 at r = 1, so B.N.Cx passes Mp.1024 (hbuf) for Cx >= 1056 and in_rows.256 (in_sb) for
# Cx > 256; at r = 2 (Mp = 512) hbuf keeps Mp.1024 up to Cx = 2048 and in_sb flips only above Cx = 512
for _cx in (32, 96, 512, 1056, 2048):
    for _r in (1, 2):
        _add(f'seg_cx{_cx}_r{_r}', 'feature_width', 'seg', Cx=_cx, r=_r, h=9, w=14, L=2, path='seg_prologue')
for _cx in (32, 512):
    _add(f'depth_cx{_cx}', 'feature_width', 'depth', Cx=_cx, h=9, w=14, L=2, path='depth_chain')
for _cx in (32, 1056):
    _add(f'bev_cx{_cx}', 'feature_width', 'bev', Cx=_cx, h=9, w=14, L=2, path='bev_chain')
_add('depth_cx512_5x7', 'feature_width', 'depth', Cx=512, h=5, w=7, L=2, path='depth_chain')
# r >= 2 with 256 < Cx <= 256 r and few tokens: x (B.N rows of Cx) and the noisy map (r.B.N rows of 256) pad to the SAME 256-row
# tile, so x needs the larger staging buffer although its unpadded product is the smaller one - the region where in_sb was once
# sized from the unpadded products (100 tokens, r = 2, Cx = 512 read 384 KiB past the workspace; 66 tokens, r = 3, Cx = 768 wrote)
_add('seg_cx512_r2_5x10', 'feature_width', 'seg', Cx=512, r=2, h=5, w=10, L=2, path='seg_prologue')
_add('seg_cx768_r3_3x11', 'feature_width', 'seg', Cx=768, r=3, h=3, w=11, L=2, path='seg_prologue')
_add('depth_cx512_r2_5x10', 'feature_width', 'depth', Cx=512, r=2, h=5, w=10, L=2, path='depth_lt')
_add('bev_cx512_r2_5x10', 'feature_width', 'bev', Cx=512, r=2, h=5, w=10, L=2, grid=(-1, -3), path='bev_chain')

# ---- depth step-head fallbacks: one-row / one-column / one-pixel maps, L = 1 (no chain), r = 2 (no chain), binned head ----------
_add('depth_1x37_L3', 'depth_fallbacks', 'depth', h=1, w=37, L=3, B=3, path='depth_chain')
_add('depth_1x37_L2_r2', 'depth_fallbacks', 'depth', h=1, w=37, L=2, r=2, path='depth_lt')
_add('depth_1x127_L2', 'depth_fallbacks', 'depth', h=1, w=127, L=2, path='depth_lt')        # B.w = 254: the padded map does not fit the FFN scratch
_add('depth_1x1_L2', 'depth_fallbacks', 'depth', h=1, w=1, L=2, B=3, path='depth_chain')
_add('depth_1x1_L1_r2', 'depth_fallbacks', 'depth', h=1, w=1, L=1, r=2, path='depth_lt')
_add('depth_23x1_L2', 'depth_fallbacks', 'depth', h=23, w=1, L=2, B=3, path='depth_chain')
_add('depth_23x1_L1_r2', 'depth_fallbacks', 'depth', h=23, w=1, L=1, r=2, path='depth_lt')
_add('depth_9x11_L1', 'depth_fallbacks', 'depth', h=9, w=11, L=1, B=3, path='depth_lt')
_add('depth_9x11_L1_scale_up', 'depth_fallbacks', 'depth', h=9, w=11, L=1, scale_up=True, path='depth_lt')
_add('depth_9x11_L1_no_eps', 'depth_fallbacks', 'depth', h=9, w=11, L=1, use_eps=False, path='depth_lt')
_add('depth_9x11_L1_scale_up_no_eps', 'depth_fallbacks', 'depth', h=9, w=11, L=1, scale_up=True, use_eps=False, path='depth_lt')
_add('depth_9x11_L2_r2', 'depth_fallbacks', 'depth', h=9, w=11, L=2, r=2, path='depth_lt')
_add('depth_1x37_L2_bins', 'depth_fallbacks', 'depth', h=1, w=37, L=2, n_bins=24, norm='softmax', path='depth_bins')
_add('depth_9x11_L1_bins', 'depth_fallbacks', 'depth', h=9, w=11, L=1, n_bins=17, norm='linear', B=3, path='depth_bins')

# ---- the limits validate() accepts: DDP_MAX_LAYERS, DDP_MAX_STEPS, a single step ------------------------------------------------
_add('seg_L12', 'limits', 'seg', L=12, h=7, w=13, path='seg_head7')
_add('depth_L12_r2', 'limits', 'depth', L=12, h=6, w=10, r=2, path='depth_lt')
_add('bev_L12', 'limits', 'bev', L=12, h=6, w=9, grid=(3, 2), path='bev_chain')
_add('seg_K64_L12', 'limits', 'seg', K=64, L=12, h=5, w=6, path='seg_head7')
_add('seg_K64_noacc', 'limits', 'seg', K=64, L=2, h=5, w=6, accumulation=False, path='seg_head7')
_add('depth_K64', 'limits', 'depth', K=64, L=2, h=5, w=6, path='depth_chain')
_add('depth_K1', 'limits', 'depth', K=1, L=2, h=5, w=7, path='depth_chain')
_add('bev_K1', 'limits', 'bev', K=1, L=2, h=6, w=9, grid=(3, 2), path='bev_chain')

# ---- DDPM outside its one fixture: B = 2, r = 2, accumulation on and off --------------------------------------------------------
_add('seg_ddpm_acc', 'ddpm', 'seg', sampler='ddpm', r=2, h=7, w=13, L=2)
_add('seg_ddpm_noacc', 'ddpm', 'seg', sampler='ddpm', r=2, h=7, w=13, L=2, accumulation=False)

# the "previously verified" configuration sampled through a fresh engine after every feature-width call: the smoke test's model
# at a small odd size (the golden fixtures and test_sample_edge_geometry_vs_oracle cover this region)
CANARY = dict(name='canary', family='canary', task='seg', B=1, r=1, K=2, L=2, Cx=256, td=1, seed=699, Kc=19, bit_scale=0.01,
              accumulation=True, sampler='ddim', h=5, w=7)

# configurations validate() must refuse (DDP_E_BADCFG with a message): (case to start from, field overrides, word in the message)
REFUSALS = [('bev_kc32_r1', dict(Kc=33), 'classes'), ('seg_L12', dict(L=13), 'num_layers'), ('seg_K64_L12', dict(K=65), 'timesteps'),
            ('depth_L12_r2', dict(L=13), 'num_layers'), ('depth_K64', dict(K=65), 'timesteps')]


def names(family=None):
    return [n for n, c in CASES.items() if family is None or c['family'] == family]


def bev_scopes(c):
    h, w = c['h'], c['w']
    gh, gw = c['grid']
    return dict(input_scope=[[-51.2, 51.2, 102.4 / h], [-51.2, 51.2, 102.4 / w]],
                output_scope=[[-50, 50, 100.0 / max(h + gh, 1)], [-50, 50, 100.0 / max(w + gw, 1)]])


def head_grid(c):
    if c['task'] != 'bev':
        return c['h'], c['w']
    return tuple(int(torch.arange(lo + st / 2, hi, st).numel()) for lo, hi, st in bev_scopes(c)['output_scope'])


def state_dict(c):
    return synthetic.make_state_dict(c['task'], c['Kc'], c['L'], c['Cx'], seed=c['seed'], n_bins=c.get('n_bins') or None)


def inputs(c):
    """-> x (B,Cx,h,w), noise (B,r,Cm,h,w), step_noise (K,B,r,Cm,h,w) or None"""
    cm = 1 if c['task'] == 'depth' else 256
    x, noise = synthetic.make_inputs(c['B'], c['h'], c['w'], c['r'], c['Cx'], cm, seed=c['seed'] + 1)
    sn = None
    if c.get('sampler') == 'ddpm':
        g = torch.Generator().manual_seed(c['seed'] + 2)
        sn = torch.randn((c['K'], c['B'], c['r'], cm, c['h'], c['w']), generator=g)
    return x, noise, sn


def depth_bins(c):
    return torch.linspace(c['min_depth'], c['max_depth'], c['n_bins']) if c.get('n_bins') else None


def engine_kwargs(c):
    """keyword arguments of ddp_amd.engine.DDPEngine (after state_dict, task)"""
    kw = dict(h=c['h'], w=c['w'], batch=c['B'], randsteps=c['r'], timesteps=c['K'], bit_scale=c['bit_scale'], time_difference=c['td'],
              feat_channels=c['Cx'])
    if c['task'] == 'seg':
        kw.update(num_classes=c['Kc'], accumulation=c['accumulation'], sampler=c['sampler'])
    elif c['task'] == 'depth':
        kw.update(min_depth=c['min_depth'], max_depth=c['max_depth'], depth_scale_up=c['scale_up'], depth_use_eps=c['use_eps'])
        if c['n_bins']:
            kw.update(depth_bins=depth_bins(c), depth_norm=c['norm'])
    else:
        s = bev_scopes(c)
        kw.update(num_classes=c['Kc'], threshold=c['threshold'], bev_input_scope=s['input_scope'], bev_output_scope=s['output_scope'])
    return kw


def make_cfg(c, gemm='bf16x3', fused_layer=True, fused_prologue=True, fused_tail=True, nchw_head=True):
    """The ``ddp_cfg`` DDPEngine builds for the case, made without a device (the GPU tests assert it is the same struct)."""
    cfg = _lib.DdpCfg()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.task = {'seg': _lib.TASK_SEG, 'depth': _lib.TASK_DEPTH, 'bev': _lib.TASK_BEV}[c['task']]
    cfg.sampler = _lib.SAMPLER_DDPM if c.get('sampler') == 'ddpm' else _lib.SAMPLER_DDIM
    cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = c['B'], c['r'], c['K'], c['L']
    cfg.num_classes, cfg.feat_channels, cfg.h, cfg.w = c['Kc'], c['Cx'], c['h'], c['w']
    cfg.head_h, cfg.head_w = head_grid(c)
    cfg.accumulation = int(bool(c.get('accumulation', False)))
    cfg.bit_scale = c['bit_scale']
    cfg.min_depth, cfg.max_depth, cfg.threshold = c.get('min_depth', 1e-3), c.get('max_depth', 80.0), c.get('threshold', 0.5)
    if c['task'] == 'bev':
        s = bev_scopes(c)
        for a, ((imin, imax, _), (omin, _, ostep)) in enumerate(zip(s['input_scope'], s['output_scope'])):
            cfg.bev_in_min[a], cfg.bev_in_max[a] = imin, imax
            cfg.bev_out_first[a], cfg.bev_out_step[a] = omin + ostep / 2, ostep
    cfg.gemm_mode = _lib.GEMM_BF16X3 if gemm == 'bf16x3' else _lib.GEMM_F32_MFMA
    cfg.flags = ((0 if fused_layer else _lib.FLAG_UNFUSED_LAYER) | (0 if fused_prologue else _lib.FLAG_UNFUSED_PROLOGUE) |
                 (0 if fused_tail else _lib.FLAG_UNFUSED_TAIL) | (0 if nchw_head else _lib.FLAG_SB_HEAD))
    if c['task'] == 'depth':
        if c['n_bins']:
            cfg.depth_n_bins = c['n_bins']
            cfg.depth_norm = {'linear': _lib.DEPTH_NORM_LINEAR, 'softmax': _lib.DEPTH_NORM_SOFTMAX, 'sigmoid': _lib.DEPTH_NORM_SIGMOID}[c['norm']]
        else:
            cfg.flags |= (_lib.FLAG_DEPTH_SCALE_UP if c['scale_up'] else 0) | (0 if c['use_eps'] else _lib.FLAG_DEPTH_NO_EPS)
        cfg.head_min_depth, cfg.head_max_depth = c['min_depth'], c['max_depth']
    return cfg


def cfg_bytes(cfg):
    return bytes(memoryview(cfg))


def query(lib, cfg):
    """-> (rc, workspace bytes, model-region bytes)"""
    n, m = C.c_size_t(0), C.c_size_t(0)
    rc = lib.ddp_query_workspace(C.byref(cfg), C.byref(n))
    if rc == 0:
        rc = lib.ddp_query_const_workspace(C.byref(cfg), C.byref(m))
    return rc, n.value, m.value


def _depth_binned(x, noise, sd, c):
    """the binned-head sampler of tests/depth_bins_util.py (decode_head.py:233-250) on the case, in the dtype of ``x``"""
    import depth_bins_util as U
    cfg = dict(randsteps=c['r'], bit_scale=c['bit_scale'], min_depth=c['min_depth'], max_depth=c['max_depth'], timesteps=c['K'],
               time_difference=c['td'], head=dict(classify=True, n_bins=c['n_bins'], bins_strategy='UD', norm_strategy=c['norm']))
    return U.sample(x, noise, sd, cfg)


def oracle_image(c, sd, x, noise, step_noise, b, dtype=torch.float32):
    """The reference's sampler (one image per call) on image ``b`` of the case's batch, evaluated in ``dtype``."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    xb, nb = x[b:b + 1].to(dtype), noise[b].to(dtype)
    with torch.no_grad():
        if c['task'] == 'seg' and c['sampler'] == 'ddpm':
            return O.ddpm_sample_seg(xb, nb, step_noise[:, b].to(dtype), sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'],
                                     time_difference=c['td'], accumulation=c['accumulation'])
        if c['task'] == 'seg':
            return O.ddim_sample_seg(xb, nb, sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'],
                                     accumulation=c['accumulation'])
        if c['task'] == 'depth' and c['n_bins']:
            return _depth_binned(xb, nb, sd, c)
        if c['task'] == 'depth':
            return O.sample_depth(xb, nb, sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'],
                                  min_depth=c['min_depth'], max_depth=c['max_depth'], scale_up=c['scale_up'], use_eps=c['use_eps'])
        return O.ddim_sample_bev(xb, nb, sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'],
                                 threshold=c['threshold'], num_classes=c['Kc'], **bev_scopes(c))


_ORACLE = {}


def oracle_batch(c, dtype=torch.float32):
    """(B, ...) expectation of the case, image by image; computed once per (case, dtype) and process"""
    key = (c['name'], dtype)
    if key not in _ORACLE:
        sd = state_dict(c)
        x, noise, sn = inputs(c)
        _ORACLE[key] = torch.cat([oracle_image(c, sd, x, noise, sn, b, dtype) for b in range(c['B'])], dim=0)
    return _ORACLE[key]


def decisions(c, out):
    """the discrete decision a classification output stands for: argmax (seg), > threshold (bev); None for depth"""
    if c['task'] == 'seg':
        return out.argmax(1)
    if c['task'] == 'bev':
        return out > c['threshold']
    return None


def steps_of(c):
    recs = schedule.step_records(c['task'], c['K'], c['td'], 0.0, 'cosine', c.get('sampler', 'ddim'))
    steps = (_lib.DdpStep * c['K'])()
    for i, r in enumerate(recs):
        for k, v in r.items():
            setattr(steps[i], k, v)
    return steps


# every caller-visible buffer of the workspace tail in one engine, at the smallest shape where every rounding matters
# (tests/test_workspace_regions_gpu.py; a target of tests/workspace_history_cases.py)
REGION_SHAPE = dict(B=2, r=2, h=3, w=5, K=2, L=1)
REGION_CASES = {'seg': dict(CASES['seg_L12'], name='regions_seg', Kc=19, **REGION_SHAPE),
                'depth': dict(CASES['depth_K1'], name='regions_depth', **REGION_SHAPE)}


# ---- what the GPU files of the sweep share (tests/test_config_space_gpu.py and the files that borrow its routes) ---------------
def variants(c):
    """(id, gemm, flags) of the case: both engines, and every diagnostic flag that selects another route for the configuration
    (flags act on the bf16x3 engine only; include/ddp_mi355x.h:66-92)"""
    v = [('bf16x3', 'bf16x3', {}), ('f32', 'f32', {}), ('unfused-layer', 'bf16x3', dict(fused_layer=False))]
    seg_ddim = c['task'] == 'seg' and c['sampler'] == 'ddim'
    if c['task'] == 'seg' and c['sampler'] == 'ddpm':           # (no tail kernels on the DDPM path: the step prologue is the only other switch)
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if seg_ddim or (c['task'] == 'depth' and not c['n_bins']) or (c['task'] == 'bev' and c['Kc'] <= 8):
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if c['task'] == 'depth' and c['n_bins']:
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if seg_ddim and c['Cx'] == 256 and c['r'] == 1:
        v.append(('sb-head', 'bf16x3', dict(nchw_head=False)))
    return v


def check_against_oracle(c, out, label):
    ref = oracle_batch(c)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f'{label}: non-finite output'
    errs = [max_rel(out[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    d, dr = decisions(c, out), decisions(c, ref)
    agree = 1.0 if d is None else float((d == dr).float().mean())
    print(f'CONFIG-SPACE {c["family"]} {label}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e}), '
          f'decisions equal {agree:.4f}')
    assert max(errs) < REL and agree > 0.999
    return max(errs)


def expected_launches(path, K, L):
    """Launch counts per tag a path implies, from the launch sites (csrc/ddp_api.hip sample_* / encoder_forward, the prof_begin
    calls of csrc/ddp_gemm_bf16.hip and csrc/ddp_layer_tail.hip).  Tags: 1 x-projection GEMM (256 outputs, TAG_XPROJ), 2 step
    prologue / first head from NCHW (k_layer MODE 2 / 7) and the concat-conv GEMM to SB, 3 layer-0 projection kernel (k_layer
    MODE 3), 7 a plain layer kernel, 8 head GEMMs / seg tails - and EVERY launch_b3_linear of <= 160 outputs or of 256 outputs
    with a tag other than 1 / 3 (launch_b3_linear's dispatch), 10 last layer + tail (k_layer MODE 6 / 8 / 9)."""
    return {
        # xproj hoist; u_0 = W_m . noise is a 256-output GEMM tagged TAG_FEAT, which launch_b3_linear records under 8; layer 0's
        # projections (MODE 3) every step: the BEV head follows a grid resampling
        'bev_chain': {1: 1, 2: 0, 3: K, 7: K * (L - 1), 8: 1, 10: K},
        # the concat-conv GEMM of every step carries TAG_XPROJ; conv_seg is a head GEMM
        'bev_separate': {1: 1 + K, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
        'seg_head7': {1: 0, 2: 1, 3: 0, 7: K * (L - 1), 8: 0, 10: K},
        'seg_prologue': {1: 1, 2: 1, 3: 0, 7: K * (L - 1), 8: 0, 10: K},
        # once per sample: xproj, rvpad (MODE 3 on xproj), rs0 (96 outputs: recorded under 8); layer 0 is MODE 10 under tag 7
        'depth_chain': {1: 1, 2: 0, 3: 1, 7: K * (L - 1), 8: 1, 10: K},
        'depth_lt': {1: 1, 2: 0, 3: K, 7: K * (L - 1), 8: 0, 10: K},
        'depth_bins': {1: 1, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
        # DDP_FLAG_UNFUSED_TAIL
        'seg_unfused_tail_head7': {1: 0, 2: 1, 3: 0, 7: K * L, 8: K, 10: 0},
        'seg_unfused_tail_prologue': {1: 1, 2: 1, 3: 0, 7: K * L, 8: K, 10: 0},
        'depth_unfused_tail': {1: 1, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
    }[path]
