"""What the test files share, each thing once: the suite's bar, the guarded NaN-patterned workspace with its readback, the guarded
engine builder and the per-file state cache, the launch-record reader, the host-side refusal check and measures, the plugin
scaffold, and the helpers more than one file needs.  A plain module, imported like golden_util; the fixtures ``dev`` and ``lib`` reach
a test file by ``from support import dev  # noqa: F401``.

Not here, on purpose: ``golden_util.max_rel`` (float32, clamped denominator - another measure than ``max_rel64``), the byte-sized
guards of the LSS / depth-LSS / evaluation / confusion files (other buffers, other sentinels), their ``_refused`` (other libraries
and entry points) and the ``_rel_live`` masks of the two prior files."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GUARD = 1024                 # floats: 4 KiB in front of and behind the workspace
PATTERN = 0x7FC0BEEF         # a quiet NaN with a payload nobody computes
REL = 2e-4                   # asserted; north_star gate is 1e-3


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from ddp_amd import _lib
    return _lib.load()


# ---- the guarded workspace ------------------------------------------------------------------------------------------------------
def _alloc(n, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


def guarded_buffer(n, dev):
    """``n`` floats between two guards of GUARD floats, every word of the allocation set to PATTERN -> (whole buffer, interior)"""
    buf = _alloc(n + 2 * GUARD, dev)
    buf.view(torch.int32).fill_(PATTERN)
    ws = buf[GUARD:GUARD + n]
    assert ws.data_ptr() % 256 == 0
    return buf, ws


class Guarded:
    """``nbytes`` of workspace for a workspace-taking entry of the C ABI, guarded and patterned as above"""

    def __init__(self, nbytes, dev):
        assert nbytes % 4 == 0
        self.guarded, self.ws = guarded_buffer(nbytes // 4, dev)

    def ptr(self):
        return self.ws.data_ptr()


def guard(eng, exact=False, floats=None):
    """move the engine onto a guarded workspace filled with the NaN pattern, interior included.  ``exact``: the engine's own
    allocation is exactly the queried size (FcnSamplerEngine allocates 64 floats more: ``floats`` names the size instead)"""
    n = eng.workspace.numel() if floats is None else floats
    if exact:
        assert n * 4 == eng._workspace_bytes()
    eng.guarded, eng.workspace = guarded_buffer(n, eng.device)
    return eng


def _overwritten(g):
    """words of the front and of the back guard that no longer hold PATTERN; ``g``: an engine or a Guarded"""
    bits = g.guarded.view(torch.int32)
    return int((bits[:GUARD] != PATTERN).sum()), int((bits[-GUARD:] != PATTERN).sum())


def guards_ok(eng):
    return _overwritten(eng) == (0, 0)


def assert_guards(eng, what):
    bad_f, bad_b = _overwritten(eng)
    assert bad_f == 0 and bad_b == 0, f'{what}: {bad_f} words written in front of the workspace, {bad_b} behind it'


# ---- engines and their state ----------------------------------------------------------------------------------------------------
def state_cache(state_dict, inputs):
    """a cache of its caller's own: ``state(c, dev=None)`` -> (state dict, inputs) of the case, made once per case name; with
    ``dev`` the inputs are kept on the device; ``state.forget(name)`` drops a case again"""
    sds, ins = {}, {}

    def state(c, dev=None):
        if c['name'] not in sds:
            sds[c['name']] = state_dict(c)
            t = inputs(c)
            ins[c['name']] = t if dev is None else tuple(None if v is None else v.to(dev) for v in t)
        return sds[c['name']], ins[c['name']]
    state.forget = lambda name: (sds.pop(name), ins.pop(name))
    return state


def engine(sd, task, kwargs, dev, gemm='bf16x3', batch=None, exact=False, **flags):
    """DDPEngine of a case (``kwargs``: its engine keywords) on a guarded, NaN-patterned workspace.  A caller region (hints, prior,
    class or score prior) holds the PATTERN afterwards: the caller sets or clears it, as the library's contract says."""
    from ddp_amd.engine import DDPEngine
    kw = dict(kwargs)
    if batch is not None:
        kw['batch'] = batch
    return guard(DDPEngine(sd, task, device=dev, gemm=gemm, **flags, **kw), exact)


def fixture_engine(cfg, sd, dev, batch=1, **over):
    """DDPEngine of a reference-made fixture (golden_util.load_case), on its own workspace"""
    from ddp_amd.engine import DDPEngine
    task = cfg['task']
    kw = dict(h=cfg['h'], w=cfg['w'], batch=batch, randsteps=cfg['randsteps'], timesteps=cfg['timesteps'],
              bit_scale=cfg['bit_scale'], time_difference=cfg.get('time_difference', 1), device=dev)
    if task == 'seg':
        kw.update(num_classes=cfg['num_classes'], accumulation=cfg['accumulation'],
                  noise_schedule=cfg['noise_schedule'], sampler=cfg['diffusion'],
                  sample_range0=cfg.get('sample_range', (0.0, 0.999))[0])
    elif task == 'depth':
        kw.update(min_depth=cfg['min_depth'], max_depth=cfg['max_depth'], depth_scale_up=cfg.get('scale_up', False),
                  depth_use_eps=cfg.get('use_eps', True))
    else:
        kw.update(num_classes=6, feat_channels=cfg['feat_channels'], bev_input_scope=cfg['input_scope'],
                  bev_output_scope=cfg['output_scope'])
    kw.update(over)
    return DDPEngine(sd, task, **kw)


# every engine / fusion level of the library runs the reference-made fixtures: the default path (bf16x3 split products,
# persistent layer kernel, fused step head and seg tail), the same arithmetic as separate tile GEMMs, and the exact
# f32-input MFMA engine (include/ddp_mi355x.h DDP_GEMM_*, DDP_FLAG_*)
VARIANTS = {'bf16x3': dict(gemm='bf16x3'), 'f32': dict(gemm='f32'),
            'bf16x3-unfused-layer': dict(gemm='bf16x3', fused_layer=False),
            'bf16x3-unfused-prologue': dict(gemm='bf16x3', fused_prologue=False),
            # the last layer of a step and the seg tail as the two kernels they were fused from (DDP_FLAG_UNFUSED_TAIL)
            'bf16x3-unfused-tail': dict(gemm='bf16x3', fused_tail=False),
            # the first step's head as NCHW -> SB conversions + x-projection GEMM + k_layer MODE 2 (DDP_FLAG_SB_HEAD)
            'bf16x3-sb-head': dict(gemm='bf16x3', nchw_head=False),
            # the LDS gather's "actual mean offset is far from the guess: refill the window" branch (DDP_FLAG_GATHER_GUESS_ZERO)
            'bf16x3-gather-refill': dict(gemm='bf16x3', gather_guess_zero=True)}


def launch_counts(eng, *args, **kw):
    """launches per profiler tag of ONE sample() call (an engine that has not prepared does so before the session is armed).  One
    process-wide session: not run concurrently."""
    from ddp_amd import _lib
    lib = eng.lib
    if not eng._prepared:
        eng.prepare()
    torch.cuda.synchronize()
    ms, n = C.c_float(0), C.c_int(0)
    _lib.check(lib.ddp_profile_begin(255), lib)
    try:
        eng.sample(*args, **kw)
        torch.cuda.synchronize()
    finally:
        rc = lib.ddp_profile_end(C.byref(ms), C.byref(n))
    _lib.check(rc, lib)
    counts = {}
    for tag in range(11):
        _lib.check(lib.ddp_profile_read(tag, C.byref(ms), C.byref(n)), lib)
        counts[tag] = n.value
    return counts


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def finite(t, what):
    assert torch.isfinite(t).all(), f'{what}: non-finite output (a NaN is a read of workspace bytes nobody wrote)'


class FcnLoop:
    """ddp_prepare_fcn / ddp_sample_fcn through the C ABI on a guarded workspace of exactly ``nbytes``.  ``sd``: the segmentor's
    state dict (transform, time_mlp, embedding, conv_seg); ``convs``: the conv array and whatever keeps its tensors alive;
    ``label``: the prefix of the guard messages"""

    def __init__(self, c, sd, dev, batch, convs, cfg, steps, nbytes, label):
        from ddp_amd import _lib
        from ddp_amd.engine import PackedWeights
        self.c, self.dev, self.lib, self.B, self.label = c, dev, _lib.load(), batch, label
        self.weights = PackedWeights(sd, 'seg', 0, dev)
        self.convs, self.keep = convs
        self.cfg, self.steps, self.nbytes = cfg, steps, nbytes
        self.g = Guarded(nbytes, dev)

    def _args(self):
        return (C.byref(self.cfg), C.byref(self.weights.struct), self.convs, self.c['num_convs'], self.c['dilation'], self.steps)

    def prepare(self):
        from ddp_amd import _lib
        self.cfg.flags &= ~_lib.FLAG_FCN_PREPARED
        _lib.check(self.lib.ddp_prepare_fcn(*self._args(), self.g.ptr(), stream(self.dev)), self.lib)
        torch.cuda.synchronize()
        assert_guards(self.g, f'{self.label} {self.c["name"]} ddp_prepare_fcn')
        self.cfg.flags |= _lib.FLAG_FCN_PREPARED

    def sample(self, x, noise, sn, what=''):
        from ddp_amd import _lib
        c = self.c
        out = torch.full((self.B, c['classes'], c['h'], c['w']), float('nan'), device=self.dev)
        _lib.check(self.lib.ddp_sample_fcn(*self._args(), x.data_ptr(), noise.data_ptr(), sn.data_ptr() if sn is not None else None,
                                           out.data_ptr(), self.g.ptr(), stream(self.dev)), self.lib)
        torch.cuda.synchronize()
        assert_guards(self.g, f'{self.label} {c["name"]} {what}')
        finite(out, f'{self.label} {c["name"]} {what}')
        return out

    def record(self):
        """(K, B, r, h, w) uint8: the step record at the end of the workspace (include/ddp_mi355x.h, DDP_FLAG_STEP_RECORD)"""
        from ddp_amd.engine import caller_regions, step_record_view
        return step_record_view(self.g.ws, caller_regions(self.cfg, self.nbytes)['step_rec'][0], self.cfg).clone().cpu()


# ---- host-side checks and measures ----------------------------------------------------------------------------------------------
def refused(lib, cfg, *words):
    """both workspace queries refuse the cfg with DDP_E_BADCFG and a message that carries every word"""
    n = C.c_size_t(0)
    for entry in (lib.ddp_query_workspace, lib.ddp_query_const_workspace):
        assert entry(C.byref(cfg), C.byref(n)) == -1               # DDP_E_BADCFG
        msg = lib.ddp_last_error()
        for w in words:
            assert w.encode() in msg, msg


def round256(n):
    return (n + 255) // 256 * 256


def max_rel64(a, b):
    """the parity measure of tests/test_hip_parity.py evaluated in float64: largest absolute difference over the largest magnitude
    of the expectation (golden_util.max_rel is the float32 form with a clamped denominator: each call site keeps its own)"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def dynamic_symbols(path):
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.split()[1:2] and l.split()[1] in 'TDBRW')


def ref_disagreement(task, rec, out, threshold=0.5):
    """the three definitions of include/ddp_mi355x.h in NumPy: rec (K,B,r,H,W), out (B,C,H,W) -> (B,H,W); depth in fp64"""
    rec, out = rec.numpy(), out.numpy()
    K, B, r, H, W = rec.shape
    flat = rec.transpose(1, 0, 2, 3, 4).reshape(B, K * r, H, W)
    if task == 'seg':
        final = out.argmax(1)                                             # first maximum wins
        return ((flat != final[:, None]).sum(1).astype(np.float32) / np.float32(K * r)).astype(np.float32)
    if task == 'bev':
        Kc = out.shape[1]
        fin = out > np.float32(threshold)                                 # (B,Kc,H,W)
        bits = ((flat.astype(np.int64)[:, :, None] >> np.arange(Kc)[None, None, :, None, None]) & 1).astype(bool)
        return ((bits != fin[:, None]).sum((1, 2)).astype(np.float32) / np.float32(K * r * Kc)).astype(np.float32)
    return flat.astype(np.float64).std(axis=1)                            # population form


def dilate(mask, r):
    """binary dilation of an (h,w) bool map by a (2r+1)^2 square, separable"""
    if r <= 0 or not bool(mask.any()):
        return mask.clone()
    m = mask[None, None].float()
    m = F.max_pool2d(m, (1, 2 * r + 1), stride=1, padding=(0, r))
    m = F.max_pool2d(m, (2 * r + 1, 1), stride=1, padding=(r, 0))
    return m[0, 0] > 0


def dependency_cone(differ, reach, accumulation):
    """Pixels of the FINAL output that a set of differing x0 decisions can influence (segmentors/ddp.py:215-246).
    ``differ[s]`` (h,w) bool: the two runs fed different classes back at step s.  The update (:238-239) and the concat-conv
    are pointwise, so the noisy map entering step s differs exactly where some earlier decision differed; one pass of the
    decoder then carries a changed input at most ``reach`` pixels (layers x (largest sampling offset + the bilinear tap)).
    Output = last step's scores, or with accumulation the mean over all steps."""
    K = len(differ)
    changed = torch.zeros_like(differ[0])
    cone = torch.zeros_like(differ[0])
    for s in range(K):
        if accumulation or s == K - 1:
            cone |= dilate(changed, reach)
        changed = changed | differ[s]
    return cone


# ---- the plugin scaffold --------------------------------------------------------------------------------------------------------
ENCODER = dict(type='DetrTransformerEncoder', num_layers=6,
               transformerlayers=dict(type='BaseTransformerLayer', use_time_mlp=True,
                                      attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=256,
                                                     num_levels=1, num_heads=8, dropout=0.),
                                      ffn_cfgs=dict(type='FFN', embed_dims=256, feedforward_channels=1024,
                                                    ffn_drop=0., act_cfg=dict(type='GELU')),
                                      operation_order=('self_attn', 'norm', 'ffn', 'norm')))
POSENC = dict(type='SinePositionalEncoding', num_feats=128, normalize=True, offset=-0.5)


def seg_cfg(**over):
    # model dict of segmentation/configs/ade/ddp_swin_t_2x8_512x512_160k_ade20k.py:11-108 (hot-path part)
    cfg = dict(type='DDP', timesteps=3, bit_scale=0.01, accumulation=True,
               decode_head=dict(type='DeformableHeadWithTime', in_channels=[256], channels=256, in_index=[0],
                                dropout_ratio=0., num_classes=150, norm_cfg=dict(type='SyncBN'), align_corners=False,
                                num_feature_levels=1, encoder=ENCODER, positional_encoding=POSENC,
                                loss_decode=dict(type='CrossEntropyLoss')),
               train_cfg=dict(), test_cfg=dict(mode='whole'))
    cfg.update(over)
    return cfg


def seg_model(cfg):
    """the segmentor of a reference-made fixture's cfg (golden_util.load_case), not yet loaded"""
    import ddp_amd
    return ddp_amd.build_segmentor(seg_cfg(
        timesteps=cfg['timesteps'], randsteps=cfg['randsteps'], bit_scale=cfg['bit_scale'],
        accumulation=cfg['accumulation'], noise_schedule=cfg['noise_schedule'], diffusion=cfg['diffusion'],
        sample_range=tuple(cfg.get('sample_range', (0, 0.999))),
        decode_head=dict(seg_cfg()['decode_head'], num_classes=cfg['num_classes'])))


def depth_model(cfg, sd, align_corners=False, min_depth=1e-3, max_depth=80):
    import ddp_amd
    dcfg = dict(type='DDP', bit_scale=cfg.get('bit_scale', 0.1), timesteps=cfg.get('timesteps', 3), randsteps=cfg.get('randsteps', 1),
                min_depth=min_depth, max_depth=max_depth, test_cfg=dict(mode='whole'),
                decode_head=dict(type='DeformableHeadWithTime', in_channels=[256], channels=256, in_index=[0],
                                 dropout_ratio=0., scale_up=False, min_depth=min_depth, max_depth=max_depth, use_eps=True,
                                 align_corners=align_corners, num_feature_levels=1, encoder=ENCODER, positional_encoding=POSENC))
    model = ddp_amd.build_depther(dcfg)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


class FixedBackbone(torch.nn.Module):
    """stands in for Swin+FPN+MultiStageMerging (frozen, upstream of the hot path): returns [x]."""

    def __init__(self, x):
        super().__init__()
        self.x = x

    def forward(self, img):
        return [self.x]


class PoolBackbone(torch.nn.Module):
    """a stand-in backbone whose feature map depends on the image it is given (slide windows, flipped augmentations): the image
    pooled to (h, w) and spread over 256 channels by a fixed seeded projection"""

    def __init__(self, h, w):
        super().__init__()
        self.hw = (h, w)
        self.register_buffer('proj', torch.randn(256, 3, generator=torch.Generator().manual_seed(17)))

    def forward(self, img):
        p = F.adaptive_avg_pool2d(img, self.hw)
        return [torch.einsum('oc,bchw->bohw', self.proj, p).contiguous()]


def seg_plugin(c, dev, sd, pool_backbone=False, **cfg):
    """the seg ``DDP`` segmentor of a config_space-style case, loaded with ``sd``; ``cfg``: further model settings (noise_seed=5 for
    the prior files); ``pool_backbone``: with a PoolBackbone at the case's map size"""
    import ddp_amd
    head = dict(seg_cfg()['decode_head'], num_classes=c['Kc'], encoder=dict(ENCODER, num_layers=c['L']))
    model = ddp_amd.build_segmentor(seg_cfg(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], accumulation=c['accumulation'],
                                            diffusion=c['sampler'], sample_range=(0, 0.999), time_difference=c['td'], decode_head=head,
                                            **cfg))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    if pool_backbone:
        model.backbone = PoolBackbone(c['h'], c['w']).to(dev)
    return model


def depth_plugin(c, dev, sd):
    """the depth ``DDP`` of a config_space-style case (regression or binned head), loaded with ``sd``"""
    import ddp_amd
    head = dict(type='DeformableHeadWithTime', in_channels=[256], channels=256, in_index=[0], dropout_ratio=0., scale_up=False,
                min_depth=c['min_depth'], max_depth=c['max_depth'], use_eps=True, align_corners=False, num_feature_levels=1,
                encoder=dict(ENCODER, num_layers=c['L']), positional_encoding=POSENC)
    if c['n_bins']:
        head.update(classify=True, n_bins=c['n_bins'], bins_strategy='UD', norm_strategy=c['norm'])
    model = ddp_amd.build_depther(dict(type='DDP', bit_scale=c['bit_scale'], timesteps=c['K'], randsteps=c['r'], time_difference=c['td'],
                                       min_depth=c['min_depth'], max_depth=c['max_depth'], test_cfg=dict(mode='whole'), decode_head=head))
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval()


def bev_plugin(sd, dev, num_layers, grid_transform, **model_kw):
    """BEVDDP and its six-class head (the plugin class has the reference's six classes), loaded from one state dict -> (model, head)"""
    import ddp_amd
    head = ddp_amd.BEVDeformableHeadWithTime(num_feature_levels=1, encoder=dict(ENCODER, num_layers=num_layers), positional_encoding=POSENC,
                                             classes=list('abcdef'), loss='focal', grid_transform=grid_transform)
    model = ddp_amd.BEVDDP(**model_kw)
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith('decode_head.')}, strict=True)
    head.load_state_dict({k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, strict=True)
    return model.to(dev).eval(), head.to(dev).eval()
