"""DDP_FLAG_X0_HINTS: the cases shared by tests/test_x0_hints_host.py (CPU) and tests/test_x0_hints_gpu.py (GPU), their hint maps
and the hinted EXPECTATION - a small loop composed from oracle.ddp_oracle's own functions (the schedules, time_mlp, the head
forwards, x0_from_logits_seg(idx=...)), one image per call like the reference's samplers.

Semantics under test (include/ddp_mi355x.h, "x0 hints"): where the caller knows the answer, it is fed back as x0 at every step in
place of the model's own prediction; the scores / depth returned stay the model's own.
  seg    hint (h, w) uint8: < num_classes -> that class replaces the argmax (segmentors/ddp.py:235); >= num_classes -> free
  depth  hint (h, w) float32: finite and > 0 -> replaces depth_pred in the x0 normalisation only (depther/ddp.py:240-241, clamped like
         a prediction by :224); 0, negative, NaN, +-inf -> free

A case is a dict of tests/config_space_cases.py (same builders: state_dict, inputs, engine_kwargs, make_cfg, ...).  Shapes: B = 2 or
3, token counts that are no multiple of 32, L = 2, K = 3 or 4; seg class counts 1, 19, 150 and 255.

``witness``: whether the hinted expectation must differ from the unhinted one by more than 10 * REL.  It is False for exactly one
case, the one-class model: its only legal hint is class 0, which is also every argmax - hints cannot change anything there, and the
case is about the class-count limit, not about an effect."""
import torch
import torch.nn.functional as F

import config_space_cases as CS
from oracle import ddp_oracle as O
from support import max_rel64 as max_rel, round256  # noqa: F401  (the float64 measure: H.max_rel at every call site)

REL = CS.REL
COND = CS.COND
WITNESS = 10 * REL

CASES = {}


def _add(name, task, **kw):
    c = dict(name=name, family='x0_hints', task=task, B=2, r=1, K=3, L=2, Cx=256, td=1, seed=len(CASES) + 900, witness=True)
    if task == 'seg':
        c.update(Kc=19, bit_scale=0.01, accumulation=True, sampler='ddim')
    else:
        c.update(Kc=1, K=4, bit_scale=0.1, min_depth=1e-3, max_depth=80.0, scale_up=False, use_eps=True, n_bins=0, norm='linear')
    c.update(kw)
    assert name not in CASES
    CASES[name] = c


# ---- seg: ddim on the head7 route (r = 1, Cx = 256) and the prologue route (r = 2), ddpm; 1 / 19 / 150 / 255 classes ----------------
_add('seg_kc19_7x13', 'seg', h=7, w=13, path='seg_head7')
_add('seg_kc150_9x14_noacc', 'seg', h=9, w=14, Kc=150, accumulation=False, K=4, path='seg_head7')
_add('seg_kc255_5x10_r2', 'seg', h=5, w=10, Kc=255, r=2, path='seg_prologue')
_add('seg_kc1_1x37', 'seg', h=1, w=37, Kc=1, B=3, witness=False, path='seg_head7')
_add('seg_kc19_1x1', 'seg', h=1, w=1, B=3, K=4, path='seg_head7')
_add('seg_ddpm_7x13', 'seg', h=7, w=13, sampler='ddpm', K=4)
# ---- depth: the GEMM-free chain, the layer-0 projection head (r = 2), the binned head, one pixel ------------------------------------
_add('depth_9x14', 'depth', h=9, w=14, path='depth_chain')
_add('depth_5x10_r2', 'depth', h=5, w=10, r=2, path='depth_lt')
_add('depth_1x37_bins', 'depth', h=1, w=37, B=3, n_bins=24, norm='softmax', path='depth_bins')
_add('depth_1x1', 'depth', h=1, w=1, B=3, K=3, path='depth_chain')


def names(task=None, sampler=None):
    return [n for n, c in CASES.items() if (task is None or c['task'] == task) and (sampler is None or c.get('sampler') == sampler)]


FREE_SEG = 255


def free_hints(c):
    """(B, h, w): every pixel free"""
    if c['task'] == 'seg':
        return torch.full((c['B'], c['h'], c['w']), FREE_SEG, dtype=torch.uint8)
    return torch.zeros((c['B'], c['h'], c['w']), dtype=torch.float32)


def full_hints(c):
    """(B, h, w): every pixel hinted - seeded classes / depths inside the range"""
    g = torch.Generator().manual_seed(c['seed'] + 5)
    shape = (c['B'], c['h'], c['w'])
    if c['task'] == 'seg':
        return torch.randint(0, c['Kc'], shape, generator=g).to(torch.uint8)
    return torch.rand(shape, generator=g) * (c['max_depth'] - 1.0) + 1.0


def partial_hints(c):
    """(B, h, w) hints of the case.
    seg: a block per image that crosses the image's rows and, in the flat token order, the 32-token groups and the image border (it
    reaches the last pixel of image b and the block of image b + 1 starts at its first), scattered pixels, and "free" written as several
    values of [num_classes, 255].
    depth: about 5 % scattered pixels and one dense block; values below min_depth and above max_depth among the hints; NaN, 0, a
    negative value and +-inf among the free pixels."""
    g = torch.Generator().manual_seed(c['seed'] + 6)
    B, h, w = c['B'], c['h'], c['w']
    N = h * w
    if c['task'] == 'seg':
        K = c['Kc']
        hint = torch.full((B, N), FREE_SEG, dtype=torch.int64)
        # free, in every encoding the class count leaves
        enc = torch.tensor(sorted({K, min(K + 1, 255), (K + 255) // 2, 254, 255} - set(range(K))), dtype=torch.int64)
        hint[:] = enc[torch.randint(0, len(enc), (B, N), generator=g)]
        cls = torch.randint(0, K, (B, N), generator=g)
        blk = max(N // 3, 1)
        for b in range(B):
            hint[b, :blk] = cls[b, :blk]                   # from the image's first token ...
            hint[b, N - blk:] = cls[b, N - blk:]           # ... and up to its last: contiguous with image b + 1's block
            sc = torch.rand(N, generator=g) < 0.15
            hint[b][sc] = cls[b][sc]
        return hint.view(B, h, w).to(torch.uint8)
    lo, hi = c['min_depth'], c['max_depth']
    hint = torch.zeros((B, N), dtype=torch.float32)
    val = torch.rand((B, N), generator=g) * (hi - 1.0) + 1.0
    for b in range(B):
        sc = torch.rand(N, generator=g) < 0.05
        hint[b][sc] = val[b][sc]
        blk = max(N // 4, 1)
        s0 = (N - blk) // 2 if b % 2 else N - blk           # a dense block (the last tokens of even images)
        hint[b, s0:s0 + blk] = val[b, s0:s0 + blk]
    # out-of-range hints (clamped like a prediction) and every free encoding, at fixed places
    special = [lo * 0.5, hi * 1.5, float('nan'), 0.0, -3.0, float('inf'), float('-inf')]
    flat = hint.view(-1)
    for i, v in enumerate(special):
        flat[(i * 7 + 1) % flat.numel()] = v
    if N == 1:                                              # one pixel per image: image 0 hinted inside the range, 1 above it, 2 free (NaN)
        flat[0], flat[1] = 0.25 * hi, hi * 1.5
        if B > 2:
            flat[2] = float('nan')
    return hint.view(B, h, w)


def hinted(c, hint_b):
    """mask (h, w) of the pixels of ONE image's hint map that are hinted"""
    if c['task'] == 'seg':
        return hint_b < c['Kc']
    return torch.isfinite(hint_b) & (hint_b > 0)


def seg_image(c, sd, x, noise, step_noise, hint, dtype=torch.float32, decisions=None, x0_index=None):
    """segmentors/ddp.py:215-246 (ddim) / :248-290 (ddpm) for one image with hints: O.ddim_sample_seg / O.ddpm_sample_seg line by line,
    the x0 class = where(hint < K, hint, argmax).  x (1,Cx,h,w), noise (r,256,h,w), step_noise (K,r,256,h,w) or None, hint (h,w) uint8.
    ``decisions`` receives the model's OWN argmax (r,h,w) of every step; ``x0_index`` (K maps (r,h,w)) replaces the whole decision."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x, noise = x.to(dtype), noise.to(dtype)
    K, r, bit = c['K'], c['r'], c['bit_scale']
    ddpm = c['sampler'] == 'ddpm'
    on = (hint < c['Kc'])[None].expand(r, -1, -1)
    hv = hint.long()[None].expand(r, -1, -1)
    xr = x.repeat(r, 1, 1, 1)
    mask_t = noise.clone()
    outs = []
    logits = None
    with torch.no_grad():
        for s, (t_now, t_next) in enumerate(O.sampling_time_pairs(K, c['td'], 0.0)):
            times_now = torch.tensor([t_now], dtype=torch.float32)
            times_next = torch.tensor([t_next], dtype=torch.float32)
            feat = F.conv2d(torch.cat([xr, mask_t], dim=1), sd['transform.conv.weight'], sd['transform.conv.bias'])
            log_snr = O.alpha_cosine_log_snr(times_now)
            log_snr_next = O.alpha_cosine_log_snr(times_next)
            pl, pln = log_snr.view(-1, 1, 1, 1), log_snr_next.view(-1, 1, 1, 1)
            alpha, sigma = O.log_snr_to_alpha_sigma(pl)
            alpha_next, sigma_next = O.log_snr_to_alpha_sigma(pln)
            temb = O.time_mlp(log_snr, sd)
            logits = O.head_forward_seg(feat, temb, sd)
            own = torch.argmax(logits, dim=1)
            if decisions is not None:
                decisions.append(own.to(torch.uint8))
            idx = torch.where(on, hv, own) if x0_index is None else x0_index[s].long()
            x0 = O.x0_from_logits_seg(logits, sd, bit, idx)
            if ddpm:
                cc = -torch.special.expm1(pl - pln)
                mean = alpha_next * (mask_t * (1 - cc) / alpha + cc * x0)
                variance = (sigma_next ** 2) * cc
                log_variance = O.log_clamped(variance)
                nz = step_noise[s].to(dtype) if t_next > 0 else torch.zeros_like(mask_t)
                mask_t = mean + (0.5 * log_variance).exp() * nz
            else:
                pred_noise = (mask_t - alpha * x0) / sigma.clamp(min=1e-8)
                mask_t = x0 * alpha_next + pred_noise * sigma_next
            if c['accumulation']:
                outs.append(logits.softmax(1))
    if c['accumulation']:
        logits = torch.cat(outs, dim=0)
    return logits.mean(dim=0, keepdim=True)


def _depth_head(c, feat, temb, sd):
    if c['n_bins']:
        import depth_bins_util as U
        head = U.head_of(dict(min_depth=c['min_depth'], max_depth=c['max_depth'],
                              head=dict(classify=True, n_bins=c['n_bins'], bins_strategy='UD', norm_strategy=c['norm'])))
        return U.head_forward(feat, temb, sd, head)
    return O.head_forward_depth(feat, temb, sd, c['min_depth'], 'gridsample', None, c['scale_up'], c['use_eps'], c['max_depth'])


def depth_image(c, sd, x, noise, hint, dtype=torch.float32, preds=None):
    """depther/ddp.py:229-247 for one image with hints: O.sample_depth line by line, the x0 normalisation reads where(hinted, hint,
    depth_pred).  x (1,Cx,h,w), noise (r,1,h,w), hint (h,w) float32.  ``preds`` receives the model's OWN prediction (r,1,h,w) per step."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x, noise = x.to(dtype), noise.to(dtype)
    r, bit, lo, hi = c['r'], c['bit_scale'], c['min_depth'], c['max_depth']
    on = hinted(c, hint)[None, None].expand(r, -1, -1, -1)
    hv = torch.where(hinted(c, hint), hint, torch.zeros_like(hint)).to(dtype)[None, None].expand(r, -1, -1, -1)
    xr = x.repeat(r, 1, 1, 1)
    depth_t = noise.clone()
    depth_pred = None
    with torch.no_grad():
        for t_now, t_next in O.sampling_time_pairs(c['K'], c['td'], 0.0):
            times_now = torch.tensor([t_now], dtype=torch.float32)
            times_next = torch.tensor([t_next], dtype=torch.float32)
            feat = F.conv2d(torch.cat([xr, depth_t], dim=1), sd['down.conv.weight'], sd['down.conv.bias'])
            temb = O.time_mlp(times_now, sd)
            depth_pred = _depth_head(c, feat, temb, sd)
            if preds is not None:
                preds.append(depth_pred.clone())
            x0 = (torch.where(on, hv, depth_pred) - lo) / (hi - lo)
            x0 = (x0 * 2 - 1) * bit
            a_now = O.gamma_cosine(times_now.view(-1, 1, 1, 1))
            a_next = O.gamma_cosine(times_next.view(-1, 1, 1, 1))
            x0 = x0.clamp(-bit, bit)
            eps = (1 / (1 - a_now).sqrt()) * (depth_t - a_now.sqrt() * x0)
            depth_t = a_next.sqrt() * x0 + (1 - a_next).sqrt() * eps
    return depth_pred.mean(dim=0, keepdim=True)


_EXPECT = {}


def expected(c, kind, dtype=torch.float32):
    """(B, ...) hinted expectation of the case for the hint map ``kind`` ('free', 'full', 'partial'), image by image; computed once
    per (case, kind, dtype) and process and never modified.  -> (out, record): record = the model's own per-step prediction,
    (K, B, r, h, w) - seg uint8 argmax, depth the metric prediction."""
    key = (c['name'], kind, dtype)
    if key not in _EXPECT:
        sd = CS.state_dict(c)
        x, noise, sn = CS.inputs(c)
        hints = {'free': free_hints, 'full': full_hints, 'partial': partial_hints}[kind](c)
        outs, recs = [], []
        for b in range(c['B']):
            rec = []
            if c['task'] == 'seg':
                outs.append(seg_image(c, sd, x[b:b + 1], noise[b], None if sn is None else sn[:, b], hints[b], dtype, decisions=rec))
            else:
                outs.append(depth_image(c, sd, x[b:b + 1], noise[b], hints[b], dtype, preds=rec))
                rec = [p[:, 0] for p in rec]
            recs.append(torch.stack(rec, 0))                       # (K, r, h, w)
        _EXPECT[key] = (torch.cat(outs, 0), torch.stack(recs, 1))  # (B, ...), (K, B, r, h, w)
    return _EXPECT[key]


def routes(c):
    """(id, gemm, flags): both engines and every flag that selects another route for the case (tests/test_config_space_gpu.py)"""
    v = [('bf16x3', 'bf16x3', {}), ('f32', 'f32', {}), ('unfused-layer', 'bf16x3', dict(fused_layer=False)),
         ('unfused-prologue', 'bf16x3', dict(fused_prologue=False))]
    if c['task'] == 'seg' and c['sampler'] == 'ddim':
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
        if c['r'] == 1:
            v.append(('sb-head', 'bf16x3', dict(nchw_head=False)))
    if c['task'] == 'seg' and c['sampler'] == 'ddpm':
        v += [('chain', 'bf16x3', dict(ddpm_chain=True)), ('chain-unfused-tail', 'bf16x3', dict(ddpm_chain=True, fused_tail=False)),
              ('chain-sb-head', 'bf16x3', dict(ddpm_chain=True, nchw_head=False))]
    if c['task'] == 'depth' and not c['n_bins']:
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
    return v


def hint_bytes(c):
    """(hint_bytes, row_bytes) of include/ddp_mi355x.h as formulas of the case"""
    e = 1 if c['task'] == 'seg' else 4
    n = c['B'] * c['h'] * c['w'] * e
    return n, n * c['r']
