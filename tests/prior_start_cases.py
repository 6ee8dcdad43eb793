"""DDP_FLAG_PRIOR_START: the cases shared by tests/test_prior_start_host.py (CPU) and tests/test_prior_start_gpu.py (GPU), their prior
maps, the start map and the EXPECTATION - a loop composed from oracle.ddp_oracle's own functions (the schedules, time_mlp, the head
forwards, x0_from_logits_seg) that takes (start_map, t_start), one image per call like the reference's samplers.

Semantics under test (include/ddp_mi355x.h, "prior start"): the chain starts from the caller's prior map noised to t_start instead
of from pure noise at t = 1, and its K steps divide [0, t_start] (ddp_amd.schedule.get_sampling_timesteps(t_start=)).
  seg    prior (h, w) uint8: < num_classes -> that class; any other value -> the ignore row embedding[num_classes] (ddp.py:151)
  depth  prior (h, w) float32 metric depth: finite and > 0 -> the x0 normalisation with its clamp; anything else -> x0 = 0
  bev    prior (h, w) int32 bit words: bit c = class c present, bits >= num_classes ignored
  start  seg / bev  alpha(t_start) x0 + sigma(t_start) eps;  depth  sqrt(gamma) x0 + eps / (1 / sqrt(1 - gamma))

A case is a dict of tests/config_space_cases.py (same builders).  Shapes: B = 2 or 3, L = 2, K in {1, 2, 3}, token counts that are no
multiple of 4 or 32 (7 x 13 = 91, 9 x 14 = 126, 5 x 10 = 50, 37, 1; bev 12 x 20 = 240 is the one multiple of 4: the 16-byte path).

``witness``: whether the prior-start output must differ from the noise-start output at the same t_start by more than 10 * REL.  It
is False for exactly one case, the one-class model: its score map has one channel, every argmax is class 0 whatever the start map.
At t_start = 1 no case can have a witness (alpha(1) = 8e-5: the prior is drowned), so every case's own t_start is 0.6 or 0.25 and
1.0 is run in addition."""
import torch
import torch.nn.functional as F

import config_space_cases as CS
from ddp_amd import schedule
from oracle import ddp_oracle as O
from support import max_rel64 as max_rel, round256  # noqa: F401  (the float64 measure: P.max_rel at every call site)

REL = CS.REL
COND = CS.COND
WITNESS = 10 * REL

CASES = {}


def _add(name, task, **kw):
    c = dict(name=name, family='prior_start', task=task, B=2, r=1, K=3, L=2, Cx=256, td=1, seed=len(CASES) + 1100, witness=True,
             t_start=0.6)
    if task == 'seg':
        c.update(Kc=19, bit_scale=0.01, accumulation=True, sampler='ddim')
    elif task == 'depth':
        c.update(Kc=1, bit_scale=0.1, min_depth=1e-3, max_depth=80.0, scale_up=False, use_eps=True, n_bins=0, norm='linear', map_gain=100.0)
    else:
        c.update(Kc=6, bit_scale=0.01, threshold=0.5, grid=(7, 9), h=12, w=20)
    c.update(kw)
    assert name not in CASES
    CASES[name] = c


_add('seg_kc19_7x13', 'seg', h=7, w=13, t_start=0.6, K=2)
_add('seg_kc150_9x14_noacc', 'seg', h=9, w=14, Kc=150, accumulation=False, t_start=0.25, K=3)
_add('seg_kc255_5x10_r2', 'seg', h=5, w=10, Kc=255, r=2, t_start=0.6, K=2)
_add('seg_kc1_1x37', 'seg', h=1, w=37, Kc=1, B=3, witness=False, t_start=0.6, K=2)
_add('seg_kc19_1x1', 'seg', h=1, w=1, B=3, t_start=0.25, K=1)
_add('seg_ddpm_7x13', 'seg', h=7, w=13, sampler='ddpm', t_start=0.6, K=3)
_add('seg_kc256_3x11', 'seg', h=3, w=11, Kc=256, t_start=0.25, K=2)
_add('depth_9x14', 'depth', h=9, w=14, t_start=0.6, K=3)
_add('depth_5x10_r2', 'depth', h=5, w=10, r=2, t_start=0.25, K=2)
_add('depth_1x37_bins', 'depth', h=1, w=37, B=3, n_bins=24, norm='softmax', t_start=0.25, K=2)
_add('depth_1x1', 'depth', h=1, w=1, B=3, t_start=0.6, K=1)
_add('bev_kc8_r1', 'bev', Kc=8, r=1, t_start=0.6, K=2)
_add('bev_kc9_r2', 'bev', Kc=9, r=2, t_start=0.25, K=3)


T_STARTS = (1.0, 0.6, 0.25)     # every case runs from 1.0 as well (test "t_start = 1"); its own t_start is one of the other two


def state_dict(c):
    """the case's model: tests/config_space_cases.py's, and for depth the concat-conv's column of the noisy map scaled by ``map_gain``.
    The 'init' profile gives that one column of 257 the weight of any other, and the depth a model predicts then moves by 1e-5 of
    its range whatever map it starts from - a loop that ignored the start map altogether would pass at REL.  With the column at
    100 x, the start map moves the output by 1e-2 (tests/test_prior_start_host.py prints the figure per case)."""
    sd = CS.state_dict(c)
    if c['task'] == 'depth':
        sd = dict(sd)
        w = sd['down.conv.weight'].clone()
        w[:, -1] *= c['map_gain']
        sd['down.conv.weight'] = w
    return sd


def names(task=None):
    return [n for n, c in CASES.items() if task is None or c['task'] == task]


PRIOR_DTYPE = {'seg': torch.uint8, 'depth': torch.float32, 'bev': torch.int32}


def cleared_prior(c):
    """(B, h, w): what DDPEngine.clear_prior writes - seg 255, depth 0, bev 0"""
    return torch.full((c['B'], c['h'], c['w']), 255 if c['task'] == 'seg' else 0, dtype=PRIOR_DTYPE[c['task']])


def prior(c, which=0):
    """(B, h, w) seeded prior map of the case (``which`` = 0, 1: two different maps).
    seg: seeded classes, about a fifth of the pixels in the ignore encodings the class count leaves ({K, K + 1, .., 254, 255});
    depth: depths inside the range, with NaN, 0, a negative value, +-inf and values below min_depth / above max_depth at fixed places;
    bev: seeded bit words over ALL 32 bits (bits >= num_classes are set in about half the pixels).
    In flat token order the map changes across the image border: the last pixel of image b and the first of image b + 1 differ."""
    g = torch.Generator().manual_seed(c['seed'] + 21 + 7 * which)
    B, h, w = c['B'], c['h'], c['w']
    N = h * w
    if c['task'] == 'seg':
        K = c['Kc']
        p = torch.randint(0, K, (B, N), generator=g)
        enc = sorted(v for v in {K, min(K + 1, 255), (K + 255) // 2, 254, 255} if K <= v <= 255)      # (256 classes: none)
        if enc:
            e = torch.tensor(enc)[torch.randint(0, len(enc), (B, N), generator=g)]
            ign = torch.rand((B, N), generator=g) < 0.2
            p = torch.where(ign, e, p)
        for b in range(B):                                     # the border: a class at the end of image b, another value at the start of b + 1
            p[b, N - 1] = (b + which) % K
            p[b, 0] = enc[b % len(enc)] if enc else (b + which + 5) % K
            if N == 1:                                         # one pixel per image: a class, the ignore row, another class
                p[b, 0] = enc[-1] if (b == 1 and enc) else (3 * b + which) % K
        return p.view(B, h, w).to(torch.uint8)
    if c['task'] == 'depth':
        lo, hi = c['min_depth'], c['max_depth']
        p = torch.rand((B, N), generator=g) * (hi - 1.0) + 1.0
        special = [lo * 0.5, hi * 1.5, float('nan'), 0.0, -3.0, float('inf'), float('-inf')]
        flat = p.view(-1)
        for i, v in enumerate(special):
            flat[(i * 7 + 1 + which) % flat.numel()] = v
        if N == 1:                                             # one pixel per image: inside the range, above it, NaN
            flat[0], flat[1] = (0.25 + 0.4 * which) * hi, hi * 1.5
            flat[2] = float('nan')
        return p.view(B, h, w)
    K = c['Kc']
    bits = torch.randint(0, 2, (B, N, 32), generator=g)
    bits[:, :, K:] *= torch.randint(0, 2, (B, N, 1), generator=g)
    for b in range(B):
        bits[b, N - 1, :K] = 1
        bits[b, 0, :K] = 0
        bits[b, 0, (b + which) % K] = 1
    word = (bits.long() << torch.arange(32)).sum(-1)           # 0 .. 2^32 - 1
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)   # the same 32 bits as int32
    return word.to(torch.int32).view(B, h, w)


def x0_of_prior(c, sd, prior_b, dtype=torch.float32):
    """the x0 the prior map of ONE image (h, w) stands for -> (1, Cm, h, w), with the oracle's own operators"""
    if c['task'] == 'seg':
        p = prior_b.long()
        idx = torch.where(p < c['Kc'], p, torch.full_like(p, c['Kc']))[None]
        return O.x0_from_logits_seg(None, {k: v.to(dtype) for k, v in sd.items() if k == 'embedding_table.weight'}, c['bit_scale'], idx)
    if c['task'] == 'depth':
        lo, hi, bit = c['min_depth'], c['max_depth'], c['bit_scale']
        ok = torch.isfinite(prior_b) & (prior_b > 0)
        d = torch.where(ok, prior_b, torch.zeros_like(prior_b)).to(dtype)
        x0 = (d - lo) / (hi - lo)
        x0 = ((x0 * 2 - 1) * bit).clamp(-bit, bit)
        return torch.where(ok, x0, torch.zeros_like(x0))[None, None]
    K = c['Kc']
    word = prior_b.long() & 0xFFFFFFFF
    on = (word[None] >> torch.arange(K).view(K, 1, 1)) & 1                      # (K, h, w)
    ids = (on * (torch.arange(K) + 1).view(K, 1, 1))[None]                      # (1, K, h, w): fusion_models/ddp.py pred * factor
    e = F.embedding(ids, sd['embedding_table.weight'].to(dtype)).mean(dim=1).permute(0, 3, 1, 2)
    return (torch.sigmoid(e) * 2 - 1) * c['bit_scale']


def start_scalars(c, t_start):
    """(alpha, sigma) of ``ddp_step`` record 0 as ddp_amd.schedule evaluates them: python floats of fp32 values"""
    r = schedule.step_records(c['task'], c['K'], c['td'], 0.0, 'cosine', c.get('sampler', 'ddim'), t_start=t_start)[0]
    return r['alpha'], r['sigma']


def start_map(c, sd, prior_b, noise_b, t_start, dtype=torch.float32):
    """m0 (r, Cm, h, w) of ONE image: the formulas of include/ddp_mi355x.h with the scalars of ``start_scalars`` and eps = noise_b
    (r, Cm, h, w), evaluated in ``dtype`` (fp64: what the GPU's start map is compared with)"""
    a, s = start_scalars(c, t_start)
    x0 = x0_of_prior(c, sd, prior_b, dtype)
    eps = noise_b.to(dtype)
    if c['task'] == 'depth':
        return a * x0 + eps / s
    return a * x0 + s * eps


def start_terms(c, sd, prior_b, noise_b, t_start):
    """(|alpha x0|, |sigma-term|) in fp64, broadcast to (r, Cm, h, w): the magnitudes the start map's error bar is made of"""
    a, s = start_scalars(c, t_start)
    x0 = x0_of_prior(c, sd, prior_b, torch.float64)
    eps = noise_b.double()
    return (a * x0).abs().expand_as(eps), (eps / s if c['task'] == 'depth' else s * eps).abs()


def time_pairs(c, t_start):
    return schedule.get_sampling_timesteps(c['K'], c['td'], 0.0, t_start=t_start)


def seg_image(c, sd, x, start, step_noise, t_start, dtype=torch.float32, decisions=None, x0_index=None):
    """segmentors/ddp.py:215-246 (ddim) / :248-290 (ddpm) for one image from (start, t_start): O.ddim_sample_seg / O.ddpm_sample_seg
    line by line with mask_t = start and the time pairs of [0, t_start].  x (1,Cx,h,w), start (r,256,h,w), step_noise (K,r,256,h,w) or
    None.  ``decisions`` receives every step's argmax (r,h,w); ``x0_index`` (K maps (r,h,w)) replaces it in the x0 projection."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    r, bit = c['r'], c['bit_scale']
    ddpm = c['sampler'] == 'ddpm'
    xr = x.repeat(r, 1, 1, 1)
    mask_t = start.to(dtype).clone()
    outs = []
    logits = None
    with torch.no_grad():
        for s, (t_now, t_next) in enumerate(time_pairs(c, t_start)):
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
            x0 = O.x0_from_logits_seg(logits, sd, bit, None if x0_index is None else x0_index[s].long())
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


def depth_image(c, sd, x, start, step_noise, t_start, dtype=torch.float32, decisions=None, x0_index=None):
    """depther/ddp.py:229-247 for one image from (start, t_start): O.sample_depth line by line with depth_t = start.
    x (1,Cx,h,w), start (r,1,h,w).  ``decisions`` receives every step's prediction (r,h,w)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    r, bit, lo, hi = c['r'], c['bit_scale'], c['min_depth'], c['max_depth']
    xr = x.repeat(r, 1, 1, 1)
    depth_t = start.to(dtype).clone()
    depth_pred = None
    with torch.no_grad():
        for t_now, t_next in time_pairs(c, t_start):
            times_now = torch.tensor([t_now], dtype=torch.float32)
            times_next = torch.tensor([t_next], dtype=torch.float32)
            feat = F.conv2d(torch.cat([xr, depth_t], dim=1), sd['down.conv.weight'], sd['down.conv.bias'])
            temb = O.time_mlp(times_now, sd)
            depth_pred = _depth_head(c, feat, temb, sd)
            if decisions is not None:
                decisions.append(depth_pred[:, 0].clone())
            x0 = (depth_pred - lo) / (hi - lo)
            x0 = (x0 * 2 - 1) * bit
            a_now = O.gamma_cosine(times_now.view(-1, 1, 1, 1))
            a_next = O.gamma_cosine(times_next.view(-1, 1, 1, 1))
            x0 = x0.clamp(-bit, bit)
            eps = (1 / (1 - a_now).sqrt()) * (depth_t - a_now.sqrt() * x0)
            depth_t = a_next.sqrt() * x0 + (1 - a_next).sqrt() * eps
    return depth_pred.mean(dim=0, keepdim=True)


def bev_image(c, sd, x, start, step_noise, t_start, dtype=torch.float32, decisions=None, x0_index=None):
    """fusion_models/ddp.py:268-301 for one sample from (start, t_start): O.ddim_sample_bev line by line with mask_t = start.
    x (1,Cx,h,w), start (r,256,h,w).  ``decisions`` receives every step's thresholded maps (r,K,H,W) bool."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    h, w = x.shape[-2:]
    K, r = c['Kc'], c['r']
    scopes = CS.bev_scopes(c)
    xr = x.repeat(r, 1, 1, 1)
    mask_t = start.to(dtype).clone()
    outs = []
    with torch.no_grad():
        for t_now, t_next in time_pairs(c, t_start):
            times_now = torch.tensor([t_now], dtype=torch.float32)
            times_next = torch.tensor([t_next], dtype=torch.float32)
            feat = F.conv2d(torch.cat([xr, mask_t], dim=1), sd['transform.conv.weight'], sd['transform.conv.bias'])
            log_snr = O.alpha_cosine_log_snr(times_now)
            log_snr_next = O.alpha_cosine_log_snr(times_next)
            alpha, sigma = O.log_snr_to_alpha_sigma(log_snr.view(-1, 1, 1, 1))
            alpha_next, sigma_next = O.log_snr_to_alpha_sigma(log_snr_next.view(-1, 1, 1, 1))
            temb = O.time_mlp(log_snr, sd)
            prob = O.head_forward_bev(feat, temb, sd, 'gridsample', **scopes)
            pred = (prob > c['threshold'])
            if decisions is not None:
                decisions.append(pred.clone())
            pred = pred * (torch.arange(K) + 1).view(1, K, 1, 1)
            pred = F.interpolate(pred.float(), size=(h, w), mode='nearest').to(torch.int64)
            e = F.embedding(pred, sd['embedding_table.weight']).mean(dim=1).permute(0, 3, 1, 2)
            x0 = (torch.sigmoid(e) * 2 - 1) * c['bit_scale']
            pred_noise = (mask_t - alpha * x0) / sigma.clamp(min=1e-8)
            mask_t = x0 * alpha_next + pred_noise * sigma_next
            outs.append(prob)
    return torch.cat(outs, dim=0).mean(dim=0, keepdim=True)


IMAGE = {'seg': seg_image, 'depth': depth_image, 'bev': bev_image}


def run_from(c, starts, t_start, dtype=torch.float32, record=None, x0_index=None):
    """(B, ...) output of the expectation loop from the start maps ``starts`` (B, r, Cm, h, w), image by image.  ``record``: a list
    that receives, per image, the list of the K per-step decisions.  ``x0_index`` (seg): (K, B, r, h, w) decisions to feed back."""
    sd = state_dict(c)
    x, _, sn = CS.inputs(c)
    outs = []
    for b in range(c['B']):
        rec = [] if record is not None else None
        xi = None if x0_index is None else [x0_index[s, b] for s in range(c['K'])]
        outs.append(IMAGE[c['task']](c, sd, x[b:b + 1], starts[b], None if sn is None else sn[:, b], t_start, dtype, decisions=rec,
                                     x0_index=xi))
        if record is not None:
            record.append(rec)
    return torch.cat(outs, 0)


def starts_of(c, prior_map, t_start, dtype=torch.float32, noise=None):
    """(B, r, Cm, h, w) start maps of the case's batch for ``prior_map`` (B, h, w) and the case's noise (or ``noise``)"""
    sd = state_dict(c)
    if noise is None:
        noise = CS.inputs(c)[1]
    return torch.stack([start_map(c, sd, prior_map[b], noise[b], t_start, dtype) for b in range(c['B'])], 0)


_EXPECT = {}


def expected(c, which=0, dtype=torch.float32, t_start=None):
    """-> (out (B, ...), record) of the case's prior ``which`` (0, 1; 'noise': the noise-start run at the same t_start) from
    ``t_start`` (default: the case's); computed once per key and process and never modified.  record: (K, B, r, h, w) uint8 for seg
    (every step's argmax), None otherwise."""
    t = c['t_start'] if t_start is None else t_start
    key = (c['name'], which, dtype, t)
    if key not in _EXPECT:
        if which == 'noise':
            starts = CS.inputs(c)[1].to(dtype)
        else:
            starts = starts_of(c, prior(c, which), t, dtype)
        rec = []
        out = run_from(c, starts, t, dtype, record=rec)
        record = torch.stack([torch.stack(r, 0) for r in rec], 1) if c['task'] == 'seg' else None     # (K, B, r, h, w)
        _EXPECT[key] = (out, record)
    return _EXPECT[key]


def routes(c):
    """(id, gemm, flags): both engines and every flag that selects another route for the case (tests/test_config_space_gpu.py)"""
    v = [('bf16x3', 'bf16x3', {}), ('f32', 'f32', {}), ('unfused-layer', 'bf16x3', dict(fused_layer=False)),
         ('unfused-prologue', 'bf16x3', dict(fused_prologue=False)), ('gather-refill', 'bf16x3', dict(gather_guess_zero=True))]
    if c['task'] == 'seg' and c['sampler'] == 'ddim':
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
        if c['r'] == 1:
            v.append(('sb-head', 'bf16x3', dict(nchw_head=False)))
    if c['task'] == 'seg' and c['sampler'] == 'ddpm':
        v += [('chain', 'bf16x3', dict(ddpm_chain=True)), ('chain-unfused-tail', 'bf16x3', dict(ddpm_chain=True, fused_tail=False)),
              ('chain-sb-head', 'bf16x3', dict(ddpm_chain=True, nchw_head=False))]
    if c['task'] == 'bev' or (c['task'] == 'depth' and not c['n_bins']):
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
    return v


def prior_bytes(c):
    """(prior_bytes, start_bytes) of include/ddp_mi355x.h as formulas of the case"""
    n = c['B'] * c['h'] * c['w']
    return n * (1 if c['task'] == 'seg' else 4), n * c['r'] * (1 if c['task'] == 'depth' else 256) * 4
