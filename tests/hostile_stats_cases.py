"""The hostile-statistics sweep shared by tests/test_hostile_stats_gpu.py (GPU: every case, route and engine variant against
the fp64 oracle) and tests/test_hostile_stats_host.py (CPU: determinism, conditioning of the oracle, a witness that the case does
what its name says).

Every other parity test draws from one benign family (``ddp_amd.utils.synthetic``): N(0, 1) features and noise, Xavier weights,
LayerNorm gamma 1 +- 0.1, O(1) attention logits, small FiLM vectors.  A case here is that benign seeded model and input plus ONE
named mutation of the statistics that flow through the dense arithmetic - LayerNorm0, LayerNorm1 x FiLM, the bf16 splits of
their outputs, GELU, the 4-point softmax, the head - on the three LayerNorm implementations of the library (the fused layer
kernel, the epilogue of the unfused bf16x3 tile GEMMs, the epilogue of the exact-product engine).

Routes (``c['routes']``):
  head   ``ddp_head_forward`` on a (1, 256, h, w) map and a time embedding: no feedback, no transform convolution
  step1  ``ddp_sample`` with one step and no accumulation: the product path's step head, layers and fused tail, no feedback
  tf2    two steps with accumulation, the fp32 oracle's argmax decisions fed to every side (DDP_FLAG_FORCE_X0)
The depth and bev cases run the head route only (bev: grid transform in front of the encoder, sigmoid behind conv_seg).

Where a mutation is of "the map": on the head route it is applied to the feature map the head receives; on the sampler routes
to x AND to the start noise (the two 256-channel maps the transform convolution mixes), so that the mutated statistics reach the
first layer.  The ``x_*`` / ``noise_*`` / ``transform_*`` cases of the sampler family mutate the one tensor they name.

Cases that rescale activations freeze the gather geometry (``sampling_offsets.weight`` = ``attention_weights.weight`` = 0 in
every layer): sampling offsets and attention weights are then the same for every token whatever the content, and the case
isolates the dense path instead of moving taps around.  With the geometry frozen everything in front of LayerNorm0 is linear,
so the ``scale_*`` cases scale the additive constants in front of it too (``transform.conv.bias``, layer 0's
``value_proj.bias`` / ``output_proj.bias``): LayerNorm0's input is then the benign row times the factor, not the factor's
floor under a 0.02 bias.

Cases that replace an ill-conditioned one of their family (the fp32 oracle itself further than CAP from its fp64 evaluation, or so
close to CAP that the figure depends on the host's thread count):
  softmax_onehot   attention logits x 40 in the bias and x 10 in the weight.  With x 40 on the weight too the fp32 oracle is
                   1.5e-6 .. 1.4e-5 from fp64 depending on seed and thread count (single tokens at a near-tie of two points, where
                   the content-dependent logits amplify rounding); with x 10 it is 0.8e-6 .. 1.6e-6 and the weights are still one-hot
                   (> 0.999) on more than 70 % of (token, head) pairs
  ln_affine_soft   the tf2 route of ln_affine (and the bev head's), conv_seg x 0.05: the accumulated output is a softmax of the scores
                   (bev: a sigmoid), and at a score scale of 100 .. 160 the fp32 oracle's probabilities are 0.5e-5 .. 1.3e-5 from fp64
  head_cancel_3    the tf2 route of head_cancel with conv_seg x 3 instead of x 50 (score scale 250: 2e-5 .. 3e-5), rows mirrored alike
  dc_50_ln0        an addition to the family: in dc_100 / dc_1e4 layer 0's value projection spreads the offset over the channels, so
                   LayerNorm0's row has |mean| / std of about 1.2; here the offset reaches it through the residual alone (> 25)

The bar (tests/test_hostile_stats_gpu.py): err = max|out - r64| / max|r64| <= 4 x max(E_ref(case), E_ref(benign of the same
shape, layers, classes and route)), E_ref the same figure of the fp32 oracle; every case must have E_ref <= CAP."""
import torch
import torch.nn.functional as F

from ddp_amd.utils import synthetic
from oracle import ddp_oracle as O

CAP = 1e-5              # a case whose fp32 oracle is further than this from its own fp64 evaluation is replaced, never kept
FACTOR = 4              # tests/test_hip_parity.py: "within 4 x the reference's distance to the fp64 oracle"
BIT_SCALE = 0.01
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0
SHAPES = {'9x13': (9, 13), '11x24': (11, 24)}     # 117 tokens: one partial 128-token tile; 264: two tiles + 8, groups straddle rows

CASES = {}
_TASK_SUFFIX = {'seg': '', 'depth': '-depth', 'bev': '-bev'}
BEV_GRID = (2, 3)       # bev: the head grid is (h + 2) x (w + 3), so the grid transform resamples (11 x 16 = 176 tokens at 9 x 13)


def _add(mutation, family, shape, *, task='seg', L=2, Kc=19, routes=('head', 'step1'), freeze=False):
    name = f'{mutation}-{shape}' + ('' if L == 2 else f'-L{L}') + ('' if Kc in (1, 6, 19) else f'-k{Kc}') + _TASK_SUFFIX[task]
    h, w = SHAPES[shape]
    assert name not in CASES
    CASES[name] = dict(name=name, mutation=mutation, family=family, shape=shape, h=h, w=w, task=task, L=L, Kc=Kc, routes=tuple(routes),
                       freeze=freeze, seed=900 + h)        # one benign model and input per shape: the mutation is the only difference


for _s in SHAPES:
    _add('benign', 'benign', _s, routes=('head', 'step1', 'tf2'))
    for _m in ('scale_1e3', 'scale_1e-3', 'scale_1e-6', 'scale_1e-30'):
        _add(_m, 'feature_scale', _s, freeze=True)
    for _m in ('dc_100', 'dc_1e4'):
        _add(_m, 'dc_offset', _s, freeze=True)
    # (head route only: behind the transform convolution the fp32 oracle itself is 2e-5 .. 3e-5 from fp64 with an offset of 100;
    # + 50 rather than + 100: with + 100 the fp32 oracle sits 7e-6 from fp64, too close to the cap to hold on every host)
    _add('dc_50_ln0', 'dc_offset', _s, routes=('head',), freeze=True)
    for _m in ('const_rows', 'zero_map', 'zero_cols'):
        _add(_m, 'degenerate_rows', _s, freeze=True)
    _add('ln_affine', 'ln_affine', _s, freeze=True)
    _add('ln_affine_soft', 'ln_affine', _s, routes=('tf2',), freeze=True)
    _add('film', 'film', _s, routes=('head', 'step1', 'tf2'))
    _add('gelu_tails', 'gelu_tails', _s, freeze=True)
    _add('softmax_onehot', 'attention_softmax', _s)
    _add('softmax_ties', 'attention_softmax', _s)
    _add('head_cancel', 'head', _s)
    _add('head_cancel_3', 'head', _s, routes=('tf2',))
    for _m in ('x_1e3', 'x_1e-6', 'x_dc_100', 'noise_1e3', 'transform_30'):
        _add(_m, 'sampler_inputs', _s, routes=('step1',), freeze=True)
    _add('benign', 'depth_head', _s, task='depth', Kc=1, routes=('head',))
    _add('dc_100', 'depth_head', _s, task='depth', Kc=1, routes=('head',), freeze=True)
# the last-layer / no-next-layer branch of the fused kernel under the LayerNorm and FiLM families
_add('benign', 'benign', '9x13', L=1, routes=('head', 'step1', 'tf2'))
_add('ln_affine', 'ln_affine', '9x13', L=1, freeze=True)
_add('film', 'film', '9x13', L=1, routes=('head', 'step1', 'tf2'))
_add('ln_affine_soft', 'ln_affine', '9x13', L=1, routes=('tf2',), freeze=True)
# more than one class chunk live in the fused tail
_add('benign', 'benign', '11x24', Kc=150, routes=('head', 'step1', 'tf2'))
_add('head_cancel', 'head', '11x24', Kc=150)
_add('head_cancel_3', 'head', '11x24', Kc=150, routes=('tf2',))
# the BEV head's one-step route (grid transform in front of the encoder, sigmoid behind conv_seg; its sampler thresholds x0 and is
# left out): the norm families; ln_affine with conv_seg x 0.05, as on tf2 - a sigmoid of scores of scale 100 is ill-conditioned
for _m, _f in (('benign', False), ('scale_1e-6', True), ('dc_100', True), ('ln_affine_soft', True), ('film', False)):
    _add(_m, 'bev_head', '9x13', task='bev', Kc=6, routes=('head',), freeze=_f)
# teacher-forced only: the x0 table (sigmoid of the embedding) saturated
_add('embedding_1e2', 'embedding', '9x13', routes=('tf2',))

ROUTES = ('head', 'step1', 'tf2')
THIRD = slice(0, 256, 3)          # the channels on which FiLM's scale is exactly -1


def names(family=None, route=None):
    return [n for n, c in CASES.items() if (family is None or c['family'] == family) and (route is None or route in c['routes'])]


def benign_of(c):
    """the yardstick case of ``c``: same shape, layers, classes and task, no mutation"""
    return CASES[f'benign-{c["shape"]}' + ('' if c['L'] == 2 else f'-L{c["L"]}') + ('' if c['Kc'] in (1, 6, 19) else f'-k{c["Kc"]}') +
                 _TASK_SUFFIX[c['task']]]


def bev_scopes(c):
    """grid_transform of the bev head: input scope = the map, output scope = BEV_GRID more rows / columns over a slightly smaller range"""
    h, w = c['h'], c['w']
    return dict(input_scope=[[-51.2, 51.2, 102.4 / h], [-51.2, 51.2, 102.4 / w]],
                output_scope=[[-50, 50, 100.0 / (h + BEV_GRID[0])], [-50, 50, 100.0 / (w + BEV_GRID[1])]])


def _layers(c):
    return [f'decode_head.encoder.layers.{l}.' for l in range(c['L'])]


def _scale_of(c):
    m = c['mutation']
    return float(m.split('_', 1)[1]) if m.startswith('scale_') else None


def state_dict(c):
    """the benign seeded model of the case's shape with the case's mutation of the WEIGHTS applied (fp32, CPU)"""
    sd = synthetic.make_state_dict(c['task'], c['Kc'], c['L'], 256, seed=c['seed'])
    g = torch.Generator().manual_seed(c['seed'] + 50)
    m = c['mutation']
    if c['freeze']:
        for p in _layers(c):
            sd[p + 'attentions.0.sampling_offsets.weight'].zero_()
            sd[p + 'attentions.0.attention_weights.weight'].zero_()
    s = _scale_of(c)
    if s is not None:
        for k in ('transform.conv.bias', _layers(c)[0] + 'attentions.0.value_proj.bias', _layers(c)[0] + 'attentions.0.output_proj.bias'):
            sd[k] *= s
    if m == 'dc_50_ln0':
        # the offset reaches LayerNorm0 through the residual alone: layer 0's value projection is made blind to a constant
        # (zero row sums).  In the plain dc cases W_v spreads the offset over the channels and the row's std grows with its mean
        wv = sd[_layers(c)[0] + 'attentions.0.value_proj.weight']
        wv -= wv.mean(dim=1, keepdim=True)
    if m in ('ln_affine', 'ln_affine_soft'):
        if m == 'ln_affine_soft':
            sd['decode_head.conv_seg.weight'] *= 0.05
        for p in _layers(c):
            for n in (0, 1):
                mag = 10.0 ** (torch.rand(256, generator=g) * 4 - 2)                     # log-uniform over 1e-2 .. 1e2
                sign = torch.where(torch.rand(256, generator=g) < 0.5, -1.0, 1.0)
                gam = mag * sign
                gam[::17] = 0.0
                sd[p + f'norms.{n}.weight'] = gam
                sd[p + f'norms.{n}.bias'] = torch.randn(256, generator=g) * 10.0
    elif m == 'film':
        for p in _layers(c):
            sd[p + 'time_mlp.1.weight'].zero_()
            b = sd[p + 'time_mlp.1.bias']
            b[:256][THIRD] = -1.0
            b[256:] = 5.0
    elif m == 'gelu_tails':
        for p in _layers(c):
            sd[p + 'ffns.0.layers.0.0.weight'] *= 16.0
            sd[p + 'ffns.0.layers.0.0.bias'] = torch.randn(1024, generator=g) * 4.0
    elif m == 'softmax_onehot':
        for p in _layers(c):
            sd[p + 'attentions.0.attention_weights.weight'] *= 10.0      # (see the module docstring: x 40 here is ill-conditioned)
            sd[p + 'attentions.0.attention_weights.bias'] *= 40.0
    elif m == 'softmax_ties':
        for p in _layers(c):
            sd[p + 'attentions.0.attention_weights.weight'].zero_()
            sd[p + 'attentions.0.attention_weights.bias'].zero_()
    elif m in ('head_cancel', 'head_cancel_3'):
        wt = sd['decode_head.conv_seg.weight'] * (50.0 if m == 'head_cancel' else 3.0)
        wt[1::2] = -wt[0:wt.shape[0] - 1:2]
        sd['decode_head.conv_seg.weight'] = wt
    elif m == 'transform_30':
        sd['transform.conv.weight'] *= 30.0
    elif m == 'embedding_1e2':
        sd['embedding_table.weight'] *= 100.0
    return sd


def _mutate_map(c, t):
    """the case's mutation of a (..., 256, h, w) map"""
    m = c['mutation']
    s = _scale_of(c)
    if s is not None:
        return t * s
    if m == 'dc_100':
        return t + 100.0
    if m == 'dc_50_ln0':
        return t + 50.0
    if m == 'dc_1e4':
        return t + 1e4
    t = t.clone()
    if m == 'const_rows':
        t[..., 1::2, :] = t[..., 1::2, :1]                 # alternate map rows: every token of the row is the row's first token
    elif m == 'zero_map':
        t.zero_()
    elif m == 'zero_cols':
        t[..., ::3] = 0.0
    return t


def degenerate_mask(c):
    """(h, w) bool: the tokens the degenerate-row cases make constant or zero (None for every other case)"""
    mask = torch.zeros(c['h'], c['w'], dtype=torch.bool)
    if c['mutation'] == 'const_rows':
        mask[1::2] = True
    elif c['mutation'] == 'zero_map':
        mask[:] = True
    elif c['mutation'] == 'zero_cols':
        mask[:, ::3] = True
    else:
        return None
    return mask


def head_inputs(c):
    """-> feat (1, 256, h, w), temb (1, 1024): what ``ddp_head_forward`` / ``O.head_forward_*`` receive (fp32, CPU)"""
    feat, _ = synthetic.make_inputs(1, c['h'], c['w'], 1, 256, 256, seed=c['seed'] + 1)
    sd = state_dict(c)
    t_in = torch.tensor([1.0]) if c['task'] == 'depth' else O.alpha_cosine_log_snr(torch.tensor([1.0]))
    return _mutate_map(c, feat).contiguous(), O.time_mlp(t_in, sd)


def sampler_inputs(c):
    """-> x (1, 256, h, w), noise (1, 1, 256, h, w) of the sampler routes"""
    x, noise = synthetic.make_inputs(1, c['h'], c['w'], 1, 256, 256, seed=c['seed'] + 2)
    m = c['mutation']
    if m == 'x_1e3':
        x = x * 1e3
    elif m == 'x_1e-6':
        x = x * 1e-6
    elif m == 'x_dc_100':
        x = x + 100.0
    elif m == 'noise_1e3':
        noise = noise * 1e3
    elif m == 'zero_cols':
        x, noise = _mutate_map(c, x), torch.zeros_like(noise)       # the zeroed columns enter the encoder as the transform's bias
    else:
        x, noise = _mutate_map(c, x), _mutate_map(c, noise)
    return x.contiguous(), noise.contiguous()


def engine_kwargs(c, route):
    kw = dict(h=c['h'], w=c['w'], batch=1, randsteps=1, bit_scale=BIT_SCALE)
    if c['task'] == 'depth':
        kw.update(timesteps=1, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
        return kw
    if c['task'] == 'bev':
        s = bev_scopes(c)
        kw.update(timesteps=1, num_classes=c['Kc'], bev_input_scope=s['input_scope'], bev_output_scope=s['output_scope'])
        return kw
    kw.update(num_classes=c['Kc'], timesteps=2 if route == 'tf2' else 1, accumulation=route == 'tf2', force_x0=route == 'tf2')
    return kw


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


_ORACLE = {}


def oracle_pair(c, route):
    """-> dict(r32, r64, e_ref, scale[, decisions]): the fp32 and the fp64 oracle of (case, route), computed once per process.
    e_ref = max|r32 - r64| / max|r64|.  tf2: ``decisions`` (2, 1, h, w) are the fp32 oracle's own argmax maps, fed to the fp64
    run (and by the GPU test to the engine), so r32 is the free-running fp32 reference and no side takes a decision of its own."""
    key = (c['name'], route)
    if key in _ORACLE:
        return _ORACLE[key]
    assert route in c['routes'], key
    sd = state_dict(c)
    res = {}
    with torch.no_grad():
        if route == 'head':
            feat, temb = head_inputs(c)
            for dt, k in ((torch.float32, 'r32'), (torch.float64, 'r64')):
                if c['task'] == 'depth':
                    res[k] = O.head_forward_depth(feat.to(dt), temb.to(dt), _cast(sd, dt), MIN_DEPTH)
                elif c['task'] == 'bev':
                    res[k] = O.head_forward_bev(feat.to(dt), temb.to(dt), _cast(sd, dt), **bev_scopes(c))
                else:
                    res[k] = O.head_forward_seg(feat.to(dt), temb.to(dt), _cast(sd, dt))
        else:
            x, noise = sampler_inputs(c)
            K, acc = (2, True) if route == 'tf2' else (1, False)
            dec = []
            res['r32'] = O.ddim_sample_seg(x, noise[0], sd, timesteps=K, randsteps=1, bit_scale=BIT_SCALE, accumulation=acc, decisions=dec)
            idx = [d.long() for d in dec]
            res['r64'] = O.ddim_sample_seg(x.double(), noise[0].double(), _cast(sd, torch.float64), timesteps=K, randsteps=1,
                                           bit_scale=BIT_SCALE, accumulation=acc, x0_index=idx)
            res['decisions'] = torch.stack(dec)
    res['scale'] = float(res['r64'].abs().max())
    res['e_ref'] = err_vs(res['r32'], res['r64'])
    _ORACLE[key] = res
    return res


def err_vs(out, r64):
    """max|out - r64| / max|r64|: the suite's max-rel, taken against the fp64 oracle"""
    return float((out.double() - r64).abs().max() / r64.abs().max().clamp(min=1e-300))


def bar_of(c, route):
    """-> (bar, e_ref of the case, e_ref of its benign yardstick); nothing here is measured on the code under test"""
    e, eb = oracle_pair(c, route)['e_ref'], oracle_pair(benign_of(c), route)['e_ref']
    return FACTOR * max(e, eb), e, eb


def fingerprint(c):
    """sum and sum of magnitudes (golden_util.fingerprint) over the case's weights and the inputs of its routes"""
    from golden_util import fingerprint as fp
    out = [synthetic.checksum(state_dict(c))]
    if 'head' in c['routes']:
        out += [v for t in head_inputs(c) for v in fp(t)]
    if 'step1' in c['routes'] or 'tf2' in c['routes']:
        out += [v for t in sampler_inputs(c) for v in fp(t)]
    return out


def first_map(c, route):
    """the (1, 256, h, w) map the encoder receives first on ``route`` (fp32): the head's input or the transform convolution's
    output of step 0"""
    if route == 'head':
        return head_inputs(c)
    sd = state_dict(c)
    x, noise = sampler_inputs(c)
    feat = F.conv2d(torch.cat([x, noise[0]], dim=1), sd['transform.conv.weight'], sd['transform.conv.bias'])
    return feat, O.time_mlp(O.alpha_cosine_log_snr(torch.tensor([1.0])), sd)


def layer_witness(c, route):
    """Intermediates of every layer of the case, from the oracle's own pieces in fp32 (nothing of its behaviour changes): per
    layer a dict of
      ln0_in   (N, 256) LayerNorm0's input (attention output + residual)
      fc1      (N, 1024) pre-activations of the GELU
      attn     (N, 8, 4) softmax weights
      offsets  (N, 64) sampling offsets in pixels
      folded_gamma  (256,) gamma1 x (1 + scale): what k_fold_affine makes of LayerNorm1 and FiLM"""
    sd = state_dict(c)
    feat, temb = first_map(c, route)
    h, w = c['h'], c['w']
    pos = O.sine_positional_encoding(h, w).flatten(1).transpose(0, 1)
    q = feat.flatten(2).transpose(1, 2)
    out = []
    with torch.no_grad():
        for l, p in enumerate(_layers(c)):
            a = p + 'attentions.0.'
            qp = q + pos[None]
            y = O.msda_forward(q, pos, h, w, sd, a)
            q1 = F.layer_norm(y, (256,), sd[p + 'norms.0.weight'], sd[p + 'norms.0.bias'], 1e-5)
            scale, _ = O.film_vectors(temb, sd, l)
            out.append(dict(ln0_in=y[0], fc1=F.linear(q1, sd[p + 'ffns.0.layers.0.0.weight'], sd[p + 'ffns.0.layers.0.0.bias'])[0],
                            attn=F.linear(qp, sd[a + 'attention_weights.weight'], sd[a + 'attention_weights.bias']).view(-1, 8, 4).softmax(-1),
                            offsets=F.linear(qp, sd[a + 'sampling_offsets.weight'], sd[a + 'sampling_offsets.bias'])[0],
                            folded_gamma=sd[p + 'norms.1.weight'] * (1 + scale[0])))
            q = O.encoder_layer(q, pos, temb, h, w, sd, l)
    return out


def top2_gap(r):
    """(h, w) gap between the two largest class scores of a (1, K, h, w) map"""
    t = r[0].topk(2, dim=0).values
    return t[0] - t[1]
