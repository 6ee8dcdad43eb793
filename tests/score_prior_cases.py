"""DDP_FLAG_SCORE_PRIOR: the cases shared by tests/test_score_prior_host.py (CPU) and tests/test_score_prior_gpu.py (GPU), their prior
maps and the EXPECTATION - the oracle's own sampler (oracle.ddp_oracle.ddim_sample_seg / ddpm_sample_seg), one image per call like the
reference's, through its ``head=`` hook, which returns ``O.head_forward_seg(...) + clamp(prior[b])`` (the hook
tests/class_prior_cases.oracle_image records with).  The code under test is never its own reference.

Semantics under test (include/ddp_mi355x.h, "score prior"): entry [b][k][n] of the (B, num_classes, h, w) map is added to the conv_seg
score of class k at pixel n of image b, for all r replicas and all K steps, in front of everything that reads the score; NaN reads as
0, every value is clamped to [-1e30, 1e30], so -inf excludes a class at a pixel with a finite score and a softmax term of exactly 0.

A case is a dict of tests/config_space_cases.py (same builders); L = 2, K in {1, 2, 3}.  The shapes are the smallest at which picking
the row of a token's pixel, or the (B, Kc, N) -> (B N, KP) transpose of k_score_prior_rows (64 pixels x 64 classes per block), can
go wrong:
  kc19_7x13_b3        N = 91: every image border falls inside a 32-token tile; a second, partial pixel tile
  kc19_8x12_b2        N = 96: the borders are tile borders
  kc255_5x10_r2       r = 2: both replicas of a pixel read one row; four class chunks with one class missing
  kc256_3x11          four whole class chunks
  kc150_9x14_noacc    three class chunks, N = 126 (two pixel tiles, the second two short), the last step's scores are the output
  kc64_4x9, kc65_4x9  the chunk edge of KP: 64 -> one whole chunk, 65 -> a second chunk with one class
  kc1_1x37            one class: KP = 64 with 63 padding columns; nothing to decide (no witness)
  kc19_37x1           one column
  kc19_1x1_b3         N = 1: three images in one tile, one-pixel rows
  ddpm_7x13           the ddpm sampler (and its chain)

Maps (``prior_map(c, kind)`` -> (B, Kc, h, w) float32):
  'soft'   +-3 on a seeded third of the (pixel, class) entries: another row at every pixel
  'excl'   -inf, at each pixel, on the class that pixel decides WITHOUT a prior (the argmax of the flag-clear expectation's output).
           Witness: every such pixel's final decision changes and the excluded class is never decided there at any step
  'odd'    the soft map with NaN, +inf and -inf entries: what the normalisation is for
  'const'  a class-prior row per image (tests/class_prior_cases.rows, 'soft') broadcast over the pixels
  'zero'   all zeros
  'both'   (three cases, ``BOTH``) the soft map of the kind's own seed together with the class-prior rows of 'const': both priors

Seeds.  The model and the inputs of a case are drawn per kind for 'soft', 'excl' and 'both' (``c['seeds'][kind]``): a seed is kept only if, in
fp64, the top-2 margin of every pixel at every step of that kind's expectation is >= MARGIN = 1e-3 of the step's largest score - five
times the parity bar REL, so a GPU result within REL takes the same decisions and no pixel is excused anywhere.  The seeds below are
the first that do, counted up from the case's ``base`` = 3000 + 100 * case index (``first_seed`` is the search, run on the CPU: between
1 and 135 oracle runs per case and kind, 434 and 1291 for the 150-class case).  tests/test_score_prior_host.py repeats the last
SEARCH_WINDOW steps of each search - every seed of the window in front of the chosen one fails the rule, the chosen one meets it - so
that the test takes seconds, not the minutes of the whole search.  'odd', 'const' and 'zero' run on the 'soft' seed: their results are compared bit for bit with another call's, not
decision by decision."""
import torch

import class_prior_cases as PC
import config_space_cases as CS
from oracle import ddp_oracle as O

REL = CS.REL
COND = CS.COND
CLAMP = PC.CLAMP
MARGIN = PC.MARGIN
clamp = PC.clamp
max_rel = PC.max_rel
round256 = PC.round256
routes = PC.routes          # both engines and every flag that selects another route: the class prior's table

CASES = {}


def rel_live(got, want, total):
    """max-rel over the entries the prior leaves in (an excluded entry's score is -1e30 on both sides: it would be the whole scale)"""
    live = clamp(total) > -CLAMP
    if not bool(live.any()):                                               # (one class, excluded everywhere: the uniform shift)
        live = torch.ones_like(live)
    d = (got.double() - want.double()).abs()[live].max()
    return float(d / want.double()[live].abs().max())


def _add(name, soft, excl, both=None, **kw):
    c = dict(name='sp_' + name, family='score_prior', task='seg', B=2, r=1, K=2, L=2, Cx=256, td=1, witness=True,
             Kc=19, bit_scale=0.01, accumulation=True, sampler='ddim', base=3000 + 100 * len(CASES))
    c.update(kw)
    c['seeds'] = dict(soft=soft, excl=excl, **({} if both is None else dict(both=both)))
    assert name not in CASES
    CASES[name] = c


_add('kc19_7x13_b3', 3024, 3058, both=3017, h=7, w=13, B=3, K=2)
_add('kc19_8x12_b2', 3134, 3160, h=8, w=12, K=3)
_add('kc255_5x10_r2', 3200, 3207, both=3273, h=5, w=10, Kc=255, r=2, K=2)
_add('kc256_3x11', 3300, 3305, h=3, w=11, Kc=256, K=2)
_add('kc150_9x14_noacc', 3833, 4690, h=9, w=14, Kc=150, accumulation=False, K=2)
_add('kc64_4x9', 3505, 3500, h=4, w=9, Kc=64, K=2)
_add('kc65_4x9', 3605, 3603, h=4, w=9, Kc=65, K=2)
_add('kc1_1x37', 3700, 3700, h=1, w=37, Kc=1, K=2, witness=False)
_add('kc19_37x1', 3800, 3805, h=37, w=1, K=2)
_add('kc19_1x1_b3', 3900, 3900, h=1, w=1, B=3, K=1)
_add('ddpm_7x13', 4021, 4134, both=4020, h=7, w=13, sampler='ddpm', K=3)

SEEDED_KINDS = ('soft', 'excl')
BOTH = [n for n, c in CASES.items() if 'both' in c['seeds']]      # the cases that also run with DDP_FLAG_CLASS_PRIOR on top
KINDS = ('soft', 'excl', 'odd', 'const', 'zero')


def seeded(c, kind):
    """the case with the model / input seed of ``kind`` ('odd', 'const', 'zero' and 'none' run on the soft seed)"""
    if 'seed' in c:
        return c
    k = kind if kind in c['seeds'] else 'soft'
    return dict(c, seed=c['seeds'][k], name=f"{c['name']}/{k}{c['seeds'][k]}")


def kp(c):
    """row length of the library's rows buffer: whole 64-class chunks"""
    return (c['Kc'] + 63) // 64 * 64


def prior_bytes(c):
    """(map_bytes, rows_bytes) of include/ddp_mi355x.h as formulas of the case"""
    n = c['B'] * c['h'] * c['w']
    return n * c['Kc'] * 4, n * kp(c) * 4


def rows_of(pm, c):
    """what k_score_prior_rows must write for the map ``pm``: (B N, KP) normalised, token-major, zero padded"""
    B, Kc, N = c['B'], c['Kc'], c['h'] * c['w']
    out = torch.zeros(B * N, kp(c))
    out[:, :Kc] = clamp(pm).reshape(B, Kc, N).permute(0, 2, 1).reshape(B * N, Kc)
    return out


def const_rows(c):
    """(B, Kc) class-prior rows of the 'const' map: the class prior family's soft rows on this case"""
    return PC.rows(seeded(c, 'const'), 'soft')


_MAPS = {}


def _soft(c):
    g = torch.Generator().manual_seed(c['seed'] * 16 + 11)
    shape = (c['B'], c['Kc'], c['h'], c['w'])
    on = torch.rand(shape, generator=g) < 1.0 / 3.0
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(3.0), torch.tensor(-3.0))
    return torch.where(on, sign, torch.tensor(0.0))


def prior_map(c, kind):
    """(B, Kc, h, w) float32 map of the case (seeded; the same tensor on every call)"""
    c = seeded(c, kind)
    key = (c['name'], kind)
    if key in _MAPS:
        return _MAPS[key]
    shape = (c['B'], c['Kc'], c['h'], c['w'])
    if kind == 'zero':
        m = torch.zeros(shape)
    elif kind == 'const':
        m = const_rows(c)[:, :, None, None].expand(shape).contiguous()
    elif kind == 'excl':
        base = expected(c, 'none')['out'].argmax(1)                        # (B, h, w): the decision without a prior
        m = torch.zeros(shape).scatter_(1, base[:, None], float('-inf'))
    else:
        m = _soft(c)
        if kind == 'odd':
            g = torch.Generator().manual_seed(c['seed'] * 16 + 12)
            u = torch.rand(shape, generator=g)
            m = torch.where(u < 0.05, torch.tensor(float('nan')), m)
            m = torch.where((u >= 0.05) & (u < 0.07), torch.tensor(float('inf')), m)
            m = torch.where((u >= 0.07) & (u < 0.12), torch.tensor(float('-inf')), m)
            flat = m.view(-1)                                              # (every kind of entry on every case, the smallest included)
            for i, v in enumerate((float('nan'), float('inf'), float('-inf'))):
                flat[(i * 7) % flat.numel()] = v
    _MAPS[key] = m
    return m


def _margin(scores, prior):
    """min over the pixels of (top1 - top2) / the step's largest |score| among the entries the prior leaves in; inf for one class"""
    if scores.shape[1] < 2:
        return float('inf')
    s = scores.double()
    top = s.topk(2, dim=1).values
    live = (clamp(prior) > -CLAMP)[None].expand_as(s)
    return float(((top[:, 0] - top[:, 1]) / s[live].abs().max()).min())


class _BelowMargin(Exception):
    pass


def _run(c, pm, dtype, class_rows=None, stop_below=None):
    """``stop_below``: raise _BelowMargin at the first step whose top-2 margin is smaller (the seed search needs no more of the run)"""
    sd = {k: v.to(dtype) for k, v in CS.state_dict(c).items()}
    x, noise, sn = CS.inputs(c)
    outs, recs, margin = [], [], float('inf')
    for b in range(c['B']):
        add = clamp(pm[b]).to(dtype)
        cadd = None if class_rows is None else clamp(class_rows[b]).to(dtype)[:, None, None]
        total = pm[b] if class_rows is None else clamp(pm[b]) + clamp(class_rows[b])[:, None, None]
        rec = []

        def head(feat, temb):
            lg = O.head_forward_seg(feat, temb, sd)
            if cadd is not None:
                lg = lg + cadd
            lg = lg + add
            rec.append(lg)
            if stop_below is not None and _margin(lg, total) < stop_below:
                raise _BelowMargin
            return lg
        outs.append(_sample(c, sd, x, noise, sn, b, dtype, head))
        margin = min([margin] + [_margin(s, total) for s in rec])
        recs.append(torch.stack([s.argmax(1).to(torch.uint8) for s in rec], 0))          # (K, r, h, w)
    return dict(out=torch.cat(outs, 0), record=torch.stack(recs, 1), margin=margin)


def _sample(c, sd, x, noise, step_noise, b, dtype, head):
    xb, nb = x[b:b + 1].to(dtype), noise[b].to(dtype)
    kw = dict(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'], accumulation=c['accumulation'],
              head=head)
    with torch.no_grad():
        if c['sampler'] == 'ddpm':
            return O.ddpm_sample_seg(xb, nb, step_noise[:, b].to(dtype), sd, **kw)
        return O.ddim_sample_seg(xb, nb, sd, **kw)


_EXPECT = {}


def expected(c, kind, dtype=torch.float32, seed_of=None, with_class_rows=False):
    """-> dict(out (B, Kc, h, w), record (K, B, r, h, w) uint8 - every step's argmax -, margin: the smallest top-2 margin of any pixel
    and step relative to the step's largest score among the entries the prior leaves in).  ``kind``: 'none' (the zero map) or a map
    kind; ``seed_of``: the kind whose seed the run uses (default: ``kind``'s); ``with_class_rows``: ``const_rows`` added as a class
    prior on top (both priors).  Computed once per key and process and never modified."""
    c = seeded(c, seed_of or kind)
    with_class_rows = with_class_rows or kind == 'both'
    key = (c['name'], kind, dtype, with_class_rows)
    if key not in _EXPECT:
        pm = torch.zeros(c['B'], c['Kc'], c['h'], c['w']) if kind == 'none' else prior_map(c, 'soft' if kind == 'both' else kind)
        _EXPECT[key] = _run(c, pm, dtype, const_rows(c) if with_class_rows else None)
    return _EXPECT[key]


def qualifies(c, kind, seed):
    """the seed rule of the header for (case, kind): fp64 top-2 margin >= MARGIN at every pixel and step; 'excl': and the witness"""
    cs = dict(c, seed=seed, name=f"{c['name']}/try{kind}{seed}")
    try:
        e = _run(cs, prior_map(cs, 'soft' if kind == 'both' else kind), torch.float64, const_rows(cs) if kind == 'both' else None,
                 stop_below=MARGIN)
        ok = e['margin'] >= MARGIN
        if ok and kind == 'excl' and c['witness']:
            ok = excl_witness(c, expected(cs, 'none')['out'].argmax(1), e)
    except _BelowMargin:
        ok = False
    for k in [k for k in _EXPECT if k[0] == cs['name']]:
        del _EXPECT[k]
    _MAPS.pop((cs['name'], 'soft' if kind == 'both' else kind), None)
    PC._ROWS.pop((cs['name'], 'soft'), None)
    return ok


def excl_witness(c, base, e):
    """every pixel's final decision differs from ``base`` (B, h, w) - the class excluded there - and no step of any replica decides
    the excluded class at that pixel"""
    fin = e['out'].argmax(1)
    never = bool((e['record'].long() != base[None, :, None].long()).all())
    return bool((fin != base).all()) and never


SEARCH_WINDOW = 10


def first_seed(c, kind, start=None, limit=2000):
    """the first seed >= ``start`` (default: the case's base) that meets the rule"""
    start = c['base'] if start is None else start
    for s in range(start, start + limit):
        if qualifies(c, kind, s):
            return s
    raise RuntimeError(f'no seed for {c["name"]}/{kind}')


# flag-clear sampler calls whose output bits are recorded from the parent's build (tests/golden/score_prior/parent_bits.json, written by
# tests/golden/gen_score_prior_parent.py): (case, gemm, engine keywords)
PARENT_BITS = {'kc19_7x13_b3/bf16x3': ('kc19_7x13_b3', 'bf16x3', {}),
               'kc150_9x14_noacc/f32': ('kc150_9x14_noacc', 'f32', {}),
               'kc65_4x9/unfused-layer': ('kc65_4x9', 'bf16x3', dict(fused_layer=False)),
               'ddpm_7x13/chain': ('ddpm_7x13', 'bf16x3', dict(ddpm_chain=True))}


def flag_clear_hashes(dev, lib_path=None):
    """sha256 of the flag-clear output of every PARENT_BITS entry with the library in use (DDP_LIB_PATH or the in-tree build)"""
    import hashlib

    from ddp_amd.engine import DDPEngine
    out = {}
    for key, (name, gemm, kw) in PARENT_BITS.items():
        c = seeded(CASES[name], 'soft')
        x, noise, sn = (None if t is None else t.to(dev) for t in CS.inputs(c))
        eng = DDPEngine(CS.state_dict(c), 'seg', device=dev, gemm=gemm, lib_path=lib_path, **kw, **CS.engine_kwargs(c))
        got = eng.sample(x.contiguous(), noise.contiguous(), None if sn is None else sn.contiguous())
        torch.cuda.synchronize()
        out[key] = hashlib.sha256(got.cpu().numpy().tobytes()).hexdigest()
    return out
