"""DDP_FLAG_CLASS_PRIOR: the cases shared by tests/test_class_prior_host.py (CPU) and tests/test_class_prior_gpu.py (GPU), their prior
rows and the EXPECTATION - the oracle's own sampler (oracle.ddp_oracle.ddim_sample_seg / ddpm_sample_seg), one image per call like the
reference's, on a state dict whose ``conv_seg.bias`` is fl32(bias + clamp(prior[b])).  The code under test is never its own reference.

Semantics under test (include/ddp_mi355x.h, "class prior"): row b of the (B, 256) table is added to the conv_seg scores of image b at
every token, replica and step, in front of everything that reads them; NaN reads as 0, every value is clamped to [-1e30, 1e30], so
-inf excludes a class with a finite score and a softmax term of exactly 0.

A case is a dict of tests/config_space_cases.py (same builders); L = 2, K in {1, 2, 3}.  The shapes are the smallest at which picking
the row of a token's image can go wrong in a 32-token tile:
  kc19_7x13_b3        r N = 91: every image boundary falls inside a tile
  kc19_8x12_b2        N = 96: the boundaries are tile boundaries
  kc150_9x14_noacc    three class chunks, the last step's scores are the output
  kc255_5x10_r2       r = 2 (r N = 100), four class chunks with one class missing
  kc256_3x11          four whole class chunks
  kc1_1x37_b3         one class: nothing to decide (no witness - see ``witness``)
  kc19_1x1_b3         three images in one tile
  ddpm_7x13           the ddpm sampler

Rows (``rows(c, kind)`` -> (B, Kc) float32, another row for every image):
  'soft'   +-3 on a third of the classes (at least one class, seeded per image; with more than one class at least one +3)
  'excl'   -inf on the classes that win most pixels WITHOUT a prior - the fewest top classes of the image's flag-clear decision map that
           together hold >= 10 % of its pixels (and never all classes but for the one-class case, where it is the uniform shift)
  'odd'    the soft row with NaN on its first class, +inf on one more and -inf on another: what the normalisation is for

Seeds.  The model and the inputs of a case are drawn per KIND of row (``c['seeds'][kind]``; ``seeded(c, kind)`` is the case with that
seed): a seed is kept only if, in fp64, the top-2 margin of every pixel at every step of that kind's expectation is >= MARGIN = 1e-3
of the step's largest score - five times the parity bar REL, so a GPU result within REL takes the same decisions and no pixel needs
to be excused - and the witness below holds.  With 130 .. 580 pixel-steps per case between one seed in 3 and one in 420 qualifies, for one kind;
the seeds below are the first that do, counted up from 1300 + 100 * case index (tests/test_class_prior_host.py asserts it for each).
The 'odd' rows run on the 'soft' seed (its expectation is compared bit for bit with another table, not decision by decision).

``witness``: False for exactly one case, the one-class model - its score map has one channel, every argmax is class 0 under any prior."""
import torch

import config_space_cases as CS
from oracle import ddp_oracle as O
from support import max_rel64 as max_rel, round256  # noqa: F401  (the float64 measure: P.max_rel at every call site)

REL = CS.REL
COND = CS.COND
CLAMP = 1e30
MARGIN = 1e-3          # fp64 top-2 margin / the step's largest score, at every pixel and step of every expectation
WITNESS_PIXELS = 0.1   # share of an image's pixels whose final decision the prior must change / the excluded classes must have held

CASES = {}


def _add(name, soft, excl, **kw):
    c = dict(name=name, family='class_prior', task='seg', B=2, r=1, K=2, L=2, Cx=256, td=1, witness=True,
             Kc=19, bit_scale=0.01, accumulation=True, sampler='ddim')
    c.update(kw)
    c['seeds'] = dict(soft=soft, excl=excl)
    assert name not in CASES
    CASES[name] = c


_add('kc19_7x13_b3', 1345, 1316, h=7, w=13, B=3, K=2)
_add('kc19_8x12_b2', 1488, 1402, h=8, w=12, K=3)
_add('kc150_9x14_noacc', 1594, 1576, h=9, w=14, Kc=150, accumulation=False, K=2)
_add('kc255_5x10_r2', 2017, 2022, h=5, w=10, Kc=255, r=2, K=2)
_add('kc256_3x11', 1705, 1710, h=3, w=11, Kc=256, K=2)
_add('kc1_1x37_b3', 1800, 1800, h=1, w=37, Kc=1, B=3, K=2, witness=False)
_add('kc19_1x1_b3', 1902, 1900, h=1, w=1, B=3, K=1)
_add('ddpm_7x13', 2003, 2008, h=7, w=13, sampler='ddpm', K=3)

KINDS = ('soft', 'excl')


def names():
    return list(CASES)


def seeded(c, kind):
    """the case with the model / input seed of ``kind`` ('soft', 'excl'; 'odd' runs on the soft seed)"""
    if 'seed' in c:
        return c
    k = 'soft' if kind == 'odd' else kind
    return dict(c, seed=c['seeds'][k], name=f"{c['name']}/{k}{c['seeds'][k]}")


def clamp(rows):
    """the library's normalisation of a table: NaN -> 0, clamp to [-1e30, 1e30] (fp32)"""
    r = rows.float()
    r = torch.where(torch.isnan(r), torch.zeros_like(r), r)
    return r.clamp(-CLAMP, CLAMP)


def table(c, rows):
    """(B, 256) float32 table of the C surface: the rows, and a NaN poison in the ignored entries k >= num_classes"""
    t = torch.full((rows.shape[0], 256), float('nan'))
    t[:, :c['Kc']] = rows
    return t


def biased_state_dict(c, sd, row, dtype=torch.float32):
    """the model of ONE image under its prior row: conv_seg.bias = fl32(bias + clamp(row)), everything in ``dtype``"""
    out = {k: v.to(dtype) for k, v in sd.items()}
    bias = sd['decode_head.conv_seg.bias'].float()
    out['decode_head.conv_seg.bias'] = (bias + clamp(row)).float().to(dtype)
    return out


def oracle_image(c, sd_b, x, noise, step_noise, b, dtype, record):
    """oracle.ddp_oracle's sampler on image ``b`` with the (already biased, already ``dtype``) state dict; ``record`` receives every
    step's score map (r, Kc, h, w) through the sampler's ``head=`` hook"""
    def head(feat, temb):
        lg = O.head_forward_seg(feat, temb, sd_b)
        record.append(lg)
        return lg
    xb, nb = x[b:b + 1].to(dtype), noise[b].to(dtype)
    kw = dict(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'], accumulation=c['accumulation'],
              head=head)
    with torch.no_grad():
        if c['sampler'] == 'ddpm':
            return O.ddpm_sample_seg(xb, nb, step_noise[:, b].to(dtype), sd_b, **kw)
        return O.ddim_sample_seg(xb, nb, sd_b, **kw)


def _top2_margin(scores, live):
    """min over pixels of (top1 - top2) / max |score| over the classes in ``live`` (the step's largest score); inf for one class"""
    if scores.shape[1] < 2:
        return float('inf')
    top = scores.double().topk(2, dim=1).values
    scale = scores.double()[:, live].abs().max()
    return float(((top[:, 0] - top[:, 1]) / scale).min())


_EXPECT = {}


def expected(c, kind, dtype=torch.float32, seed_of=None):
    """``seed_of``: the kind whose seed the run uses (default: ``kind`` itself; 'none' needs it).
    -> dict(out (B, Kc, h, w), record (K, B, r, h, w) uint8 - every step's argmax -, margin: the smallest top-2 margin of any pixel
    and step relative to the step's largest score among the classes the row leaves in).  ``kind``: 'none' (no prior), 'soft', 'excl',
    'odd'.  Computed once per key and process and never modified."""
    c = seeded(c, seed_of or kind)
    key = (c['name'], kind, dtype)
    if key not in _EXPECT:
        sd = CS.state_dict(c)
        x, noise, sn = CS.inputs(c)
        rws = torch.zeros(c['B'], c['Kc']) if kind == 'none' else rows(c, kind)
        outs, recs, margin = [], [], float('inf')
        for b in range(c['B']):
            rec = []
            sd_b = biased_state_dict(c, sd, rws[b], dtype)
            outs.append(oracle_image(c, sd_b, x, noise, sn, b, dtype, rec))
            live = clamp(rws[b]) > -CLAMP
            if not bool(live.any()):
                live = torch.ones_like(live)
            margin = min([margin] + [_top2_margin(s, live) for s in rec])
            recs.append(torch.stack([s.argmax(1).to(torch.uint8) for s in rec], 0))          # (K, r, h, w)
        _EXPECT[key] = dict(out=torch.cat(outs, 0), record=torch.stack(recs, 1), margin=margin)
    return _EXPECT[key]


def final_decisions(c, kind, dtype=torch.float32, seed_of=None):
    """(B, h, w) argmax of the expectation's output"""
    return expected(c, kind, dtype, seed_of)['out'].argmax(1)


_ROWS = {}


def excluded(c):
    """per image the list of excluded classes of the 'excl' row"""
    c = seeded(c, 'excl')
    base = final_decisions(c, 'none')
    out = []
    for b in range(c['B']):
        counts = torch.bincount(base[b].reshape(-1), minlength=c['Kc'])
        order = torch.argsort(counts, descending=True, stable=True)
        need = WITNESS_PIXELS * base[b].numel()
        picked, held = [], 0
        for k in order.tolist():
            if held >= need or (len(picked) + 1 >= c['Kc'] and c['Kc'] > 1):
                break
            picked.append(k)
            held += int(counts[k])
        out.append(sorted(picked))
    return out


def rows(c, kind):
    """(B, Kc) float32 rows of the case (seeded; the same tensor on every call)"""
    c = seeded(c, kind)
    key = (c['name'], kind)
    if key in _ROWS:
        return _ROWS[key]
    B, K = c['B'], c['Kc']
    if kind == 'excl':
        r = torch.zeros(B, K)
        for b, ks in enumerate(excluded(c)):
            r[b, ks] = float('-inf')
    else:
        r = torch.zeros(B, K)
        n = max(1, K // 3)
        for b in range(B):
            g = torch.Generator().manual_seed(c['seed'] * 16 + b + 5)
            idx = torch.randperm(K, generator=g)[:n]
            sign = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(3.0), torch.tensor(-3.0))
            if K > 1:
                sign[0] = 3.0
            r[b, idx] = sign
        if kind == 'odd':
            for b in range(B):
                r[b, 0] = float('nan')
                if K > 2:
                    r[b, (b + 1) % (K - 1) + 1] = float('inf')
                    r[b, (b + 2) % (K - 1) + 1] = float('-inf')
    _ROWS[key] = r
    return r


def routes(c):
    """(id, gemm, flags): both engines and every flag that selects another route for the case"""
    v = [('bf16x3', 'bf16x3', {}), ('f32', 'f32', {}), ('unfused-layer', 'bf16x3', dict(fused_layer=False)),
         ('unfused-prologue', 'bf16x3', dict(fused_prologue=False))]
    if c['sampler'] == 'ddim':
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
        if c['r'] == 1:
            v.append(('sb-head', 'bf16x3', dict(nchw_head=False)))
    else:
        v += [('chain', 'bf16x3', dict(ddpm_chain=True)), ('chain-unfused-tail', 'bf16x3', dict(ddpm_chain=True, fused_tail=False)),
              ('chain-sb-head', 'bf16x3', dict(ddpm_chain=True, nchw_head=False))]
    return v


def rel_live(got, want, rows):
    """max-rel over the classes the rows leave in (an excluded class's score is -1e30 on both sides: it would be the whole scale)"""
    live = clamp(rows) > -CLAMP                                            # (B, Kc)
    if not bool(live.any()):
        live = torch.ones_like(live)
    m = live[:, :, None, None].expand_as(want)
    d = (got.double() - want.double()).abs()[m].max()
    return float(d / want.double()[m].abs().max())


def prior_bytes(c):
    """(table_bytes, bias_bytes) of include/ddp_mi355x.h as formulas of the case"""
    return c['B'] * 256 * 4, 2 * c['B'] * 256 * 4


# flag-clear sampler calls whose output bits are recorded from the parent's build (tests/golden/class_prior/parent_bits.json, written by
# tests/golden/gen_class_prior_parent.py): (case, gemm, engine keywords)
PARENT_BITS = {'kc19_7x13_b3/bf16x3': ('kc19_7x13_b3', 'bf16x3', {}),
               'kc150_9x14_noacc/f32': ('kc150_9x14_noacc', 'f32', {}),
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
