"""DDP_FLAG_CLASS_PRIOR on the GPU, per route x engine.  Needs an MI355X: ``pytest -m gpu``.  (CPU companion:
tests/test_class_prior_host.py; cases, rows and expectation: tests/class_prior_cases.py.)

  1  a zero table gives the bits of the flag-clear engine - output and x0 trace - on every route x engine
  2  with soft rows and with exclusion rows, on every route x engine: the output is within REL of the expectation (the oracle's sampler
     per image on a state dict whose conv_seg.bias is fl32(bias + clamp(prior[b]))), the step record holds the expectation's decisions
     at every step (no pixel excused: the CPU companion asserts a top-2 margin of 5 REL), and the batched call gives the bits of
     single-image calls of the same flagged engine with that image's row (a wrong image index, a straddling tile)
     exclusion: no recorded decision names an excluded class, its accumulated probability is exactly 0, the returned scores are
     finite and ddp_seg_postprocess on them yields no excluded label
  3  NaN, +inf and -inf entries give the bits of 0, 1e30 and -1e30; entries k >= num_classes are ignored
  4  DDP_FLAG_FORCE_X0: the forced decision is fed back, the scores carry the prior; DDP_FLAG_RECORD_X0 holds the same decisions
  5  graph: captured once, replayed with a new table == a fresh call
  6  DDP_FLAG_X0_HINTS + DDP_FLAG_PRIOR_START + DDP_FLAG_STEP_RECORD + DDP_FLAG_SEEDED_NOISE + the flag in one engine
  7  engine surface; 8 the call-time ``class_prior=`` of the seg plugin: simple_test / forward, aug_test and slide inference give what
     the same call gives on a model whose conv_seg.bias was edited
  9  flag-clear bits equal to the parent commit's on three sampler cases (tests/golden/class_prior/parent_bits.json)

Every engine samples through a workspace that is filled with a NaN pattern and has 4 KiB guards at both ends.  Every flagged test fails
on the parent commit: the C ABI refuses the cfg with "unknown flags 0x20000", the plugin raises an unexpected-keyword TypeError."""
import json
import os

import numpy as np
import pytest
import torch

import class_prior_cases as P
import config_space_cases as S
import support
from ddp_amd import _lib
from support import REL, dev, guards_ok as _guards_ok  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {(n, vid): (gemm, fl) for n, c in P.CASES.items() for vid, gemm, fl in P.routes(c)}
_state = support.state_cache(S.state_dict, S.inputs)


def _engine(c, dev, gemm='bf16x3', batch=None, sd=None, **kw):
    """DDPEngine of the (seeded) case on a guarded, NaN-patterned workspace.  The table of a class_prior engine holds the PATTERN
    afterwards (a NaN: it reads as 0); the caller sets or clears it, as the library's contract says."""
    return support.engine(sd if sd is not None else _state(c, dev)[0], 'seg', S.engine_kwargs(c), dev, gemm, batch, **kw)


def _sample(eng, c, dev, rows=None, sl=None, seed=None):
    """one call; ``rows``: (B, Kc) for a class_prior engine (None: the table as it is); ``sl``: the image slice of a single-image
    engine; ``seed``: a seeded engine's"""
    _, (x, nz, sn) = _state(c, dev)
    if sl is not None:
        x, nz, sn = x[sl].clone(), nz[sl].clone(), None if sn is None else sn[:, sl].clone()     # (fresh, aligned allocations)
    if rows is not None:
        eng.set_class_prior(rows.to(dev))
    if seed is not None:
        out = eng.sample(x.contiguous(), seed=seed)
    else:
        out = eng.sample(x.contiguous(), nz.contiguous(), None if sn is None else sn.contiguous())
    torch.cuda.synchronize()
    assert _guards_ok(eng), f'{c["name"]}: workspace guards overwritten'
    return out.cpu()


def test_bars():
    assert P.REL == REL == 2e-4 and P.MARGIN == 5 * REL


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', sorted(ROUTES))
def test_zero_table_gives_the_flag_clear_bits(dev, name, vid):
    c = P.seeded(P.CASES[name], 'soft')
    gemm, fl = ROUTES[(name, vid)]
    eng = _engine(c, dev, gemm, class_prior=True, record_x0=True, **fl)
    clear = _engine(c, dev, gemm, record_x0=True, **fl)
    assert clear.cfg.flags | _lib.FLAG_CLASS_PRIOR == eng.cfg.flags
    want = _sample(clear, c, dev)
    as_allocated = _sample(eng, c, dev)                                    # the NaN pattern: every entry reads as 0
    eng.clear_class_prior()
    got = _sample(eng, c, dev)
    assert bool((eng.class_prior_view() == 0).all())
    assert torch.equal(got, want) and torch.equal(as_allocated, want), (name, vid)
    assert torch.equal(eng.x0_trace().cpu(), clear.x0_trace().cpu())


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', P.KINDS)
@pytest.mark.parametrize('name,vid', sorted(ROUTES))
def test_output_and_decisions_match_the_expectation(dev, name, vid, kind):
    c = P.seeded(P.CASES[name], kind)
    gemm, fl = ROUTES[(name, vid)]
    rows = P.rows(c, kind)
    e = P.expected(c, kind)
    eng = _engine(c, dev, gemm, class_prior=True, record_steps=True, **fl)
    got = _sample(eng, c, dev, rows)
    rec = eng.step_record().cpu()                                          # (K, B, r, h, w)
    err = P.rel_live(got, e['out'], rows)
    agree = float((rec == e['record']).float().mean())
    print(f'CLASS-PRIOR {name}[{vid}]/{kind}: max-rel {err:.2e} (bar {REL:.0e}), decisions equal {agree:.4f}')
    assert torch.isfinite(got).all()
    assert err < REL
    assert torch.equal(rec, e['record'])                                   # at every step, no pixel excused
    # the batched call == single-image calls of the same flagged engine with that image's row
    one = _engine(c, dev, gemm, batch=1, class_prior=True, record_steps=True, **fl)
    for b in range(c['B']):
        single = _sample(one, c, dev, rows[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(single, got[b:b + 1]), (name, vid, kind, b)
        assert torch.equal(one.step_record().cpu(), rec[:, b:b + 1])
    if kind == 'excl':
        from ddp_amd.engine import seg_postprocess
        ex = P.excluded(c)
        lab = seg_postprocess(got.to(dev), (3 * c['h'] + 1, 2 * c['w'] + 3)).cpu()
        for b in range(c['B']):
            for k in ex[b] if c['Kc'] > 1 else []:                          # (one class: the uniform shift, class 0 stays)
                assert int((rec[:, b] == k).sum()) == 0 and int((lab[b] == k).sum()) == 0
            if c['accumulation'] and c['Kc'] > 1:
                assert bool((got[b, ex[b]] == 0).all())                    # the softmax term is exactly 0 at every step
            elif not c['accumulation']:
                assert float(got[b, ex[b]].max()) <= -9e29


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vid', ['bf16x3', 'f32', 'unfused-layer', 'unfused-tail'])
@pytest.mark.parametrize('name', ['kc19_7x13_b3', 'kc150_9x14_noacc', 'kc255_5x10_r2'])
def test_nan_and_inf_entries_read_as_zero_and_the_clamp(dev, name, vid):
    c = P.seeded(P.CASES[name], 'odd')
    gemm, fl = ROUTES[(name, vid)]
    odd = P.rows(c, 'odd')
    assert bool(torch.isnan(odd).any()) and bool((odd == float('inf')).any()) and bool((odd == float('-inf')).any())
    eng = _engine(c, dev, gemm, class_prior=True, **fl)
    got = _sample(eng, c, dev, odd)
    # the ignored entries k >= num_classes hold the workspace's NaN pattern here; now +inf
    eng.class_prior_view()[:, c['Kc']:] = float('inf')
    again = _sample(eng, c, dev)
    want = _sample(eng, c, dev, P.clamp(odd))
    assert torch.isfinite(got).all() and torch.equal(got, want) and torch.equal(again, want)
    e = P.expected(c, 'odd')
    assert torch.equal(got.argmax(1), e['out'].argmax(1))                  # a +1e30 class wins everywhere


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vid', ['bf16x3', 'f32', 'unfused-tail'])
def test_forced_decisions_are_fed_back_and_the_scores_carry_the_prior(dev, vid):
    name = 'kc19_7x13_b3'
    c = P.seeded(P.CASES[name], 'soft')
    K, B, r, h, w = c['K'], c['B'], c['r'], c['h'], c['w']
    gemm, fl = ROUTES[(name, vid)]
    rows, e = P.rows(c, 'soft'), P.expected(c, 'soft')
    forced = _engine(c, dev, gemm, class_prior=True, force_x0=True, **fl)
    forced.set_x0_decisions(e['record'].reshape(K, B * r, h, w).to(dev))
    got = _sample(forced, c, dev, rows)
    assert P.rel_live(got, e['out'], rows) < REL
    assert torch.equal(forced.x0_trace().cpu().view(K, B, r, h, w), e['record'])        # its own argmax, under the prior
    # other decisions fed back: the first step's scores are the same, the later ones move
    other = (e['record'].long() + 1) % c['Kc']
    forced.set_x0_decisions(other.reshape(K, B * r, h, w).to(dev))
    got2 = _sample(forced, c, dev, rows)
    assert not torch.equal(got2, got)
    assert torch.equal(forced.x0_trace().cpu()[0], e['record'].reshape(K, B * r, h, w)[0])
    rec = _engine(c, dev, gemm, class_prior=True, record_x0=True, **fl)
    _sample(rec, c, dev, rows)
    assert torch.equal(rec.x0_trace().cpu().view(K, B, r, h, w), e['record'])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['kc19_7x13_b3', 'kc255_5x10_r2', 'ddpm_7x13'])
def test_graph_replays_pick_up_a_new_table(dev, name):
    c = P.seeded(P.CASES[name], 'soft')
    _, (x, noise, sn) = _state(c, dev)
    tabs = [P.rows(c, 'soft'), P.rows(c, 'odd'), torch.zeros(c['B'], c['Kc'])]
    eng = _engine(c, dev, class_prior=True)
    want = [_sample(eng, c, dev, t) for t in tabs]
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[0], want[2])
    eng.clear_class_prior()
    g = eng.capture(x, noise, sn)
    for i in (0, 1, 0, 2):
        out = g.replay(class_prior=tabs[i].to(dev))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[i]), (name, i)
    assert torch.equal(g.replay().cpu(), want[2])                          # no table given: what the buffer holds
    assert _guards_ok(eng)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_hints_prior_start_step_record_and_class_prior_in_one_engine(dev):
    """all four conditioning flags (and seeded noise): a zero table gives the bits of the same engine without the flag, the batched call
    the bits of the single-image calls, and the class prior shows in the record on top of hints and start map"""
    import prior_start_cases as PS
    import x0_hint_cases as H
    c = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    rows = P.rows(c, 'soft')
    hints = H.partial_hints(c)
    g = torch.Generator().manual_seed(31)
    prior = torch.randint(0, c['Kc'] + 1, (c['B'], c['h'], c['w']), generator=g).to(torch.uint8)
    common = dict(x0_hints=True, prior_start=True, t_start=0.6, record_steps=True, seeded_noise=True)

    def run(eng, tab, sl=None):
        s = slice(None) if sl is None else sl
        eng.set_hints(hints[s].to(dev))
        eng.set_prior(prior[s].to(dev))
        if tab is not None:
            eng.set_class_prior(tab.to(dev))
        x = _state(c, dev)[1][0][s].contiguous()
        out = eng.sample(x, seed=77, image_base=0 if sl is None else sl.start)
        torch.cuda.synchronize()
        assert _guards_ok(eng)
        return out.cpu(), eng.step_record().cpu()
    full = _engine(c, dev, class_prior=True, **common)
    without = _engine(c, dev, **common)
    assert full.cfg.flags == (without.cfg.flags | _lib.FLAG_CLASS_PRIOR)
    o0, r0 = run(full, torch.zeros_like(rows))
    ow, rw = run(without, None)
    assert torch.equal(o0, ow) and torch.equal(r0, rw)
    o1, r1 = run(full, rows)
    assert float((r1 != r0).float().mean()) > P.WITNESS_PIXELS              # the record holds the decisions under the prior
    one = _engine(c, dev, batch=1, class_prior=True, **common)
    for b in range(c['B']):
        ob, rb = run(one, rows[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(ob, o1[b:b + 1]) and torch.equal(rb, r1[:, b:b + 1]), b
    assert PS.REL == REL


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_engine_class_prior_methods(dev):
    from ddp_amd.engine import DDPEngine, class_mask_to_prior, class_prior_places
    c = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    sd, _ = _state(c, dev)
    eng = DDPEngine(sd, 'seg', device=dev, class_prior=True, record_steps=True, **S.engine_kwargs(c))
    v = eng.class_prior_view()
    assert v.dtype == torch.float32 and tuple(v.shape) == (c['B'], 256) and bool((v == 0).all())                 # allocated: cleared
    tb, bb = P.prior_bytes(c)
    rec, smap = (c['K'] * c['B'] * c['r'] * c['h'] * c['w'], c['B'] * c['h'] * c['w'] * 4)
    off = v.data_ptr() - eng.workspace.data_ptr()
    assert off == eng.workspace.numel() * 4 - P.round256(rec) - P.round256(smap) - P.round256(tb)               # the header's formula
    assert class_prior_places(eng.cfg, eng.workspace.numel() * 4) == (off, tb, off - P.round256(bb), bb)
    rows = P.rows(c, 'soft')
    eng.set_class_prior(rows.to(dev))
    assert torch.equal(eng.class_prior_view()[:, :c['Kc']].cpu(), rows) and bool((eng.class_prior_view()[:, c['Kc']:] == 0).all())
    eng.set_class_prior(rows.double().to(dev))                                                                  # any float dtype
    for bad in (rows, rows.to(dev)[:1], rows.to(dev)[:, :5], rows.to(dev).long(), torch.zeros(c['B'], 256, device=dev)):
        with pytest.raises(_lib.DdpError, match='class'):
            eng.set_class_prior(bad)
    mask = torch.ones(c['B'], c['Kc'], dtype=torch.bool, device=dev)
    mask[:, 3] = False
    eng.set_class_prior(class_mask_to_prior(mask))
    assert bool(torch.isinf(eng.class_prior_view()[:, 3]).all())
    eng.set_geometry(batch=c['B'], h=c['h'] + 1, w=c['w'])                                                      # every set_geometry: cleared
    assert bool((eng.class_prior_view() == 0).all())
    eng.set_class_prior(rows.to(dev))
    eng.set_geometry(batch=c['B'] + 1, h=4 * c['h'], w=4 * c['w'])                                              # regrown workspace
    assert tuple(eng.class_prior_view().shape) == (c['B'] + 1, 256) and bool((eng.class_prior_view() == 0).all())
    plain = DDPEngine(sd, 'seg', device=dev, **S.engine_kwargs(c))
    for m in (plain.class_prior_view, plain.clear_class_prior):
        with pytest.raises(_lib.DdpError, match='class_prior'):
            m()
    import prior_start_cases as PS
    d = PS.CASES['depth_9x14']
    with pytest.raises(ValueError, match='class_prior'):
        DDPEngine(PS.state_dict(d), 'depth', device=dev, class_prior=True, **S.engine_kwargs(d))
    # ddp_head_forward ignores the flag
    feat = torch.randn(c['B'] * c['r'], 256, c['h'], c['w'], generator=torch.Generator().manual_seed(3)).to(dev)
    heng = _engine(c, dev, class_prior=True)
    heng.set_class_prior(rows.to(dev))
    assert torch.equal(heng.head_forward(feat, None).cpu(), _engine(c, dev).head_forward(feat, None).cpu()) and _guards_ok(heng)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def _plugin(c, dev, sd):
    model = support.seg_plugin(c, dev, sd, pool_backbone=True, noise_seed=5)
    # ddpm: on the fused step boundary, where - as on the ddim product route - the prior row is the accumulator start of conv_seg and
    # the edited bias gives the same bits (the GEMM routes add the row behind the GEMM: equal to rounding, test 2 bounds them)
    model.ddpm_chain = c['sampler'] == 'ddpm'
    return model


@pytest.mark.parametrize('name,kind', [('kc19_8x12_b2', 'soft'), ('kc19_8x12_b2', 'excl'), ('ddpm_7x13', 'soft')])
def test_plugin_class_prior_is_the_edited_bias(dev, name, kind):
    """b = 1: simple_test / forward, aug_test (two augmentations, one flipped) and slide inference with ``class_prior=`` give what the same
    call gives on a model whose conv_seg.bias is fl32(bias + clamp(row)) - seeded noise (noise_seed), so both models draw the same"""
    c = dict(P.seeded(P.CASES[name], kind), B=1)
    sd = S.state_dict(c)
    row = P.rows(P.CASES[name], kind)[:1]
    edited = dict(sd)
    edited['decode_head.conv_seg.bias'] = sd['decode_head.conv_seg.bias'] + P.clamp(row[0])
    model, ref = _plugin(c, dev, sd), _plugin(c, dev, edited)
    g = torch.Generator().manual_seed(23)
    H, W = 4 * c['h'], 4 * c['w']
    img = torch.randn(1, 3, H, W, generator=g).to(dev)
    meta = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False)]
    fmeta = [dict(meta[0], flip=True, flip_direction='horizontal')]
    cp = row.to(dev)
    x = model.extract_feat(img)[0]
    sample = model.ddim_sample if c['sampler'] == 'ddim' else model.ddpm_sample
    rsample = ref.ddim_sample if c['sampler'] == 'ddim' else ref.ddpm_sample
    scores = sample(x, None, class_prior=cp).cpu()
    assert torch.equal(scores, rsample(x, None).cpu())
    assert not torch.equal(scores, sample(x, None).cpu())                   # ... and class_prior is part of the engine key
    assert len(model._engine_cache) == 2
    calls = {
        'simple_test': lambda m, kw: m.simple_test(img, meta, rescale=True, **kw),
        'forward': lambda m, kw: m(img=[img], img_metas=[meta], return_loss=False, rescale=True, **kw),
        'aug_test': lambda m, kw: m.aug_test([img, img.flip(3)], [meta, fmeta], rescale=True, **kw),
        'forward-aug': lambda m, kw: m(img=[img, img.flip(3)], img_metas=[meta, fmeta], return_loss=False, **kw),
    }
    for what, call in calls.items():
        got, want, plain = np.stack(call(model, dict(class_prior=cp))), np.stack(call(ref, {})), np.stack(call(model, {}))
        assert got.shape == (1, H, W) and (got == want).all(), what
        assert (got != plain).mean() > 0.05, what
    if kind == 'excl':
        ex = P.excluded(P.CASES[name])[0]
        assert not np.isin(np.stack(calls['simple_test'](model, dict(class_prior=cp))), ex).any()
    # slide mode: every window of the image samples with the image's row.  (ddp_seg_slide_postprocess takes the windows' scores as
    # 16-byte aligned slices of one tensor: K h w must be a multiple of 4 - the 8 x 12 map, not the 7 x 13 one)
    if (c['Kc'] * c['h'] * c['w']) % 4:
        assert name == 'ddpm_7x13'
        return
    for m in (model, ref):
        m.test_cfg = dict(mode='slide', crop_size=(3 * c['h'], 3 * c['w']), stride=(c['h'], c['w']))
    got, want = np.stack(model.simple_test(img, meta, rescale=True, class_prior=cp)), np.stack(ref.simple_test(img, meta, rescale=True))
    assert (got == want).all() and (got != np.stack(model.simple_test(img, meta, rescale=True))).mean() > 0.05
    s_got, s_want = model.slide_inference(img, meta, True, class_prior=cp), ref.slide_inference(img, meta, True)
    assert torch.equal(s_got.cpu(), s_want.cpu())
    p_got, p_want = model.inference(img, meta, True, class_prior=cp), ref.inference(img, meta, True)
    assert torch.equal(p_got.cpu(), p_want.cpu())
    with pytest.raises(ValueError, match='class_prior'):
        model.simple_test(img, meta, class_prior=cp[:, :5])


def test_plugin_self_aligned_predict_and_fcn_head(dev):
    import ddp_amd
    from support import ENCODER, seg_cfg
    name = 'kc19_7x13_b3'
    c = P.seeded(P.CASES[name], 'soft')
    sd, (x, noise, _) = _state(c, dev)
    rows = P.rows(c, 'soft')
    head = dict(seg_cfg()['decode_head'], num_classes=c['Kc'], encoder=dict(ENCODER, num_layers=c['L']))
    model = ddp_amd.build_segmentor(seg_cfg(type='SelfAlignedDDP', timesteps=c['K'], bit_scale=c['bit_scale'], decode_head=head))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    nz = noise[:, 0].contiguous()
    preds, logits = model.self_aligned_predict(x, noise=nz, return_logits=True, class_prior=rows.to(dev))
    _, plain = model.self_aligned_predict(x, noise=nz, return_logits=True)
    # one pass, no feedback: the scores are the plain ones plus the row, to rounding; the projected classes follow them
    want = plain.cpu() + rows[:, :, None, None]
    assert P.max_rel(logits.cpu(), want) < 1e-6 and not torch.equal(logits.argmax(1), plain.argmax(1))
    emb = sd['embedding_table.weight']
    x0 = (torch.sigmoid(emb[logits.argmax(1).cpu()]) * 2 - 1) * c['bit_scale']
    assert P.max_rel(preds.cpu(), x0.permute(0, 3, 1, 2)) < 1e-5


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_flag_clear_bits_are_the_parents(dev):
    """tests/golden/class_prior/parent_bits.json: sha256 of three flag-clear sampler outputs, recorded from the parent commit's build by
    tests/golden/gen_class_prior_parent.py"""
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'class_prior', 'parent_bits.json')))
    assert sorted(want) == sorted(P.PARENT_BITS) and len(want) == 3
    assert P.flag_clear_hashes(dev) == want
