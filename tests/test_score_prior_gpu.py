"""DDP_FLAG_SCORE_PRIOR on the GPU, per route x engine.  Needs an MI355X: ``pytest -m gpu``.  (CPU companion:
tests/test_score_prior_host.py; cases, maps and expectation: tests/score_prior_cases.py.)

  1  the rows kernel alone: after a call the library's rows buffer is the normalised transpose of the map, bit for bit, on every shape
     and every map kind ('odd' included), the padding columns are zero, the caller's map is untouched and so are the guards
  2  a zero map gives the bits of the flag-clear engine - output and x0 trace - on every route x engine
  3  a map constant over the pixels of each image gives the bits of DDP_FLAG_CLASS_PRIOR with that row, on every route x engine
  4  soft and exclusion maps, on every route x engine (ddpm and the ddpm chain included): the output is within REL of the expectation
     (the oracle's sampler per image, its head returning scores + clamp(prior[b])), the step record holds the expectation's decisions
     at every step (no pixel excused: the CPU companion asserts a top-2 margin of 5 REL), and the batched call gives the bits of
     single-image calls with that image's map.  exclusion: the excluded class is never decided at its pixel, its accumulated
     probability there is exactly 0, the returned scores are finite.  r = 2: both replicas take the expectation's decisions, which
     see one row
  5  NaN, +inf and -inf entries give the bits of 0, 1e30 and -1e30
  6  with DDP_FLAG_CLASS_PRIOR both priors add; with DDP_FLAG_FORCE_X0 the forced decision is fed back and the scores carry the prior;
     hints, prior start, step record, seeded noise and class prior with the flag in one engine
  7  graph: captured once, replayed with a new map == a fresh call
  8  engine surface; the call-time ``score_prior=`` of the seg plugin: simple_test / forward == the engine fed the resized map; refusals
  9  flag-clear bits equal to the parent commit's on four sampler cases (tests/golden/score_prior/parent_bits.json)

Every engine samples through a workspace that is filled with a NaN pattern, is exactly as long as ddp_query_workspace says and has 4 KiB
guards at both ends.  Every flagged test fails on the parent commit: the C ABI refuses the cfg with "unknown flags 0x100000"."""
import json
import os

import numpy as np
import pytest
import torch

import config_space_cases as S
import score_prior_cases as P
import support
from ddp_amd import _lib
from support import REL, dev, guards_ok as _guards_ok  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = {(n, vid): (gemm, fl) for n, c in P.CASES.items() for vid, gemm, fl in P.routes(c)}
_state = support.state_cache(S.state_dict, S.inputs)


def _engine(c, dev, gemm='bf16x3', batch=None, **kw):
    """DDPEngine of the (seeded) case on a guarded, NaN-patterned workspace of exactly the queried size.  The map of a score_prior engine
    holds the PATTERN afterwards (a NaN: it reads as 0); the caller sets or clears it, as the library's contract says."""
    return support.engine(_state(c, dev)[0], 'seg', S.engine_kwargs(c), dev, gemm, batch, exact=True, **kw)


def _sample(eng, c, dev, pm=None, sl=None, seed=None):
    """one call; ``pm``: (B, Kc, h, w) for a score_prior engine (None: the map as it is); ``sl``: the image slice of a single-image
    engine; ``seed``: a seeded engine's"""
    _, (x, nz, sn) = _state(c, dev)
    if sl is not None:
        x, nz, sn = x[sl].clone(), nz[sl].clone(), None if sn is None else sn[:, sl].clone()     # (fresh, aligned allocations)
    if pm is not None:
        eng.set_score_prior(pm.to(dev))
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
@pytest.mark.parametrize('name', list(P.CASES))
def test_rows_buffer_is_the_normalised_transpose(dev, name):
    c = P.seeded(P.CASES[name], 'soft')
    n = c['B'] * c['h'] * c['w']
    eng = _engine(c, dev, score_prior=True)
    for kind in ('odd', 'soft', 'excl', 'const', 'zero'):
        pm = P.prior_map(P.CASES[name], kind)
        _sample(eng, c, dev, pm)
        rows = eng._region('sprior_rows', torch.float32, (n, P.kp(c))).cpu()
        want = P.rows_of(pm, c)
        assert rows.numpy().tobytes() == want.numpy().tobytes(), (name, kind)             # bit for bit, -0.0 and the clamp included
        assert not bool(rows[:, c['Kc']:].any())                                           # the padding columns
        assert eng.score_prior_view().cpu().numpy().tobytes() == pm.numpy().tobytes()      # the library does not write the caller's map
    from ddp_amd.engine import score_prior_places
    mo, mb, ro, rb = score_prior_places(eng.cfg, eng.workspace.numel() * 4)
    assert (mb, rb) == P.prior_bytes(c) and ro + P.round256(rb) == mo and mo + P.round256(mb) == eng.workspace.numel() * 4


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', list(ROUTES))
def test_zero_map_gives_the_flag_clear_bits(dev, name, vid):
    c = P.seeded(P.CASES[name], 'zero')
    gemm, fl = ROUTES[(name, vid)]
    eng = _engine(c, dev, gemm, score_prior=True, record_x0=True, **fl)
    clear = _engine(c, dev, gemm, record_x0=True, **fl)
    assert clear.cfg.flags | _lib.FLAG_SCORE_PRIOR == eng.cfg.flags
    want = _sample(clear, c, dev)
    as_allocated = _sample(eng, c, dev)                                    # the NaN pattern: every entry reads as 0
    eng.clear_score_prior()
    got = _sample(eng, c, dev)
    assert bool((eng.score_prior_view() == 0).all())
    assert torch.equal(got, want) and torch.equal(as_allocated, want), (name, vid)
    assert torch.equal(eng.x0_trace().cpu(), clear.x0_trace().cpu())


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', list(ROUTES))
def test_constant_map_gives_the_class_prior_bits(dev, name, vid):
    c = P.seeded(P.CASES[name], 'const')
    gemm, fl = ROUTES[(name, vid)]
    eng = _engine(c, dev, gemm, score_prior=True, record_steps=True, **fl)
    cp = _engine(c, dev, gemm, class_prior=True, record_steps=True, **fl)
    cp.set_class_prior(P.const_rows(c).to(dev))
    want = _sample(cp, c, dev)
    got = _sample(eng, c, dev, P.prior_map(c, 'const'))
    assert torch.equal(got, want), (name, vid)
    assert torch.equal(eng.step_record().cpu(), cp.step_record().cpu())


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', P.SEEDED_KINDS)
@pytest.mark.parametrize('name,vid', list(ROUTES))
def test_output_and_decisions_match_the_expectation(dev, name, vid, kind):
    c = P.seeded(P.CASES[name], kind)
    gemm, fl = ROUTES[(name, vid)]
    pm = P.prior_map(c, kind)
    e = P.expected(c, kind)
    eng = _engine(c, dev, gemm, score_prior=True, record_steps=True, **fl)
    got = _sample(eng, c, dev, pm)
    rec = eng.step_record().cpu()                                          # (K, B, r, h, w)
    err = P.rel_live(got, e['out'], pm)
    agree = float((rec == e['record']).float().mean())
    print(f'SCORE-PRIOR {name}[{vid}]/{kind}: max-rel {err:.2e} (bar {REL:.0e}), decisions equal {agree:.4f}')
    assert torch.isfinite(got).all()
    assert err < REL
    assert torch.equal(rec, e['record'])                                   # at every step, no pixel excused; r = 2: both replicas
    # the batched call == single-image calls of the same flagged engine with that image's map
    one = _engine(c, dev, gemm, batch=1, score_prior=True, record_steps=True, **fl)
    for b in range(c['B']):
        single = _sample(one, c, dev, pm[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(single, got[b:b + 1]), (name, vid, kind, b)
        assert torch.equal(one.step_record().cpu(), rec[:, b:b + 1])
    if kind == 'excl' and c['witness']:
        base = P.expected(c, 'none', seed_of='excl')['out'].argmax(1)      # (B, h, w): the class excluded at each pixel
        assert bool((rec.long() != base[None, :, None].long()).all())      # never decided there, at any step, by any replica
        at = got.gather(1, base[:, None])
        if c['accumulation']:
            assert bool((at == 0).all())                                   # the softmax term is exactly 0 at every step
        else:
            assert float(at.max()) <= -9e29 and bool(torch.isfinite(at).all())
        assert bool((got.argmax(1) != base).all())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vid', ['bf16x3', 'f32', 'unfused-layer', 'unfused-tail'])
@pytest.mark.parametrize('name', ['kc19_7x13_b3', 'kc150_9x14_noacc', 'kc255_5x10_r2'])
def test_nan_and_inf_entries_read_as_zero_and_the_clamp(dev, name, vid):
    c = P.seeded(P.CASES[name], 'odd')
    gemm, fl = ROUTES[(name, vid)]
    odd = P.prior_map(c, 'odd')
    eng = _engine(c, dev, gemm, score_prior=True, **fl)
    got = _sample(eng, c, dev, odd)
    want = _sample(eng, c, dev, P.clamp(odd))
    assert torch.isfinite(got).all() and torch.equal(got, want)
    e = P.expected(c, 'odd')
    hit = (odd == float('inf')).any(1)                                     # a +1e30 class wins its pixel
    assert torch.equal(got.argmax(1)[hit], e['out'].argmax(1)[hit]) and bool(hit.any())


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', [(n, v) for n in P.BOTH for v in ('bf16x3', 'f32', 'unfused-layer', 'unfused-tail', 'chain') if (n, v) in ROUTES])
def test_both_priors_add(dev, name, vid):
    """DDP_FLAG_CLASS_PRIOR + DDP_FLAG_SCORE_PRIOR against the expectation with both added in the oracle's head, on the 'both' seed (whose
    margin the CPU companion asserts): output within REL, the same decisions at every step"""
    c = P.seeded(P.CASES[name], 'both')
    gemm, fl = ROUTES[(name, vid)]
    pm, cr = P.prior_map(c, 'soft'), P.const_rows(c)
    e = P.expected(c, 'both')
    eng = _engine(c, dev, gemm, score_prior=True, class_prior=True, record_steps=True, **fl)
    eng.set_class_prior(cr.to(dev))
    got = _sample(eng, c, dev, pm)
    err = P.max_rel(got, e['out'])
    print(f'SCORE-PRIOR {name}[{vid}] + class prior: max-rel {err:.2e} (bar {REL:.0e})')
    assert err < REL
    assert torch.equal(eng.step_record().cpu(), e['record'])
    alone = _sample(_engine(c, dev, gemm, score_prior=True, **fl), c, dev, pm)
    assert not torch.equal(alone, got)


@pytest.mark.parametrize('vid', ['bf16x3', 'f32', 'unfused-tail'])
def test_forced_decisions_are_fed_back_and_the_scores_carry_the_prior(dev, vid):
    name = 'kc19_7x13_b3'
    c = P.seeded(P.CASES[name], 'soft')
    K, B, r, h, w = c['K'], c['B'], c['r'], c['h'], c['w']
    gemm, fl = ROUTES[(name, vid)]
    pm, e = P.prior_map(c, 'soft'), P.expected(c, 'soft')
    forced = _engine(c, dev, gemm, score_prior=True, force_x0=True, **fl)
    forced.set_x0_decisions(e['record'].reshape(K, B * r, h, w).to(dev))
    got = _sample(forced, c, dev, pm)
    assert P.max_rel(got, e['out']) < REL
    assert torch.equal(forced.x0_trace().cpu().view(K, B, r, h, w), e['record'])        # its own argmax, under the prior
    # other decisions fed back: the first step's scores are the same, the later ones move
    other = (e['record'].long() + 1) % c['Kc']
    forced.set_x0_decisions(other.reshape(K, B * r, h, w).to(dev))
    got2 = _sample(forced, c, dev, pm)
    assert not torch.equal(got2, got)
    assert torch.equal(forced.x0_trace().cpu()[0], e['record'].reshape(K, B * r, h, w)[0])
    rec = _engine(c, dev, gemm, score_prior=True, record_x0=True, **fl)
    _sample(rec, c, dev, pm)
    assert torch.equal(rec.x0_trace().cpu().view(K, B, r, h, w), e['record'])


def test_every_conditioning_flag_in_one_engine(dev):
    """hints, prior start, step record, seeded noise, class prior and the score prior: a zero map gives the bits of the same engine
    without the flag, the batched call the bits of the single-image calls, and the score prior shows in the record"""
    import x0_hint_cases as H
    c = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    pm, cr = P.prior_map(c, 'soft'), P.const_rows(c)
    hints = H.partial_hints(c)
    g = torch.Generator().manual_seed(31)
    prior = torch.randint(0, c['Kc'] + 1, (c['B'], c['h'], c['w']), generator=g).to(torch.uint8)
    common = dict(x0_hints=True, prior_start=True, t_start=0.6, record_steps=True, seeded_noise=True, class_prior=True)

    def run(eng, m, sl=None):
        s = slice(None) if sl is None else sl
        eng.set_hints(hints[s].to(dev))
        eng.set_prior(prior[s].to(dev))
        eng.set_class_prior(cr[s].to(dev))
        if m is not None:
            eng.set_score_prior(m.to(dev))
        x = _state(c, dev)[1][0][s].contiguous()
        out = eng.sample(x, seed=77, image_base=0 if sl is None else sl.start)
        torch.cuda.synchronize()
        assert _guards_ok(eng)
        return out.cpu(), eng.step_record().cpu()
    full = _engine(c, dev, score_prior=True, **common)
    without = _engine(c, dev, **common)
    assert full.cfg.flags == (without.cfg.flags | _lib.FLAG_SCORE_PRIOR)
    o0, r0 = run(full, torch.zeros_like(pm))
    ow, rw = run(without, None)
    assert torch.equal(o0, ow) and torch.equal(r0, rw)
    o1, r1 = run(full, pm)
    assert float((r1 != r0).float().mean()) > 0.1                            # the record holds the decisions under the prior
    one = _engine(c, dev, batch=1, score_prior=True, **common)
    for b in range(c['B']):
        ob, rb = run(one, pm[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(ob, o1[b:b + 1]) and torch.equal(rb, r1[:, b:b + 1]), b


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['kc19_7x13_b3', 'kc255_5x10_r2', 'ddpm_7x13'])
def test_graph_replays_pick_up_a_new_map(dev, name):
    c = P.seeded(P.CASES[name], 'soft')
    _, (x, noise, sn) = _state(c, dev)
    maps = [P.prior_map(c, 'soft'), P.prior_map(c, 'odd'), P.prior_map(c, 'zero')]
    eng = _engine(c, dev, score_prior=True)
    want = [_sample(eng, c, dev, m) for m in maps]
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[0], want[2])
    eng.clear_score_prior()
    g = eng.capture(x, noise, sn)
    for i in (0, 1, 0, 2):
        out = g.replay(score_prior=maps[i].to(dev))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[i]), (name, i)
    assert torch.equal(g.replay().cpu(), want[2])                          # no map given: what the buffer holds
    assert _guards_ok(eng)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_engine_score_prior_methods(dev):
    from ddp_amd.engine import DDPEngine, score_prior_places
    c = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    sd, _ = _state(c, dev)
    eng = DDPEngine(sd, 'seg', device=dev, score_prior=True, class_prior=True, record_steps=True, **S.engine_kwargs(c))
    v = eng.score_prior_view()
    shape = (c['B'], c['Kc'], c['h'], c['w'])
    assert v.dtype == torch.float32 and tuple(v.shape) == shape and bool((v == 0).all())                         # allocated: cleared
    mb, rb = P.prior_bytes(c)
    rec, smap = (c['K'] * c['B'] * c['r'] * c['h'] * c['w'], c['B'] * c['h'] * c['w'] * 4)
    off = v.data_ptr() - eng.workspace.data_ptr()
    total = eng.workspace.numel() * 4
    assert off == total - P.round256(rec) - P.round256(smap) - 3 * P.round256(c['B'] * 1024) - P.round256(mb)   # the header's list
    assert score_prior_places(eng.cfg, total) == (off, mb, off - P.round256(rb), rb)
    pm = P.prior_map(c, 'soft')
    eng.set_score_prior(pm.to(dev))
    assert torch.equal(eng.score_prior_view().cpu(), pm)
    eng.set_score_prior(pm.double().to(dev))                                                                     # any float dtype
    for bad in (pm, pm.to(dev)[:1], pm.to(dev)[:, :5], pm.to(dev).long(), pm.to(dev)[:, :, :, :5]):
        with pytest.raises(_lib.DdpError, match='score_prior|engine lives'):
            eng.set_score_prior(bad)
    eng.set_geometry(batch=c['B'], h=c['h'] + 1, w=c['w'])                                                       # every set_geometry: cleared
    assert tuple(eng.score_prior_view().shape) == (c['B'], c['Kc'], c['h'] + 1, c['w']) and bool((eng.score_prior_view() == 0).all())
    eng.score_prior_view().fill_(1.0)
    eng.set_geometry(batch=c['B'] + 1, h=4 * c['h'], w=4 * c['w'])                                               # regrown workspace
    assert tuple(eng.score_prior_view().shape) == (c['B'] + 1, c['Kc'], 4 * c['h'], 4 * c['w']) and bool((eng.score_prior_view() == 0).all())
    plain = DDPEngine(sd, 'seg', device=dev, **S.engine_kwargs(c))
    for m in (plain.score_prior_view, plain.clear_score_prior):
        with pytest.raises(_lib.DdpError, match='score_prior'):
            m()
    import prior_start_cases as PS
    d = PS.CASES['depth_9x14']
    with pytest.raises(ValueError, match='score_prior'):
        DDPEngine(PS.state_dict(d), 'depth', device=dev, score_prior=True, **S.engine_kwargs(d))
    # ddp_head_forward ignores the flag
    feat = torch.randn(c['B'] * c['r'], 256, c['h'], c['w'], generator=torch.Generator().manual_seed(3)).to(dev)
    heng = _engine(c, dev, score_prior=True)
    heng.set_score_prior(pm.to(dev))
    assert torch.equal(heng.head_forward(feat, None).cpu(), _engine(c, dev).head_forward(feat, None).cpu()) and _guards_ok(heng)


@pytest.mark.parametrize('name', ['kc19_8x12_b2', 'ddpm_7x13'])
def test_plugin_score_prior_is_the_engine_fed_the_resized_map(dev, name):
    """simple_test / forward / whole_inference / encode_decode with ``score_prior=`` in the frame of the image == the engine (seeded with
    the plugin's key) fed F.interpolate(map, (h, w), bilinear, align_corners of the model), through the plugin's own epilogue; a map
    already at (h, w) goes in unchanged; aug_test and slide inference refuse"""
    import torch.nn.functional as F

    from ddp_amd.engine import DDPEngine, seg_postprocess
    c = P.seeded(P.CASES[name], 'soft')
    B, h, w = c['B'], c['h'], c['w']
    sd = S.state_dict(c)
    model = support.seg_plugin(c, dev, sd, pool_backbone=True, noise_seed=5)
    H, W = 4 * h, 4 * w
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(23)).to(dev)
    meta = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False)] * B
    big = (torch.randn(B, c['Kc'], H, W, generator=torch.Generator().manual_seed(24)) * 3).to(dev)
    x = model.extract_feat(img)[0]
    resized = F.interpolate(big, size=(h, w), mode='bilinear', align_corners=model.align_corners)
    eng = DDPEngine(sd, 'seg', device=dev, score_prior=True, seeded_noise=True, **S.engine_kwargs(c))
    eng.set_score_prior(resized.contiguous())
    want = eng.sample(x.contiguous().float(), seed=5, image_base=0, call=0)
    sample = model.ddim_sample if c['sampler'] == 'ddim' else model.ddpm_sample
    assert torch.equal(sample(x, None, score_prior=big).cpu(), want.cpu())
    assert torch.equal(sample(x, None, score_prior=resized).cpu(), want.cpu())               # at (h, w): unchanged
    assert not torch.equal(sample(x, None).cpu(), want.cpu())                                # ... and part of the engine key
    labels = np.stack(seg_postprocess(want, (H, W), (H, W), (H, W), model.align_corners, None).cpu().numpy().astype('int64'))
    for what, call in (('simple_test', lambda kw: model.simple_test(img, meta, rescale=True, **kw)),
                       ('forward', lambda kw: model(img=[img], img_metas=[meta], return_loss=False, rescale=True, **kw))):
        got, plain = np.stack(call(dict(score_prior=big))), np.stack(call({}))
        assert got.shape == (B, H, W) and (got == labels).all(), what
        assert (got != plain).mean() > 0.05, what
    up = F.interpolate(want, size=(H, W), mode='bilinear', align_corners=model.align_corners)
    assert torch.equal(model.encode_decode(img, meta, score_prior=big).cpu(), up.cpu())
    assert torch.equal(model.whole_inference(img, meta, False, score_prior=big).cpu(), up.cpu())
    for bad in (big[:, :5], big[:1], big[0], big.long()):
        with pytest.raises(ValueError, match='score_prior must be a float'):
            model.simple_test(img, meta, score_prior=bad)
    with pytest.raises(ValueError, match='score_prior is not built for aug_test'):
        model(img=[img, img.flip(3)], img_metas=[meta, meta], return_loss=False, score_prior=big)
    model.test_cfg = dict(mode='slide', crop_size=(3 * h, 3 * w), stride=(h, w))
    with pytest.raises(ValueError, match='score_prior is not built for slide inference'):
        model.simple_test(img, meta, score_prior=big)


def test_plugin_self_aligned_predict(dev):
    import ddp_amd
    from support import ENCODER, seg_cfg
    c = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    sd, (x, noise, _) = _state(c, dev)
    pm = P.prior_map(c, 'soft')
    head = dict(seg_cfg()['decode_head'], num_classes=c['Kc'], encoder=dict(ENCODER, num_layers=c['L']))
    model = ddp_amd.build_segmentor(seg_cfg(type='SelfAlignedDDP', timesteps=c['K'], bit_scale=c['bit_scale'], decode_head=head))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    nz = noise[:, 0].contiguous()
    preds, logits = model.self_aligned_predict(x, noise=nz, return_logits=True, score_prior=pm.to(dev))
    _, plain = model.self_aligned_predict(x, noise=nz, return_logits=True)
    # one pass, no feedback: the scores are the plain ones plus the map, to rounding; the projected classes follow them
    assert P.max_rel(logits.cpu(), plain.cpu() + pm) < 1e-6 and not torch.equal(logits.argmax(1), plain.argmax(1))
    emb = sd['embedding_table.weight']
    x0 = (torch.sigmoid(emb[logits.argmax(1).cpu()]) * 2 - 1) * c['bit_scale']
    assert P.max_rel(preds.cpu(), x0.permute(0, 3, 1, 2)) < 1e-5


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_flag_clear_bits_are_the_parents(dev):
    """tests/golden/score_prior/parent_bits.json: sha256 of four flag-clear sampler outputs, recorded from the parent commit's build by
    tests/golden/gen_score_prior_parent.py"""
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'score_prior', 'parent_bits.json')))
    assert sorted(want) == sorted(P.PARENT_BITS) and len(want) == 4
    assert P.flag_clear_hashes(dev) == want
