"""DDP_FLAG_PRIOR_START on the GPU, per route x engine.  Needs an MI355X: ``pytest -m gpu``.  (CPU companion:
tests/test_prior_start_host.py; cases, prior maps, start map and expectation loop: tests/prior_start_cases.py.)

  1  start map: last_start() against the fp64 evaluation of the header's formulas, elementwise within
     2^-21 (|alpha x0| + |sigma-term|) + 2^-21 bit_scale - two products and one sum each round once (2^-24 relative each), the table
     sigmoid is held by the device-math probe's own bar; 8 ulp leaves room
  2  same bits from every writer: a prior-and-seeded engine and a prior-only engine fed the seeded-only engine's last_noise()
  3  output: the flag-set engine with (prior, noise) == the flag-clear engine with the same t_start fed noise = last_start(), bit
     for bit, on every route x engine the case's task has; within REL of the expectation loop, seg teacher-forced with the
     expectation's decisions (DDP_FLAG_FORCE_X0) as well as free-running
  4  t_start = 1: within REL of the flag-clear noise-start output (alpha(1) = 8e-5: not bitwise)
  5  a batched call == single-image calls, bit for bit
  6  graph: captured once, replayed with a new prior == a fresh call
  7  DDP_FLAG_X0_HINTS + DDP_FLAG_STEP_RECORD + the flag in one engine
  8  engine surface, 9 the call-time ``prior=`` / ``t_start=`` of the three plugin classes

Every engine samples through a workspace that is filled with a NaN pattern and has 4 KiB guards at both ends."""
import pytest
import torch
import torch.nn.functional as F

import config_space_cases as S
import prior_start_cases as P
import support
from ddp_amd import _lib
from support import PATTERN, REL, FixedBackbone as _Backbone, dev, guards_ok as _guards_ok  # noqa: F401

pytestmark = pytest.mark.gpu

START_BAR = 2.0 ** -21
ROUTES = {(n, vid): (gemm, fl) for n, c in P.CASES.items() for vid, gemm, fl in P.routes(c)}
_state = support.state_cache(P.state_dict, S.inputs)


def _engine(c, dev, gemm='bf16x3', batch=None, **kw):
    """DDPEngine of the case on a guarded, NaN-patterned workspace.  The prior map of a prior_start engine holds the PATTERN
    afterwards: the caller sets or clears it, as the library's contract says."""
    return support.engine(_state(c, dev)[0], c['task'], S.engine_kwargs(c), dev, gemm, batch, **kw)


def _sample(eng, c, dev, prior=None, noise=None, sl=None, seed=None):
    """one call; ``prior``: a (B,h,w) tensor for a prior_start engine; ``noise``: in place of the case's; ``sl``: the image slice of a
    single-image engine; ``seed``: a seeded engine's"""
    _, (x, nz, sn) = _state(c, dev)
    if noise is not None:
        nz = noise
    if sl is not None:
        x, nz, sn = x[sl].clone(), nz[sl].clone(), None if sn is None else sn[:, sl].clone()     # (fresh, aligned allocations)
    if prior is not None:
        eng.set_prior(prior.to(dev))
    if seed is not None:
        out = eng.sample(x.contiguous(), seed=seed)
    else:
        out = eng.sample(x.contiguous(), nz.contiguous(), None if sn is None else sn.contiguous())
    torch.cuda.synchronize()
    assert _guards_ok(eng), f'{c["name"]}: workspace guards overwritten'
    return out.cpu()


def _rel(a, b):
    return P.max_rel(a, b)


def test_bars():
    assert P.REL == REL == 2e-4 and START_BAR == 2.0 ** -21


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t_start', P.T_STARTS)
@pytest.mark.parametrize('name', sorted(P.CASES))
def test_start_map_accuracy(dev, name, t_start):
    c = P.CASES[name]
    sd, (x, noise, sn) = _state(c, dev)
    worst = 0.0
    for which in (0, 1):
        pr = P.prior(c, which)
        eng = _engine(c, dev, prior_start=True, t_start=t_start)
        _sample(eng, c, dev, pr)
        got = eng.last_start().cpu().double()
        assert tuple(got.shape) == (c['B'], c['r'], 1 if c['task'] == 'depth' else 256, c['h'], c['w'])
        for b in range(c['B']):
            want = P.start_map(c, sd, pr[b], noise[b].cpu(), t_start, torch.float64)
            ta, ts = P.start_terms(c, sd, pr[b], noise[b].cpu(), t_start)
            bar = START_BAR * (ta + ts) + START_BAR * c['bit_scale']
            ratio = float(((got[b] - want).abs() / bar).max())
            worst = max(worst, ratio)
    print(f'PRIOR-START start map {name} t_start {t_start}: worst |error| / bar {worst:.3f} (bar: 2^-21 (|a x0| + |s eps|) + 2^-21 bit_scale)')
    assert worst <= 1.0


def test_start_map_with_more_items_than_blocks(dev):
    """the one size-dependent path of k_prior_start_tab: a block walks several (image, 1024-pixel chunk) items once there are more
    items than 4 blocks per CU and slab (128 on 256 CUs).  2 x 260 x 256 pixels are 130 items - and a pixel count that is a multiple
    of 4, the 16-byte path on the seg instantiation.  Same bar as above; the fp64 reference is formed on the device (136 MB map)."""
    c = dict(P.CASES['seg_kc19_7x13'], name='seg_kc19_260x256', h=260, w=256, K=1)
    sd, (x, noise, _) = _state(c, dev)
    N = c['h'] * c['w']
    assert c['B'] * ((N + 1023) // 1024) > 128 and N % 4 == 0
    g = torch.Generator().manual_seed(9)
    pr = torch.randint(0, 256, (c['B'], c['h'], c['w']), generator=g).to(torch.uint8)            # classes and ignore values
    eng = _engine(c, dev, prior_start=True, t_start=0.6)
    _sample(eng, c, dev, pr)
    a, s = P.start_scalars(c, 0.6)
    tab = (torch.sigmoid(sd['embedding_table.weight'].to(dev).double()) * 2 - 1) * c['bit_scale']
    idx = pr.to(dev).long().clamp(max=c['Kc']).view(c['B'], N)
    ax0 = (a * tab[idx]).permute(0, 2, 1).reshape(c['B'], 1, 256, c['h'], c['w'])
    se = s * noise.double()
    bar = START_BAR * (ax0.abs() + se.abs()) + START_BAR * c['bit_scale']
    worst = float(((eng.last_start().double() - (ax0 + se)).abs() / bar).max())
    print(f'PRIOR-START start map {c["name"]}: worst |error| / bar {worst:.3f}')
    _state.forget(c['name'])                                              # (the only large inputs of this file)
    assert worst <= 1.0


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(P.CASES))
def test_same_bits_from_every_writer(dev, name):
    c = P.CASES[name]
    t, pr = c['t_start'], P.prior(c, 0)
    seeded = _engine(c, dev, seeded_noise=True, t_start=t)
    _sample(seeded, c, dev, seed=77)
    eps = seeded.last_noise().clone()
    both = _engine(c, dev, seeded_noise=True, prior_start=True, t_start=t)
    out_both = _sample(both, c, dev, pr, seed=77)
    m_both = both.last_start().cpu()
    only = _engine(c, dev, prior_start=True, t_start=t)
    _sample(only, c, dev, pr, noise=eps)
    m_only = only.last_start().cpu()
    assert not torch.equal(m_both, eps.cpu()) and torch.equal(m_both, m_only), name
    with pytest.raises(_lib.DdpError, match=r'last_start\(\)'):
        both.last_noise()
    if c.get('sampler') != 'ddpm':                                        # (ddpm: the seeded step noise is not the case's tensor)
        assert torch.equal(out_both, _sample(only, c, dev, pr, noise=eps))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', sorted(ROUTES))
def test_output_is_the_flag_clear_loop_on_the_start_map(dev, name, vid):
    c = P.CASES[name]
    gemm, fl = ROUTES[(name, vid)]
    t, pr = c['t_start'], P.prior(c, 0)
    rec_kw = dict(record_x0=True) if c['task'] == 'seg' else {}
    eng = _engine(c, dev, gemm, prior_start=True, t_start=t, **rec_kw, **fl)
    got = _sample(eng, c, dev, pr)
    m0 = eng.last_start().clone()
    clear = _engine(c, dev, gemm, t_start=t, **rec_kw, **fl)
    assert clear.cfg.flags | _lib.FLAG_PRIOR_START == eng.cfg.flags
    same = _sample(clear, c, dev, noise=m0)
    assert torch.equal(got, same), (name, vid)                            # the same loop on the same bytes
    want, rec_want = P.expected(c, 0)
    e_free = _rel(got, want)
    line = f'PRIOR-START {name}[{vid}]: free-running {e_free:.2e}'
    if c['task'] == 'seg':
        own = eng.x0_trace().cpu()
        assert torch.equal(own, clear.x0_trace().cpu())
        K, B, r, h, w = c['K'], c['B'], c['r'], c['h'], c['w']
        agree = float((own.view(K, B, r, h, w) == rec_want).float().mean())
        forced = _engine(c, dev, gemm, prior_start=True, t_start=t, force_x0=True, **fl)
        forced.set_x0_decisions(rec_want.reshape(K, B * r, h, w).to(dev))
        e_forced = _rel(_sample(forced, c, dev, pr), want)                # (fed its own argmax, the expectation loop is its free run)
        line += f', teacher-forced {e_forced:.2e}, decisions equal {agree:.4f}'
        assert e_forced < REL
    print(line + f' (bar {REL:.0e})')
    assert e_free < REL
    if c['witness']:
        assert _rel(got, P.expected(c, 'noise')[0]) > P.WITNESS - REL     # ... and it is not the noise-start result


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(P.CASES))
def test_t_start_one_is_the_noise_start(dev, name):
    c = P.CASES[name]
    want = _sample(_engine(c, dev), c, dev)
    eng = _engine(c, dev, prior_start=True, t_start=1.0)
    assert [eng.steps[i].alpha for i in range(c['K'])] == [S.steps_of(c)[i].alpha for i in range(c['K'])]
    got = _sample(eng, c, dev, P.prior(c, 0))
    d, e = _rel(got, want), _rel(got, P.expected(c, 0, t_start=1.0)[0])
    print(f'PRIOR-START t_start 1 {name}: vs flag-clear noise start {d:.2e}, vs expectation {e:.2e} (bar {REL:.0e})')
    assert d < REL and e < REL
    assert not torch.equal(eng.last_start().cpu(), _state(c, dev)[1][1].cpu())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(P.CASES))
def test_batched_call_is_the_single_image_calls(dev, name):
    c = P.CASES[name]
    pr = P.prior(c, 0)
    eng = _engine(c, dev, prior_start=True, t_start=c['t_start'])
    got = _sample(eng, c, dev, pr)
    m0 = eng.last_start().cpu()
    one = _engine(c, dev, batch=1, prior_start=True, t_start=c['t_start'])
    for b in range(c['B']):
        single = _sample(one, c, dev, pr[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(single, got[b:b + 1]) and torch.equal(one.last_start().cpu(), m0[b:b + 1]), (name, b)
    # another prior for image 0 only: images 1.. keep their bits
    other = pr.clone()
    other[0] = P.prior(c, 1)[0]
    got2 = _sample(eng, c, dev, other)
    assert torch.equal(got2[1:], got[1:])
    assert (not c['witness']) or not torch.equal(got2[0], got[0])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_kc19_7x13', 'seg_kc255_5x10_r2', 'seg_ddpm_7x13', 'depth_9x14', 'depth_1x37_bins', 'bev_kc8_r1',
                                  'bev_kc9_r2'])
def test_graph_replays_pick_up_a_new_prior(dev, name):
    c = P.CASES[name]
    _, (x, noise, sn) = _state(c, dev)
    maps = [P.prior(c, 0), P.prior(c, 1), P.cleared_prior(c)]
    eng = _engine(c, dev, prior_start=True, t_start=c['t_start'])
    want = [_sample(eng, c, dev, m) for m in maps]
    assert not torch.equal(want[0], want[1])
    eng.set_prior(maps[2].to(dev))
    g = eng.capture(x, noise, sn)
    for i in (0, 1, 0, 2):
        out = g.replay(prior=maps[i].to(dev))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[i]), (name, i)
    assert torch.equal(g.replay().cpu(), want[2])                        # no prior given: what the map holds
    assert _guards_ok(eng)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_hints_step_record_and_prior_in_one_engine(dev):
    """DDP_FLAG_X0_HINTS | DDP_FLAG_STEP_RECORD | DDP_FLAG_PRIOR_START: with D_s = where(hint < K, hint, the run's recorded argmax of
    step s), the expectation loop from the start map under the decisions D is within REL, and the record holds the model's own
    decisions - the expectation's own argmax under D - not the hinted classes"""
    import x0_hint_cases as H
    c = P.CASES['seg_kc19_7x13']
    K, B, r, h, w = c['K'], c['B'], c['r'], c['h'], c['w']
    hints = H.partial_hints(c)
    pr = P.prior(c, 0)
    eng = _engine(c, dev, prior_start=True, x0_hints=True, record_steps=True, t_start=c['t_start'])
    eng.set_hints(hints.to(dev))
    got = _sample(eng, c, dev, pr)
    rec = eng.step_record().cpu()                                         # (K, B, r, h, w)
    hr = hints[None, :, None].expand(K, -1, r, -1, -1)
    D = torch.where(hr < c['Kc'], hr, rec)
    own = []
    want = P.run_from(c, P.starts_of(c, pr, c['t_start']), c['t_start'], record=own, x0_index=D)
    own = torch.stack([torch.stack(o, 0) for o in own], 1)
    e = _rel(got, want)
    on = hr < c['Kc']
    differ = float((rec[on] != hr[on]).float().mean())
    print(f'PRIOR-START hints + record: max-rel {e:.2e} (bar {REL:.0e}); the record differs from the hints at {differ:.3f} of the hinted pixels')
    assert e < REL and torch.equal(rec, own) and differ > 0
    # the hints have an effect on top of the prior (K = 2: through the one update)
    plain = _sample(_engine(c, dev, prior_start=True, t_start=c['t_start']), c, dev, pr)
    assert not torch.equal(plain, got)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_engine_prior_methods(dev):
    from ddp_amd.engine import DDPEngine
    c = P.CASES['seg_kc19_7x13']
    sd, _ = _state(c, dev)
    eng = DDPEngine(sd, 'seg', device=dev, prior_start=True, t_start=0.6, record_steps=True, **S.engine_kwargs(c))
    v = eng.prior_view()
    assert v.dtype == torch.uint8 and tuple(v.shape) == (c['B'], c['h'], c['w']) and bool((v == 255).all())     # allocated: cleared
    pb, sb = P.prior_bytes(c)
    rec, smap = (c['K'] * c['B'] * c['r'] * c['h'] * c['w'], c['B'] * c['h'] * c['w'] * 4)
    off = v.data_ptr() - eng.workspace.data_ptr()
    assert off == eng.workspace.numel() * 4 - P.round256(rec) - P.round256(smap) - P.round256(pb)               # the header's formula
    with pytest.raises(_lib.DdpError, match='sample'):
        eng.last_start()
    eng.set_prior(P.prior(c, 0).to(dev))
    assert not bool((eng.prior_view() == 255).all())
    for bad in (P.prior(c, 0), P.prior(c, 0).to(dev).float(), P.prior(c, 0).to(dev)[:1]):                        # device, dtype, shape
        with pytest.raises(_lib.DdpError):
            eng.set_prior(bad)
    eng.set_geometry(batch=c['B'], h=c['h'] + 1, w=c['w'])                                                      # every set_geometry: cleared
    assert bool((eng.prior_view() == 255).all()) and tuple(eng.prior_view().shape) == (c['B'], c['h'] + 1, c['w'])
    eng.set_prior(torch.zeros_like(eng.prior_view()))
    eng.set_geometry(batch=c['B'], h=4 * c['h'], w=4 * c['w'])                                                  # regrown workspace
    assert bool((eng.prior_view() == 255).all())
    assert eng._prior_places()[2] == off_of(eng) - P.round256(eng._prior_places()[3])                           # (the start map sits in front)
    d = P.CASES['depth_9x14']
    deng = DDPEngine(_state(d, dev)[0], 'depth', device=dev, prior_start=True, t_start=0.25, **S.engine_kwargs(d))
    assert deng.prior_view().dtype == torch.float32 and bool((deng.prior_view() == 0).all())
    b = P.CASES['bev_kc9_r2']
    beng = DDPEngine(_state(b, dev)[0], 'bev', device=dev, prior_start=True, seeded_noise=True, **S.engine_kwargs(b))
    assert beng.prior_view().dtype == torch.int32 and bool((beng.prior_view() == 0).all()) and beng.t_start == 1.0
    plain = DDPEngine(sd, 'seg', device=dev, **S.engine_kwargs(c))
    for m in (plain.prior_view, plain.clear_prior, plain.last_start):
        with pytest.raises(_lib.DdpError, match='prior_start'):
            m()
    for bad in (0.0, 1.5):
        with pytest.raises(ValueError, match='t_start'):
            DDPEngine(sd, 'seg', device=dev, t_start=bad, **S.engine_kwargs(c))
    b33 = dict(S.CASES['bev_kc32_r1'], Kc=33)
    with pytest.raises(ValueError, match='prior_start'):
        DDPEngine(S.state_dict(b33), 'bev', device=dev, prior_start=True, **S.engine_kwargs(b33))
    # ddp_head_forward ignores the flag
    feat = torch.randn(c['B'] * c['r'], 256, c['h'], c['w'], generator=torch.Generator().manual_seed(3)).to(dev)
    heng = _engine(c, dev, prior_start=True, t_start=0.6)
    assert torch.equal(heng.head_forward(feat, None).cpu(), _engine(c, dev, t_start=0.6).head_forward(feat, None).cpu()) and _guards_ok(heng)


def off_of(eng):
    return eng.prior_view().data_ptr() - eng.workspace.data_ptr()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def _image_frame(c, prior_map, ratio=(3.5, 2.75)):
    """the prior in the frame of a network input whose size is a NON-integer multiple of the map: every map pixel's value is written
    to the image pixel nearest resampling reads for it - floor(dst * in / out) - and everything else is poison, so that any other
    resampling rule shows"""
    B, h, w = prior_map.shape
    Hp, Wp = int(h * ratio[0]) + 1, int(w * ratio[1]) + 2
    ys = torch.floor(torch.arange(h, dtype=torch.float32) * (Hp / h)).long()
    xs = torch.floor(torch.arange(w, dtype=torch.float32) * (Wp / w)).long()
    poison = {'seg': 0, 'depth': 0.5 * (c.get('min_depth', 0) + c.get('max_depth', 0)), 'bev': -1}[c['task']]
    img = torch.full((B, Hp, Wp), poison, dtype=prior_map.dtype)
    img[:, ys[:, None], xs[None, :]] = prior_map
    return img


@pytest.mark.parametrize('name', ['seg_kc19_7x13', 'seg_kc255_5x10_r2', 'seg_ddpm_7x13'])
def test_plugin_seg_prior(dev, name):
    c = P.CASES[name]
    _, (x, noise, sn) = _state(c, dev)
    t = c['t_start']
    img_prior = _image_frame(c, P.prior(c, 0)).to(dev)
    model = support.seg_plugin(c, dev, P.state_dict(c))
    want, _ = P.expected(c, 0)
    if c['sampler'] == 'ddim':
        sample, kw = model.ddim_sample, dict(noise=noise)
    else:
        sample, kw = model.ddpm_sample, dict(noise=noise, step_noise=sn)
    out = sample(x, None, prior=img_prior, t_start=t, **kw)
    e = _rel(out.cpu(), want)
    e_t = _rel(sample(x, None, t_start=t, **kw).cpu(), P.expected(c, 'noise')[0])       # t_start alone: the noise as the start map
    print(f'PRIOR-START plugin {name}: max-rel {e:.2e}, t_start alone {e_t:.2e} (bar {REL:.0e})')
    assert e < REL and e_t < REL
    assert len(model._engine_cache) == 2                                   # prior / t_start are part of the engine key
    # simple_test / forward: the labels are the argmax of those scores resized to the image (the noise drawn as the reference does)
    model.backbone = _Backbone(x)
    Hp, Wp = img_prior.shape[1:]
    img = torch.zeros(c['B'], 3, Hp, Wp, device=dev)
    torch.manual_seed(11)
    drawn = torch.randn((c['B'], c['r'], 256, c['h'], c['w']), device=dev)
    dsn = torch.randn((c['K'], c['B'], c['r'], 256, c['h'], c['w']), device=dev) if c['sampler'] == 'ddpm' else None
    kw = dict(noise=drawn) if dsn is None else dict(noise=drawn, step_noise=dsn)
    scores = sample(x, None, prior=img_prior, t_start=t, **kw)
    ref = F.interpolate(scores, size=(Hp, Wp), mode='bilinear', align_corners=False).argmax(1).cpu()
    for call in (lambda: model.simple_test(img, None, rescale=False, prior=img_prior, t_start=t),
                 lambda: model(img=[img], img_metas=None, return_loss=False, rescale=False, prior=[img_prior], t_start=t)):
        torch.manual_seed(11)
        lab = torch.from_numpy(__import__('numpy').stack(call()))
        assert lab.shape == ref.shape and float((lab != ref).float().mean()) < 1e-3
    # what is not built raises ValueError
    with pytest.raises(ValueError, match='prior'):
        model.aug_test([img, img], [None, None], prior=img_prior, t_start=t)
    with pytest.raises(ValueError, match='prior'):
        model(img=[img, img], img_metas=[None, None], return_loss=False, prior=img_prior, t_start=t)
    model.test_cfg = dict(mode='slide', crop_size=(8, 8), stride=(4, 4))
    with pytest.raises(ValueError, match='prior'):
        model.simple_test(img, None, rescale=False, prior=img_prior, t_start=t)
    with pytest.raises(ValueError, match='prior'):
        model.slide_inference(img, None, False, prior=img_prior, t_start=t)
    model.test_cfg = dict(mode='whole')
    with pytest.raises(ValueError, match='prior'):
        model.ddim_sample(x, None, noise=noise, prior=img_prior[:1], t_start=t)
    with pytest.raises(ValueError, match='t_start'):
        model.ddim_sample(x, None, noise=noise, prior=img_prior)


@pytest.mark.parametrize('name', ['depth_9x14', 'depth_5x10_r2', 'depth_1x37_bins'])
def test_plugin_depth_prior(dev, name):
    c = P.CASES[name]
    _, (x, noise, _) = _state(c, dev)
    t = c['t_start']
    img_prior = _image_frame(c, P.prior(c, 0)).to(dev)
    model = support.depth_plugin(c, dev, P.state_dict(c))
    out = model.sample(x, None, noise=noise, prior=img_prior, t_start=t)
    e = _rel(out.cpu(), P.expected(c, 0)[0])
    e_t = _rel(model.sample(x, None, noise=noise, t_start=t).cpu(), P.expected(c, 'noise')[0])
    print(f'PRIOR-START plugin {name}: max-rel {e:.2e}, t_start alone {e_t:.2e} (bar {REL:.0e})')
    assert e < REL and e_t < REL
    # simple_test / forward: clamp + bilinear resize of that map (depther/ddp.py:95-109), the noise drawn as the reference does
    model.backbone = _Backbone(x)
    Hp, Wp = img_prior.shape[1:]
    img = torch.zeros(c['B'], 3, Hp, Wp, device=dev)
    torch.manual_seed(12)
    drawn = torch.randn((c['B'], c['r'], 1, c['h'], c['w']), device=dev)
    low = model.sample(x, None, noise=drawn, prior=img_prior, t_start=t)
    ref = F.interpolate(low.clamp(c['min_depth'], c['max_depth']), size=(Hp, Wp), mode='bilinear', align_corners=False).cpu()
    meta = [dict(ori_shape=(Hp, Wp, 3), img_shape=(Hp, Wp, 3), pad_shape=(Hp, Wp, 3))] * c['B']
    for call in (lambda: model.simple_test(img, meta, rescale=True, prior=img_prior, t_start=t),
                 lambda: model(img=[img], img_metas=[meta], return_loss=False, rescale=True, prior=[img_prior], t_start=t)):
        torch.manual_seed(12)
        got = torch.from_numpy(__import__('numpy').stack(call()))
        assert got.shape == ref.shape and _rel(got, ref) < REL
    with pytest.raises(ValueError, match='prior'):
        model.aug_test([img, img], [meta, meta], prior=img_prior, t_start=t)
    with pytest.raises(ValueError, match='prior'):
        model(img=[img, img], img_metas=[meta, meta], return_loss=False, prior=img_prior, t_start=t)


def test_plugin_bev_prior(dev):
    """the bev plugin class has the reference's six classes: the geometry of bev_kc8_r1 with 6"""
    c = dict(P.CASES['bev_kc8_r1'], Kc=6, name='bev_kc6_plugin')
    sd, (x, noise, _) = _state(c, dev)
    t = c['t_start']
    pr = P.prior(c, 0)
    img_prior = _image_frame(c, pr).to(dev)
    model, head = support.bev_plugin(sd, dev, c['L'], S.bev_scopes(c), bit_scale=c['bit_scale'], timesteps=c['K'], randsteps=c['r'],
                                     feat_channels=c['Cx'], threshold=c['threshold'], time_difference=c['td'])
    out = model.ddim_sample([x], head, noise=noise, prior=img_prior, t_start=t)
    want = P.run_from(c, P.starts_of(c, pr, t), t)
    away = P.run_from(c, S.inputs(c)[1], t)
    e, e_t = _rel(out.cpu(), want), _rel(model.ddim_sample([x], head, noise=noise, t_start=t).cpu(), away)
    print(f'PRIOR-START plugin bev: max-rel {e:.2e}, t_start alone {e_t:.2e} (bar {REL:.0e}); prior vs noise start {_rel(want, away):.2e}')
    assert e < REL and e_t < REL and _rel(want, away) > P.WITNESS
    with pytest.raises(ValueError, match='t_start'):
        model.ddim_sample([x], head, noise=noise, prior=img_prior)
