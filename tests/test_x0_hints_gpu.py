"""DDP_FLAG_X0_HINTS on the GPU, per route x engine.  Needs an MI355X: ``pytest -m gpu``.  (CPU companion: tests/test_x0_hints_host.py;
cases, hint maps and the hinted expectation: tests/x0_hint_cases.py.)

  1  all-free hints == the flag-clear engine, torch.equal on outputs, step records and disagreement maps; the launch records show
     the same kernels per tag plus the one expand launch
  2  seg, every pixel hinted == a DDP_FLAG_FORCE_X0 engine fed those classes at every step, bit for bit
  3  seg, partial hints: with D_s = where(hint < K, hint, the run's own recorded argmax of step s), a FORCE_X0 engine fed D is
     bit-identical, O.ddim_sample_seg(x0_index=D) and the free-running hinted helper are within REL; ddim, ddpm and ddpm with
     DDP_FLAG_DDPM_CHAIN (the chain against the flag-clear route at CHAIN_VS_CLEAR)
  4  depth, sparse hints within REL of the hinted helper; the record still holds the model's own prediction
  5  a batched call == single-image calls bit for bit; the hints of image b change nothing in image b' != b
  6  graph: captured once, replayed with two hint maps, each replay == the uncaptured call bit for bit
  7  plugin surface: ``hints=`` through ddim_sample / ddpm_sample / sample / simple_test / forward with the nearest resampling at a
     non-integer ratio; the ValueError cases

Every engine samples through a workspace that is filled with a NaN pattern and has 4 KiB guards at both ends (the carve of the two
new buffers; a kernel that reads hint bytes nobody wrote shows: the pattern's bytes are classes < 150 and a NaN)."""
import pytest
import torch
import torch.nn.functional as F

import config_space_cases as S
import support
import x0_hint_cases as H
from ddp_amd import _lib
from ddpm_chain_cases import CHAIN_VS_CLEAR
from oracle import ddp_oracle as O
from support import PATTERN, REL, FixedBackbone as _Backbone, dev, guards_ok as _guards_ok  # noqa: F401

pytestmark = pytest.mark.gpu

ROUTES = {(n, vid): (gemm, fl) for n, c in H.CASES.items() for vid, gemm, fl in H.routes(c)}
_state = support.state_cache(S.state_dict, S.inputs)


def _engine(c, dev, gemm='bf16x3', batch=None, **kw):
    """DDPEngine of the case on a guarded, NaN-patterned workspace.  The hint map of an x0_hints engine holds the PATTERN afterwards:
    the caller sets or clears the hints, as the library's contract says."""
    return support.engine(_state(c, dev)[0], c['task'], S.engine_kwargs(c), dev, gemm, batch, **kw)


def _sample(eng, c, dev, hints=None, sl=None):
    """one call; ``hints``: None (no x0_hints engine), 'nan-pattern' (leave the workspace pattern in the map) or a (B,h,w) tensor;
    ``sl``: the image slice of a single-image engine"""
    _, (x, noise, sn) = _state(c, dev)
    if sl is not None:
        x, noise, sn = x[sl].clone(), noise[sl].clone(), None if sn is None else sn[:, sl].clone()     # (fresh, aligned allocations)
    if torch.is_tensor(hints):
        eng.set_hints(hints.to(dev))
    out = eng.sample(x.contiguous(), noise.contiguous(), None if sn is None else sn.contiguous())
    torch.cuda.synchronize()
    assert _guards_ok(eng), f'{c["name"]}: workspace guards overwritten'
    return out.cpu()


def _counts(eng, c, dev):
    return support.launch_counts(eng, *_state(c, dev)[1])


def _rel(a, b):
    return H.max_rel(a, b)


def test_bars():
    assert H.REL == REL == 2e-4 and CHAIN_VS_CLEAR == 5e-5


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', sorted(ROUTES))
def test_free_hints_are_the_flag_clear_engine(dev, name, vid):
    c = H.CASES[name]
    gemm, fl = ROUTES[(name, vid)]
    clear = _engine(c, dev, gemm, record_steps=True, **fl)
    hint = _engine(c, dev, gemm, record_steps=True, x0_hints=True, **fl)
    assert hint.cfg.flags == clear.cfg.flags | _lib.FLAG_X0_HINTS
    want = _sample(clear, c, dev)
    # free as the engine writes it, and free in other encodings: seg a value in [K, 255), depth NaN / -1 / inf (the workspace pattern is a NaN)
    maps = [H.free_hints(c)]
    if c['task'] == 'seg':
        if c['Kc'] < 255:
            maps.append(torch.full_like(maps[0], c['Kc']))
    else:
        maps.append('nan-pattern')
        alt = torch.full_like(maps[0], -1.0)
        alt.view(-1)[::2] = float('inf')
        maps.append(alt)
    for m in maps:
        if not torch.is_tensor(m):
            hint.hints_view().view(torch.int32).fill_(PATTERN)
        got = _sample(hint, c, dev, m)
        assert torch.equal(got, want), (name, vid)
        assert torch.equal(hint.step_record().cpu(), clear.step_record().cpu())
        assert torch.equal(hint.step_disagreement().cpu(), clear.step_disagreement().cpu())
    hint.clear_hints()
    a, b = _counts(clear, c, dev), _counts(hint, c, dev)
    print(f'X0-HINTS launches {name}[{vid}]: clear {a} hinted {b}')
    assert {t: b[t] for t in range(1, 11)} == {t: a[t] for t in range(1, 11)} and b[0] == a[0] + 1


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------------
def _forced(c, dev, gemm, fl, decisions):
    eng = _engine(c, dev, gemm, force_x0=True, **fl)
    eng.set_x0_decisions(decisions.to(dev))
    out = _sample(eng, c, dev)
    return out, eng.x0_trace().cpu()


@pytest.mark.parametrize('name,vid', sorted(k for k in ROUTES if H.CASES[k[0]]['task'] == 'seg'))
def test_seg_full_hints_are_teacher_forcing(dev, name, vid):
    c = H.CASES[name]
    gemm, fl = ROUTES[(name, vid)]
    hints = H.full_hints(c)
    eng = _engine(c, dev, gemm, x0_hints=True, record_x0=True, **fl)
    got = _sample(eng, c, dev, hints)
    own = eng.x0_trace().cpu()                                            # (K, B*r, h, w): the model's own argmax
    dec = hints[:, None].expand(-1, c['r'], -1, -1).reshape(1, c['B'] * c['r'], c['h'], c['w']).expand(c['K'], -1, -1, -1)
    want, own_forced = _forced(c, dev, gemm, fl, dec.contiguous())
    assert torch.equal(got, want) and torch.equal(own, own_forced), (name, vid)


@pytest.mark.parametrize('name,vid', sorted(k for k in ROUTES if H.CASES[k[0]]['task'] == 'seg'))
def test_seg_partial_hints(dev, name, vid):
    c = H.CASES[name]
    gemm, fl = ROUTES[(name, vid)]
    B, r, K, h, w = c['B'], c['r'], c['K'], c['h'], c['w']
    hints = H.partial_hints(c)
    eng = _engine(c, dev, gemm, x0_hints=True, record_x0=True, **fl)
    got = _sample(eng, c, dev, hints)
    rec = eng.x0_trace().cpu()                                            # (K, B*r, h, w)
    hr = hints[:, None].expand(-1, r, -1, -1).reshape(1, B * r, h, w).expand(K, -1, -1, -1)
    D = torch.where(hr < c['Kc'], hr, rec)
    want, own_forced = _forced(c, dev, gemm, fl, D)
    assert torch.equal(got, want) and torch.equal(rec, own_forced), (name, vid)
    # the oracle under the same decisions, image by image
    sd = S.state_dict(c)
    x, noise, sn = S.inputs(c)
    Db = D.view(K, B, r, h, w)
    errs = []
    for b in range(B):
        idx = [Db[s, b] for s in range(K)]
        if c['sampler'] == 'ddim':
            with torch.no_grad():
                ref = O.ddim_sample_seg(x[b:b + 1], noise[b], sd, timesteps=K, randsteps=r, bit_scale=c['bit_scale'], time_difference=c['td'],
                                        accumulation=c['accumulation'], x0_index=idx)
        else:       # (O.ddpm_sample_seg takes no decisions: the helper's ddpm branch, which is that function line by line)
            ref = H.seg_image(c, sd, x[b:b + 1], noise[b], sn[:, b], hints[b], x0_index=idx)
        errs.append(_rel(got[b:b + 1], ref))
    free_run, rec_ref = H.expected(c, 'partial')
    e_free = _rel(got, free_run)
    agree = float((rec.view(K, B, r, h, w) == rec_ref).float().mean())
    print(f'X0-HINTS seg {name}[{vid}]: forced-oracle max-rel {" ".join(f"{e:.2e}" for e in errs)}, free-running helper {e_free:.2e} '
          f'(bar {REL:.0e}), own decisions equal {agree:.4f}')
    assert max(errs) < REL and e_free < REL
    if c['witness']:
        assert _rel(got, H.expected(c, 'free')[0]) > H.WITNESS - REL      # ... and it is not the unhinted sampler's result
    if vid.startswith('chain'):
        plain = {k: v for k, v in fl.items() if k != 'ddpm_chain'}
        base = _sample(_engine(c, dev, gemm, x0_hints=True, **plain), c, dev, hints)
        d = _rel(got, base)
        print(f'X0-HINTS chain vs flag-clear route {name}[{vid}]: {d:.2e} (bar {CHAIN_VS_CLEAR:.0e})')
        assert d < CHAIN_VS_CLEAR


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['partial', 'full'])
@pytest.mark.parametrize('name,vid', sorted(k for k in ROUTES if H.CASES[k[0]]['task'] == 'depth'))
def test_depth_hints(dev, name, vid, kind):
    c = H.CASES[name]
    gemm, fl = ROUTES[(name, vid)]
    hints = {'partial': H.partial_hints, 'full': H.full_hints}[kind](c)
    eng = _engine(c, dev, gemm, x0_hints=True, record_steps=True, **fl)
    got = _sample(eng, c, dev, hints)
    want, rec_want = H.expected(c, kind)
    e, e_rec = _rel(got, want), _rel(eng.step_record().cpu(), rec_want)
    away = _rel(got, H.expected(c, 'free')[0])
    print(f'X0-HINTS depth {name}[{vid}] {kind}: max-rel {e:.2e}, record {e_rec:.2e} (bar {REL:.0e}); from the unhinted result {away:.2e}')
    assert torch.isfinite(got).all() and e < REL and e_rec < REL and away > H.WITNESS - REL


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('name', sorted(H.CASES))
def test_batched_call_is_the_single_image_calls(dev, name, gemm):
    c = H.CASES[name]
    hints = H.partial_hints(c)
    eng = _engine(c, dev, gemm, x0_hints=True)
    got = _sample(eng, c, dev, hints)
    one = _engine(c, dev, gemm, batch=1, x0_hints=True)
    for b in range(c['B']):
        single = _sample(one, c, dev, hints[b:b + 1], sl=slice(b, b + 1))
        assert torch.equal(single, got[b:b + 1]), (name, gemm, b)
    # other hints for image 0 only: images 1.. keep their bits, image 0 does not (where hints can have an effect)
    other = hints.clone()
    other[0] = H.free_hints(c)[0]
    got2 = _sample(eng, c, dev, other)
    assert torch.equal(got2[1:], got[1:])
    assert (not c['witness']) or not torch.equal(got2[0], got[0])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_kc19_7x13', 'seg_kc255_5x10_r2', 'seg_ddpm_7x13', 'depth_9x14', 'depth_5x10_r2', 'depth_1x37_bins'])
def test_graph_replays_pick_up_new_hints(dev, name):
    c = H.CASES[name]
    _, (x, noise, sn) = _state(c, dev)
    maps = [H.partial_hints(c), H.full_hints(c), H.free_hints(c)]
    eng = _engine(c, dev, x0_hints=True)
    want = [_sample(eng, c, dev, m) for m in maps]
    assert not torch.equal(want[0], want[1])
    eng.set_hints(maps[2].to(dev))
    g = eng.capture(x, noise, sn)
    for i in (0, 1, 0, 2):
        out = g.replay(hints=maps[i].to(dev))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want[i]), (name, i)
    assert torch.equal(g.replay().cpu(), want[2])                        # no hints given: what the map holds
    assert _guards_ok(eng)


# ---- engine surface -----------------------------------------------------------------------------------------------------------------
def test_engine_hint_methods(dev):
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine
    c = H.CASES['seg_kc19_7x13']
    sd, _ = _state(c, dev)
    eng = DDPEngine(sd, 'seg', device=dev, x0_hints=True, record_steps=True, **S.engine_kwargs(c))
    v = eng.hints_view()
    assert v.dtype == torch.uint8 and tuple(v.shape) == (c['B'], c['h'], c['w']) and bool((v == 255).all())     # allocated: all free
    hb, _ = H.hint_bytes(c)
    rec, smap = (c['K'] * c['B'] * c['r'] * c['h'] * c['w'], c['B'] * c['h'] * c['w'] * 4)
    off = v.data_ptr() - eng.workspace.data_ptr()
    assert off == eng.workspace.numel() * 4 - H.round256(rec) - H.round256(smap) - H.round256(hb)               # the header's formula
    eng.set_hints(H.partial_hints(c).to(dev))
    assert not bool((eng.hints_view() == 255).all())
    for bad in (H.partial_hints(c), H.partial_hints(c).to(dev).float(), H.partial_hints(c).to(dev)[:1]):         # device, dtype, shape
        with pytest.raises(_lib.DdpError):
            eng.set_hints(bad)
    eng.set_geometry(batch=c['B'], h=c['h'] + 1, w=c['w'])                                                      # every set_geometry: all free
    assert bool((eng.hints_view() == 255).all()) and tuple(eng.hints_view().shape) == (c['B'], c['h'] + 1, c['w'])
    eng.set_hints(torch.zeros_like(eng.hints_view()))
    eng.set_geometry(batch=c['B'], h=4 * c['h'], w=4 * c['w'])                                                  # regrown workspace
    assert bool((eng.hints_view() == 255).all())
    eng.clear_hints()
    d = H.CASES['depth_9x14']
    sdd, _ = _state(d, dev)
    deng = DDPEngine(sdd, 'depth', device=dev, x0_hints=True, **S.engine_kwargs(d))
    assert deng.hints_view().dtype == torch.float32 and bool((deng.hints_view() == 0).all())
    plain = DDPEngine(sd, 'seg', device=dev, **S.engine_kwargs(c))
    with pytest.raises(_lib.DdpError, match='x0_hints'):
        plain.hints_view()
    with pytest.raises(ValueError, match='x0_hints'):
        DDPEngine(sd, 'seg', device=dev, x0_hints=True, force_x0=True, **S.engine_kwargs(c))
    b = S.CASES['bev_kc8_r1']
    with pytest.raises(ValueError, match='x0_hints'):
        DDPEngine(S.state_dict(b), 'bev', device=dev, x0_hints=True, **S.engine_kwargs(b))
    with pytest.raises(_lib.DdpError, match='DDP_FLAG_X0_HINTS'):
        DDPEngine(S.state_dict(dict(c, Kc=256)), 'seg', device=dev, x0_hints=True, **S.engine_kwargs(dict(c, Kc=256)))
    # K = 1 is accepted and the hints have no effect
    c1 = dict(c, K=1, name='seg_k1')
    e1 = _engine(c1, dev, x0_hints=True)
    assert torch.equal(_sample(e1, c1, dev, H.full_hints(c1)), _sample(e1, c1, dev, H.free_hints(c1)))
    # ddp_head_forward ignores the flag
    feat = torch.randn(c['B'] * c['r'], 256, c['h'], c['w'], generator=torch.Generator().manual_seed(3)).to(dev)
    heng = _engine(c, dev, x0_hints=True)
    assert torch.equal(heng.head_forward(feat, None).cpu(), _engine(c, dev).head_forward(feat, None).cpu()) and _guards_ok(heng)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def _image_frame_hints(c, hints_map, ratio=(3.5, 2.75)):
    """hints in the frame of a network input whose size is a NON-integer multiple of the map: every map pixel's value is written to
    the image pixels that F.interpolate(mode='nearest') reads for it - floor(dst * in / out) - and everything else is poison (seg:
    another class / free flipped, depth: another depth), so that any other resampling rule shows"""
    B, h, w = hints_map.shape
    Hh, Wh = int(h * ratio[0]) + 1, int(w * ratio[1]) + 2
    ys = torch.floor(torch.arange(h, dtype=torch.float32) * (Hh / h)).long()
    xs = torch.floor(torch.arange(w, dtype=torch.float32) * (Wh / w)).long()
    if hints_map.dtype == torch.uint8:
        img = torch.full((B, Hh, Wh), 0, dtype=torch.uint8)
    else:
        img = torch.full((B, Hh, Wh), 0.5 * (c['min_depth'] + c['max_depth']), dtype=torch.float32)
    img[:, ys[:, None], xs[None, :]] = hints_map
    assert torch.equal(F.interpolate(img[:, None].float(), size=(h, w), mode='nearest')[:, 0].to(hints_map.dtype).nan_to_num(-7.0),
                       hints_map.nan_to_num(-7.0))
    return img


@pytest.mark.parametrize('name', ['seg_kc19_7x13', 'seg_kc255_5x10_r2', 'seg_ddpm_7x13'])
def test_plugin_seg_hints(dev, name):
    c = H.CASES[name]
    _, (x, noise, sn) = _state(c, dev)
    hints = H.partial_hints(c)
    img_hints = _image_frame_hints(c, hints).to(dev)
    model = support.seg_plugin(c, dev, S.state_dict(c))
    want, _ = H.expected(c, 'partial')
    if c['sampler'] == 'ddim':
        out = model.ddim_sample(x, None, noise=noise, hints=img_hints)
    else:
        out = model.ddpm_sample(x, None, noise=noise, step_noise=sn, hints=img_hints)
    e = _rel(out.cpu(), want)
    print(f'X0-HINTS plugin {name}: max-rel {e:.2e} (bar {REL:.0e})')
    assert e < REL
    # simple_test / forward: the labels are the argmax of the hinted scores resized to the image (the noise drawn as the reference does)
    model.backbone = _Backbone(x)
    Hh, Wh = img_hints.shape[1:]
    img = torch.zeros(c['B'], 3, Hh, Wh, device=dev)
    torch.manual_seed(11)
    drawn = torch.randn((c['B'], c['r'], 256, c['h'], c['w']), device=dev)
    dsn = torch.randn((c['K'], c['B'], c['r'], 256, c['h'], c['w']), device=dev) if c['sampler'] == 'ddpm' else None
    sample = model.ddim_sample if c['sampler'] == 'ddim' else model.ddpm_sample
    kw = dict(noise=drawn) if dsn is None else dict(noise=drawn, step_noise=dsn)
    scores = sample(x, None, hints=img_hints, **kw)
    ref = F.interpolate(scores, size=(Hh, Wh), mode='bilinear', align_corners=False).argmax(1).cpu()
    for call in (lambda: model.simple_test(img, None, rescale=False, hints=img_hints),
                 lambda: model(img=[img], img_metas=None, return_loss=False, rescale=False, hints=[img_hints])):
        torch.manual_seed(11)
        lab = torch.from_numpy(__import__('numpy').stack(call()))
        assert lab.shape == ref.shape and float((lab != ref).float().mean()) < 1e-3
    # what is not built raises ValueError
    with pytest.raises(ValueError, match='hints'):
        model.aug_test([img, img], [None, None], hints=img_hints)
    with pytest.raises(ValueError, match='hints'):
        model(img=[img, img], img_metas=[None, None], return_loss=False, hints=img_hints)
    model.test_cfg = dict(mode='slide', crop_size=(8, 8), stride=(4, 4))
    with pytest.raises(ValueError, match='hints'):
        model.simple_test(img, None, rescale=False, hints=img_hints)
    with pytest.raises(ValueError, match='hints'):
        model.slide_inference(img, None, False, hints=img_hints)
    model.test_cfg = dict(mode='whole')
    with pytest.raises(ValueError, match='hints'):
        model.ddim_sample(x, None, noise=noise, hints=img_hints[:1])


@pytest.mark.parametrize('name', ['depth_9x14', 'depth_5x10_r2', 'depth_1x37_bins'])
def test_plugin_depth_hints(dev, name):
    c = H.CASES[name]
    _, (x, noise, _) = _state(c, dev)
    hints = H.partial_hints(c)
    img_hints = _image_frame_hints(c, hints).to(dev)
    model = support.depth_plugin(c, dev, S.state_dict(c))
    want, rec_want = H.expected(c, 'partial')
    out, rec, _ = model.sample(x, None, noise=noise, hints=img_hints, return_steps=True)
    e, e_rec = _rel(out.cpu(), want), _rel(rec.cpu(), rec_want)
    print(f'X0-HINTS plugin {name}: max-rel {e:.2e}, record {e_rec:.2e} (bar {REL:.0e})')
    assert e < REL and e_rec < REL
    # simple_test / forward: clamp + bilinear resize of the hinted map (depther/ddp.py:95-109), the noise drawn as the reference does
    model.backbone = _Backbone(x)
    Hh, Wh = img_hints.shape[1:]
    img = torch.zeros(c['B'], 3, Hh, Wh, device=dev)
    torch.manual_seed(12)
    drawn = torch.randn((c['B'], c['r'], 1, c['h'], c['w']), device=dev)
    low = model.sample(x, None, noise=drawn, hints=img_hints)
    ref = F.interpolate(low.clamp(c['min_depth'], c['max_depth']), size=(Hh, Wh), mode='bilinear', align_corners=False).cpu()
    meta = [dict(ori_shape=(Hh, Wh, 3), img_shape=(Hh, Wh, 3), pad_shape=(Hh, Wh, 3))] * c['B']
    for call in (lambda: model.simple_test(img, meta, rescale=True, hints=img_hints),
                 lambda: model(img=[img], img_metas=[meta], return_loss=False, rescale=True, hints=[img_hints])):
        torch.manual_seed(12)
        got = torch.from_numpy(__import__('numpy').stack(call()))
        assert got.shape == ref.shape and _rel(got, ref) < REL
    with pytest.raises(ValueError, match='hints'):
        model.aug_test([img, img], [meta, meta], hints=img_hints)
    with pytest.raises(ValueError, match='hints'):
        model(img=[img, img], img_metas=[meta, meta], return_loss=False, hints=img_hints)
