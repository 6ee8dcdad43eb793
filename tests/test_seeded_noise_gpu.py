"""DDP_FLAG_SEEDED_NOISE on the GPU (``pytest -m gpu``): start noise and ddpm step noise generated on the device from a key.

Every engine samples through the guarded, NaN-patterned workspace of tests/test_config_space_gpu.py; the noise buffer sits in front
of the step-record buffers or at the very end, so an overrun lands in the rear guard.  Shapes (tests/seeded_noise_util.py): seg and
the FCN loop 7 x 13 (w % 4 != 0: counter groups straddle rows), depth 1 x 37 and 5 x 9 (Cm = 1: the last counter of an image is used
in part), bev 5 x 9; L = 2, K = 3 (depth 4), r in {1, 2}, B in {1, 3}.

  1 values        last_noise() against the NumPy restatement, element by element: |gpu - ref| <= 8 * 2^-23 * max(1, rad)
  2 consumption   a seeded ddim call == an unseeded call fed last_noise().clone(), bit for bit, on every task / engine / route
  3 ddpm          the token-major writer == the NCHW writer: an unseeded ddpm call fed the step noise rebuilt from seeded ddim
                  engines (stream_base = 1 + s) == the seeded ddpm call, bit for bit (ddp_sample r = 2, ddp_sample_fcn)
  4 cutting       B = 3 at image_base 5 == three B = 1 calls at 5, 6, 7 (noise and outputs, bit for bit); call / seed /
                  image_base change the noise
  5 graph         capture with seed A, replay with seed B == an eager call with seed B; a replay without arguments repeats it
  6 fence         guards intact; seeded_noise=False: the launch records of _expected, the parent's bits
  7 launches      tag 0: ddim + 1 per call; ddpm + 1 per call + 1 per noise-adding step (in place of the untagged transpose)
  8 plugins       DDP(noise_seed=7).simple_test on a batch of 3 == three single-image calls with image_base = i; noise_seed=None
                  unchanged; aug_test uses two call values; sample_sharded over [a, b) == the slice of the whole-batch call
"""
import numpy as np
import pytest
import torch

import config_space_cases as S
import seeded_noise_util as U
import support
from ddp_amd import _lib
from support import assert_guards, dev, guard, launch_counts  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = U.SEED


def _engine(c, dev, seeded, batch=None, gemm='bf16x3', **flags):
    return support.engine(S.state_dict(c), c['task'], S.engine_kwargs(c), dev, gemm, batch, seeded_noise=seeded, **flags)


_FCN_MODELS = {}


def _fcn_engine(c, dev, seeded, batch=None, sampler=None, record_steps=False):
    import ddp_amd
    from ddp_amd.engine import FcnSamplerEngine
    from ddp_amd.utils import synthetic
    key = (c['num_convs'], c['Kc'])
    if key not in _FCN_MODELS:
        model = ddp_amd.build_segmentor(dict(
            type='DDP', timesteps=c['K'], randsteps=c['r'], bit_scale=0.01, accumulation=True, diffusion='ddim',
            decode_head=dict(type='FCNHeadWithTime', num_convs=c['num_convs'], concat_input=False, dilation=1, in_channels=256,
                             channels=256, num_classes=c['Kc'], in_index=0, norm_cfg=dict(type='BN'))))
        model.load_state_dict(synthetic.make_fcn_segmentor_state_dict(c['num_convs'], c['Kc'], True, False, seed=31), strict=True)
        _FCN_MODELS[key] = model.to(dev).eval()
    model = _FCN_MODELS[key]
    return guard(FcnSamplerEngine(model.hot_path_state_dict(), model.decode_head, h=c['h'], w=c['w'], batch=batch or c['B'],
                                  randsteps=c['r'], timesteps=c['K'], num_classes=c['Kc'], bit_scale=0.01, accumulation=True,
                                  sampler=sampler or c['sampler'], device=dev, seeded_noise=seeded, record_steps=record_steps))


def _x(c, dev):
    return S.inputs(dict(c, sampler='ddim'))[0].to(dev)


def _fcn_x(c, dev):
    g = torch.Generator().manual_seed(77)
    return torch.randn((c['B'], 256, c['h'], c['w']), generator=g).to(dev)


_RUNS = {}


def _run(name, dev):
    """one seeded call of the case (image_base 5, call 2), computed once per process: out, noise, engine, x"""
    if name not in _RUNS:
        if name in U.FCN_CASES:
            c = U.FCN_CASES[name]
            eng, x = _fcn_engine(c, dev, True), _fcn_x(c, dev)
        else:
            c, flags = U.CASES[name]
            eng, x = _engine(c, dev, True, **flags), _x(c, dev)
        with pytest.raises(_lib.DdpError, match='sample'):
            eng.last_noise()
        out = eng.sample(x, seed=SEED, image_base=5, call=2)
        torch.cuda.synchronize()
        assert_guards(eng, name)
        _RUNS[name] = dict(out=out.cpu(), noise=eng.last_noise().clone(), eng=eng, x=x, c=c)
    return _RUNS[name]


ALL = sorted(U.CASES) + sorted(U.FCN_CASES)


def _case(n):
    return U.FCN_CASES[n] if n in U.FCN_CASES else U.CASES[n][0]


DDIM = [n for n in ALL if _case(n).get('sampler', 'ddim') == 'ddim']
_MEASURED = {}


# ---- 1. values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_values_match_the_restatement(dev, name):
    r = _run(name, dev)
    c = r['c']
    cm = 1 if c.get('task') == 'depth' else 256
    got = r['noise'].cpu().numpy()
    assert got.shape == (c['B'], c['r'], cm, c['h'], c['w']) and got.dtype == np.float32
    per = c['r'] * cm * c['h'] * c['w']
    ref, rad = U.noise_ref(SEED, 5, 0, 2, c['B'], per)
    err = np.abs(got.reshape(c['B'], per).astype(np.float64) - ref) / np.maximum(1.0, rad)
    worst = err.max() / 2.0 ** -23
    _MEASURED[name] = worst
    print(f'SEEDED-NOISE values {name}: worst |gpu - ref| / max(1, rad) = {worst:.3f} x 2^-23 (bound 8), over all cases so far '
          f'{max(_MEASURED.values()):.3f}')
    assert np.isfinite(got).all() and err.max() <= U.BOUND_UNIT


# ---- 2. the loop consumes what was generated ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DDIM)
def test_seeded_call_equals_unseeded_call_fed_the_generated_noise(dev, name):
    r = _run(name, dev)
    if name in U.FCN_CASES:
        plain = _fcn_engine(r['c'], dev, False)
    else:
        plain = _engine(r['c'], dev, False, **U.CASES[name][1])
    out = plain.sample(r['x'], r['noise'].clone())
    torch.cuda.synchronize()
    assert_guards(plain, name)
    assert torch.equal(out.cpu(), r['out'])
    with pytest.raises(_lib.DdpError, match='seed'):
        r['eng'].sample(r['x'], r['noise'])                       # noise= on a seeded engine
    with pytest.raises(_lib.DdpError, match='seeded_noise'):
        plain.sample(r['x'], seed=1)
    with pytest.raises(_lib.DdpError, match='seeded_noise'):
        plain.last_noise()


# ---- 3. token-major writer == NCHW writer, ddpm end to end --------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_ddpm', 'seg_ddpm_f32', 'fcn_ddpm'])
def test_ddpm_equals_unseeded_ddpm_fed_the_rebuilt_step_noise(dev, name):
    r = _run(name, dev)
    c = r['c']
    fcn = name in U.FCN_CASES
    flags = {} if fcn else U.CASES[name][1]
    make = (lambda seeded, **kw: _fcn_engine(c, dev, seeded, **kw)) if fcn else (lambda seeded, **kw: _engine(dict(c, **kw), dev, seeded, **flags))
    ddim = make(True, sampler='ddim')
    adds = [int(s.ddpm_add_noise) for s in r['eng'].steps]
    assert sum(adds) >= 1 and adds[-1] == 0                      # (time_difference = 1: only the steps whose t_next > 0 add noise)
    stack = torch.zeros((c['K'],) + tuple(r['noise'].shape), device=dev)
    for s, add in enumerate(adds):
        if add:
            ddim.sample(r['x'], seed=SEED, image_base=5, call=2, stream_base=1 + s)
            stack[s] = ddim.last_noise()
    ddim.sample(r['x'], seed=SEED, image_base=5, call=2)
    assert torch.equal(ddim.last_noise(), r['noise'])            # the same start noise from either sampler's engine
    plain = make(False)
    out = plain.sample(r['x'], r['noise'].clone(), stack)
    torch.cuda.synchronize()
    assert_guards(plain, name)
    assert torch.equal(out.cpu(), r['out'])
    assert not torch.equal(plain.sample(r['x'], r['noise'].clone(), torch.zeros_like(stack)).cpu(), r['out'])    # the step noise does count


# ---- 4. independence from how the work is cut ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_fused', 'seg_ddpm', 'depth_chain_1x37', 'depth_unfused', 'depth_f32', 'bev_chain', 'bev_f32', 'fcn_ddim'])
def test_batched_call_equals_single_image_calls(dev, name):
    r = _run(name, dev)
    c = r['c']
    assert c['B'] == 3
    one = _fcn_engine(c, dev, True, batch=1) if name in U.FCN_CASES else _engine(c, dev, True, batch=1, **U.CASES[name][1])
    for b in range(3):
        o = one.sample(r['x'][b:b + 1].clone(), seed=SEED, image_base=5 + b, call=2).cpu()
        assert_guards(one, name)
        assert torch.equal(one.last_noise()[0], r['noise'][b]), f'{name}: noise of image {b}'
        assert torch.equal(o[0], r['out'][b]), f'{name}: output of image {b}'


@pytest.mark.parametrize('name', ['seg_fused', 'depth_r2', 'bev_chain_r2'])
def test_key_words_change_the_noise(dev, name):
    r = _run(name, dev)
    eng, base = r['eng'], r['noise']
    for kw in (dict(seed=SEED, image_base=5, call=3), dict(seed=SEED + 1, image_base=5, call=2), dict(seed=SEED + (1 << 32), image_base=5, call=2),
               dict(seed=SEED, image_base=6, call=2), dict(seed=SEED, image_base=5, call=2, stream_base=1)):
        eng.sample(r['x'], **kw)
        n = eng.last_noise()
        same = float((n == base).float().mean())
        assert not torch.equal(n, base) and same < 0.01, (kw, same)
    eng.sample(r['x'], seed=SEED, image_base=5, call=2)
    assert torch.equal(eng.last_noise(), base)                   # and the same key gives the same noise again
    if r['c']['B'] > 1:                                             # image_base 6 is image_base 5 shifted by one image
        eng.sample(r['x'], seed=SEED, image_base=6, call=2)
        assert torch.equal(eng.last_noise()[:-1], base[1:])
    assert_guards(eng, name)


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_fused', 'seg_ddpm', 'depth_chain', 'bev_chain'])
def test_graph_replay_picks_up_a_new_key(dev, name):
    c, flags = U.CASES[name]
    x = _x(c, dev)
    eng = _engine(c, dev, True, **flags)
    want_a = eng.sample(x, seed=11, image_base=1, call=0).clone()
    want_b = eng.sample(x, seed=U.SEED_B, image_base=1, call=0).clone()
    noise_b = eng.last_noise().clone()
    assert not torch.equal(want_a, want_b)
    graph = eng.capture(x, seed=11, image_base=1)
    out = graph.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    out = graph.replay(seed=U.SEED_B).clone()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b) and torch.equal(eng.last_noise(), noise_b)
    out = graph.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b)
    with pytest.raises(_lib.DdpError, match='seed'):
        graph.replay(noise=noise_b)
    assert_guards(eng, name)


# ---- 6. / 7. fence and launch counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(U.PATHS))
def test_launch_records_with_the_flag_clear_and_set(dev, name):
    c, flags = U.CASES[name]
    want = S.expected_launches(U.PATHS[name], c['K'], c['L'])
    r = _run(name, dev)
    plain = _engine(c, dev, False, **flags)
    got = launch_counts(plain, r['x'], r['noise'].clone())
    assert_guards(plain, name)
    assert {t: got[t] for t in want} == want and got[0] == 0, (name, got)
    eng = r['eng']
    eng.prepare()
    lib, ms, n = eng.lib, _lib.C.c_float(0), _lib.C.c_int(0)
    _lib.check(lib.ddp_profile_begin(255), lib)
    try:
        eng.sample(r['x'], seed=SEED, image_base=5, call=2)
        torch.cuda.synchronize()
    finally:
        rc = lib.ddp_profile_end(_lib.C.byref(ms), _lib.C.byref(n))
    _lib.check(rc, lib)
    counts = {}
    for tag in range(11):
        _lib.check(lib.ddp_profile_read(tag, _lib.C.byref(ms), _lib.C.byref(n)), lib)
        counts[tag] = n.value
    assert {t: counts[t] for t in want} == want and counts[0] == 1, (name, counts)      # exactly one launch more: k_noise_fill_nchw


@pytest.mark.parametrize('name', ['seg_ddpm', 'seg_ddpm_f32', 'fcn_ddpm', 'fcn_ddim'])
def test_ddpm_launch_counts(dev, name):
    """tag 0 (which no launch of the samplers otherwise carries): the start-noise fill once per call, and the token-major fill once
    per noise-adding step - where the unseeded call runs the (untagged) NCHW -> token-major transpose"""
    r = _run(name, dev)
    eng, lib = r['eng'], r['eng'].lib
    ms, n = _lib.C.c_float(0), _lib.C.c_int(0)
    torch.cuda.synchronize()
    _lib.check(lib.ddp_profile_begin(0), lib)
    try:
        eng.sample(r['x'], seed=SEED, image_base=5, call=2)
        torch.cuda.synchronize()
    finally:
        rc = lib.ddp_profile_end(_lib.C.byref(ms), _lib.C.byref(n))
    _lib.check(rc, lib)
    adds = sum(int(s.ddpm_add_noise) for s in eng.steps) if r['c']['sampler'] == 'ddpm' else 0
    assert n.value == 1 + adds, (name, n.value, adds)


def test_record_and_noise_buffers_coexist(dev):
    """both flags: the record and the map stay the last of the workspace (ddp_x0_trace's base), the noise buffer in front of them"""
    from ddp_amd.engine import step_record_sizes
    c, flags = U.CASES['seg_r2_cx96']
    r = _run('seg_r2_cx96', dev)
    both = _engine(c, dev, True, record_steps=True)
    rec_only = _engine(c, dev, False, record_steps=True)
    out = both.sample(r['x'], seed=SEED, image_base=5, call=2)
    want = rec_only.sample(r['x'], r['noise'].clone())
    torch.cuda.synchronize()
    assert_guards(both, 'both')
    assert torch.equal(out.cpu(), r['out']) and torch.equal(want.cpu(), r['out'])
    assert torch.equal(both.last_noise(), r['noise'])
    assert torch.equal(both.step_record(), rec_only.step_record()) and torch.equal(both.step_disagreement(), rec_only.step_disagreement())
    rec, smap = step_record_sizes(both.cfg)
    end = both._workspace_bytes()
    assert both._step_base() == end - U.round256(smap) - U.round256(rec)
    assert both.last_noise().data_ptr() - both.workspace.data_ptr() == both._step_base() - U.noise_bytes(c)


# ---- 8. plugin surface ----------------------------------------------------------------------------------------------------------
def _seg_plugin(dev, noise_seed, test_cfg=None):
    import ddp_amd
    from ddp_amd.utils import synthetic
    from support import ENCODER, seg_cfg
    cfg = seg_cfg(noise_seed=noise_seed, test_cfg=test_cfg or dict(mode='whole'),
                  decode_head=dict(seg_cfg()['decode_head'], num_classes=20, encoder=dict(ENCODER, num_layers=2)))
    model = ddp_amd.build_segmentor(cfg)
    model.load_state_dict(synthetic.make_state_dict('seg', 20, 2, 256, seed=5), strict=True)      # (20 x 7 x 13 floats per image: 16-byte multiples)
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(123)
    feats = torch.randn((3, 256, 7, 13), generator=g).to(dev)
    model.extract_feat = lambda img: [feats[img[:, 0, 0, 0].long()].contiguous()]      # pixel (0, 0) of an image names its feature map
    return model, feats


def _imgs(idx, dev, hw=(28, 52)):
    img = torch.zeros((len(idx), 3) + hw, device=dev)
    img[:, 0, 0, 0] = torch.tensor(idx, dtype=torch.float32, device=dev)
    return img


def test_plugin_simple_test_batch_equals_single_image_calls(dev):
    model, feats = _seg_plugin(dev, 7)
    metas = [dict(img_shape=(28, 52, 3), ori_shape=(30, 50, 3), flip=False),
             dict(img_shape=(26, 48, 3), ori_shape=(28, 52, 3), flip=True, flip_direction='horizontal'),
             dict(img_shape=(28, 52, 3), ori_shape=(28, 52, 3), flip=False)]
    whole = model.simple_test(_imgs([0, 1, 2], dev), metas, rescale=True, image_base=4)
    for i in range(3):
        one = model.simple_test(_imgs([i], dev), [metas[i]], rescale=True, image_base=4 + i)
        assert np.array_equal(one[0], whole[i]), f'image {i}'
    again = model(img=[_imgs([0, 1, 2], dev)], img_metas=[metas], return_loss=False, image_base=4)
    assert all(np.array_equal(a, b) for a, b in zip(again, whole))
    other = model.simple_test(_imgs([0, 1, 2], dev), metas, rescale=True, image_base=5)
    assert any(not np.array_equal(a, b) for a, b in zip(other, whole))
    seeded = [e for e in model._engine_cache.values() if e.seeded]
    assert seeded and all(e.cfg.flags & _lib.FLAG_SEEDED_NOISE for e in seeded)


def test_plugin_without_a_seed_is_unchanged(dev):
    model, feats = _seg_plugin(dev, None)
    torch.manual_seed(3)
    out = model.ddim_sample(feats, None)
    torch.manual_seed(3)
    noise = torch.randn((3, model.randsteps, 256, 7, 13), device=dev)
    assert torch.equal(out, model.ddim_sample(feats, None, noise=noise))
    assert not any(e.seeded for e in model._engine_cache.values())
    model.noise_seed = 7                                            # an explicit noise= still wins over the seed
    assert torch.equal(out, model.ddim_sample(feats, None, noise=noise))


def test_plugin_aug_test_uses_one_call_value_per_augmentation(dev):
    model, feats = _seg_plugin(dev, 7)
    keys, noises = [], []
    real = model._engine_for

    def spy(*a, **kw):
        eng = real(*a, **kw)
        if not getattr(eng, '_spied', False):
            inner = eng.sample

            def sample(*sa, **skw):
                out = inner(*sa, **skw)
                keys.append(list(eng._key_words))
                noises.append(eng.last_noise().clone())
                return out
            eng.sample, eng._spied = sample, True
        return eng
    model._engine_for = spy
    meta = dict(img_shape=(28, 52, 3), ori_shape=(28, 52, 3), flip=False)
    flip = dict(meta, flip=True, flip_direction='horizontal')
    model.aug_test([_imgs([1], dev), _imgs([1], dev)], [[meta], [flip]], rescale=True, image_base=9)
    assert [k[2] for k in keys] == [9, 9] and [k[4] for k in keys] == [0, 1] and keys[0][:2] == [7, 0]
    assert not torch.equal(noises[0], noises[1]) and float((noises[0] == noises[1]).float().mean()) < 0.01


def test_plugin_depther_and_bev_take_the_seed(dev):
    import ddp_amd
    from ddp_amd.utils import synthetic
    sd = synthetic.make_state_dict('depth', 1, 6, 256, seed=2)
    model = support.depth_model(dict(timesteps=2), sd)
    model.noise_seed = 7
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 256, 5, 9), generator=g).to(dev)
    whole = model.sample(x, image_base=2)
    for i in range(3):
        assert torch.equal(model.sample(x[i:i + 1].contiguous(), image_base=2 + i)[0], whole[i])
    assert not torch.equal(model.sample(x, image_base=2, call=1), whole)
    c = U.CASES['bev_chain'][0]
    bev, head = support.bev_plugin(S.state_dict(c), dev, c['L'], S.bev_scopes(c), bit_scale=c['bit_scale'], timesteps=c['K'],
                                   randsteps=c['r'], feat_channels=c['Cx'], noise_seed=SEED)
    r = _run('bev_chain', dev)
    assert torch.equal(bev.ddim_sample([r['x']], head, image_base=5, call=2).cpu(), r['out'])


def test_sample_sharded_equals_the_slice_of_the_whole_batch(dev):
    from ddp_amd import parallel
    c, flags = U.CASES['seg_fused']
    r = _run('seg_fused', dev)
    for rank, world in ((0, 2), (1, 2), (2, 3)):
        a, b = parallel.shard_range(c['B'], rank, world)
        eng = _engine(c, dev, True, batch=b - a, **flags)
        out = eng.sample(r['x'][a:b].contiguous(), seed=SEED, image_base=5 + a, call=2)
        assert torch.equal(out.cpu(), r['out'][a:b]) and torch.equal(eng.last_noise(), r['noise'][a:b])
    # the function itself (world size 1: the shard is the batch, image_base = 0)
    out, (a, b) = parallel.sample_sharded(lambda n: _engine(c, dev, True, batch=n, **flags), r['x'], seed=SEED, call=2)
    assert (a, b) == (0, 3)
    base0 = _engine(c, dev, True, **flags).sample(r['x'], seed=SEED, image_base=0, call=2)
    assert torch.equal(out, base0)
    with pytest.raises(ValueError, match='seed'):
        parallel.sample_sharded(lambda n: _engine(c, dev, True, batch=n, **flags), r['x'], r['noise'])
