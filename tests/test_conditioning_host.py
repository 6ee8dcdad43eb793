"""The caller's conditioning inputs (x0 hints, prior start with t_start, class prior, score prior) on the host, no device: what every
entry point of the seg and depth plugin classes hands to the next member down its call chain, the frame-bound refusals of slide
inference and test-time augmentation with their precedence, and the engine's words for a flag-clear engine and for the FCN-head
loop.  The expectations are literals: a member that stops forwarding a keyword, forwards one nobody gave, or refuses in another
order fails here.  (On the device: tests/test_conditioning_gpu.py.)"""
import pytest
import torch

import conditioning_cases as CC
import config_space_cases as S
from ddp_amd import _lib, engine
from ddp_amd.depther.ddp import DDP as DepthDDP
from ddp_amd.engine import DDPEngine, FcnSamplerEngine, caller_regions
from ddp_amd.segmentors.ddp import DDP as SegDDP

IMG = torch.zeros(1, 3, 16, 16)
IMG2 = torch.zeros(1, 3, 16, 16)
FEAT = torch.zeros(1, 256, 4, 4)
META = [dict(img_shape=(16, 16, 3), ori_shape=(16, 16, 3), flip=False)]
META2 = [dict(img_shape=(16, 16, 3), ori_shape=(16, 16, 3), flip=True, flip_direction='horizontal')]
HINTS = torch.full((1, 16, 16), 255, dtype=torch.uint8)
PRIOR = torch.zeros(1, 16, 16, dtype=torch.uint8)
CP = torch.zeros(1, 5)
SP = torch.zeros(1, 5, 4, 4)

# what the caller gives -> what travels down the chain, as far as the member called takes it
GIVEN = {'nothing': {}, 'hints': dict(hints=HINTS), 'prior': dict(prior=PRIOR), 'prior_t': dict(prior=PRIOR, t_start=0.5),
         't_start': dict(t_start=0.5), 'class_prior': dict(class_prior=CP), 'score_prior': dict(score_prior=SP),
         'on_device': dict(on_device=True)}
SENT = {'nothing': {}, 'hints': {'hints': HINTS}, 'prior': {'prior': PRIOR, 't_start': None}, 'prior_t': {'prior': PRIOR, 't_start': 0.5},
        't_start': {'prior': None, 't_start': 0.5}, 'class_prior': {'class_prior': CP}, 'score_prior': {'score_prior': SP},
        'on_device': {'on_device': True}}
ALL = tuple(GIVEN)
FRAMED = ('hints', 'prior', 'prior_t', 't_start')          # in the frame of one image: no slide windows, no augmentations
SEEDS = (None, 7)


def _same(a, b):
    """equal structures; tensors by identity (nothing on the way may copy or convert what the caller gave)"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return a is b
    if isinstance(a, dict):
        return isinstance(b, dict) and list(sorted(a)) == list(sorted(b)) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


class Recorder:
    def __init__(self, ret):
        self.calls, self.ret = [], ret

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.ret()


def _check(rec, *want):
    assert len(rec.calls) == len(want), rec.calls
    for (args, kwargs), (wargs, wkwargs) in zip(rec.calls, want):
        assert _same(args, wargs), (args, wargs)
        assert _same(kwargs, wkwargs), (kwargs, wkwargs)


def _seg(mode, seed, member, ret, diffusion='ddim'):
    """a seg DDP nobody constructed, its next member down the chain replaced by a recorder"""
    m = object.__new__(SegDDP)
    m.noise_seed, m.diffusion, m.num_classes, m.align_corners = seed, diffusion, 5, False
    m.test_cfg = dict(mode=mode, crop_size=(8, 8), stride=(8, 8))
    m.extract_feat = lambda img: [FEAT]
    rec = Recorder(ret)
    setattr(m, member, rec)
    return m, rec


def _depth(seed, member, ret):
    m = object.__new__(DepthDDP)
    m.noise_seed, m.test_cfg = seed, dict(mode='whole')
    m.extract_feat = lambda img: [FEAT]
    m._post = lambda maps, flips, size: torch.zeros(1, 1, 16, 16)
    rec = Recorder(ret)
    setattr(m, member, rec)
    return m, rec


def _scores():
    return torch.zeros(1, 5, 4, 4)


def _probs():
    return torch.zeros(1, 5, 16, 16)


def _classes():
    return torch.zeros(1, 16, 16, dtype=torch.uint8)


def _depth_map():
    return torch.zeros(1, 1, 16, 16)


@pytest.fixture
def epilogues(monkeypatch):
    """the fused epilogues are device code: stand-ins of the right shape"""
    monkeypatch.setattr(engine, 'seg_postprocess', lambda out, *a, **k: torch.zeros(out.shape[0], 16, 16, dtype=torch.uint8))
    monkeypatch.setattr(engine, 'seg_aug_postprocess', lambda scores, *a, **k: torch.zeros(scores[0].shape[0], 16, 16, dtype=torch.uint8))


def _sent(case, takes, seed, seed_kw):
    """the literal of the case, cut to what the member takes, with the seed's keywords of this hop"""
    kw = dict(SENT[case]) if case in takes else {}
    if seed is not None:
        kw.update(seed_kw)
    return kw


# ---- seg ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ALL)
def test_seg_forward(case, seed):
    seedkw = {} if seed is None else dict(image_base=9)
    for img, metas in (([IMG], [META]), (IMG, META)):                       # the one-element augmentation lists, or bare
        m, rec = _seg('whole', seed, 'simple_test', list)
        m.forward(img, metas, **seedkw, **GIVEN[case])
        _check(rec, ((IMG, META, True), _sent(case, ALL, seed, {'image_base': 9})))
    m, rec = _seg('whole', seed, 'aug_test', list)
    m.forward([IMG, IMG2], [META, META2], rescale=False, **seedkw, **GIVEN[case])
    _check(rec, (([IMG, IMG2], [META, META2], False), _sent(case, ALL, seed, {'image_base': 9})))


@pytest.mark.parametrize('diffusion', ('ddim', 'ddpm'))
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ALL)
def test_seg_simple_test_whole(case, seed, diffusion, epilogues):
    m, rec = _seg('whole', seed, diffusion + '_sample', _scores, diffusion)
    out = m.simple_test(IMG, META, **({} if seed is None else dict(image_base=9)), **GIVEN[case])
    _check(rec, ((FEAT, META), _sent(case, ALL[:-1], seed, {'image_base': 9, 'call': 0})))       # (on_device stays here: _deliver)
    assert len(out) == 1 and (torch.is_tensor(out[0]) if case == 'on_device' else out[0].dtype == 'int64')


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior', 'on_device'))
def test_seg_simple_test_slide(case, seed):
    m, rec = _seg('slide', seed, '_slide', _classes)
    m.simple_test(IMG, META, **({} if seed is None else dict(image_base=9)), **GIVEN[case])
    _check(rec, ((IMG, META, True, 'seg', None), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 0})))


@pytest.mark.parametrize('diffusion', ('ddim', 'ddpm'))
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior', 'on_device'))
def test_seg_aug_test_whole(case, seed, diffusion, epilogues):
    m, rec = _seg('whole', seed, diffusion + '_sample', _scores, diffusion)
    m.aug_test([IMG, IMG2], [META, META2], **({} if seed is None else dict(image_base=9)), **GIVEN[case])
    _check(rec, ((FEAT, META), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 0})),
           ((FEAT, META2), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 1})))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior', 'on_device'))
def test_seg_aug_test_slide(case, seed):
    m, rec = _seg('slide', seed, 'inference', _probs)
    m.aug_test([IMG, IMG2], [META, META2], **({} if seed is None else dict(image_base=9)), **GIVEN[case])
    _check(rec, ((IMG, META, True), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 0})),
           ((IMG2, META2, True), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 65536})))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior'))
def test_seg_inference(case, seed):
    seedkw = {} if seed is None else dict(image_base=9, call=3)
    m, rec = _seg('whole', seed, 'whole_inference', _probs)
    m.inference(IMG, META, True, **seedkw, **GIVEN[case])
    _check(rec, ((IMG, META, True), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 3})))
    m, rec = _seg('slide', seed, '_slide', _probs)
    m.inference(IMG, META2, False, **seedkw, **GIVEN[case])
    _check(rec, ((IMG, META2, False, 'prob', 'horizontal'), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 3})))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior', 'score_prior'))
def test_seg_whole_inference_and_encode_decode(case, seed):
    seedkw = {} if seed is None else dict(image_base=9, call=3)
    m, rec = _seg('whole', seed, 'encode_decode', _probs)
    m.whole_inference(IMG, META, False, **seedkw, **GIVEN[case])
    _check(rec, ((IMG, META), _sent(case, ('class_prior', 'score_prior'), seed, {'image_base': 9, 'call': 3})))
    for diffusion in ('ddim', 'ddpm'):
        m, rec = _seg('whole', seed, diffusion + '_sample', _scores, diffusion)
        assert tuple(m.encode_decode(IMG, META, **seedkw, **GIVEN[case]).shape) == (1, 5, 16, 16)
        _check(rec, ((FEAT, META), _sent(case, ('class_prior', 'score_prior'), seed, {'image_base': 9, 'call': 3})))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', ('nothing', 'class_prior'))
def test_seg_slide_inference_and_sample(case, seed):
    seedkw = {} if seed is None else dict(image_base=9, call=3)
    m, rec = _seg('slide', seed, '_slide', _probs)
    m.slide_inference(IMG, META, False, **seedkw, **GIVEN[case])
    _check(rec, ((IMG, META, False, 'scores'), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 3})))
    for diffusion in ('ddim', 'ddpm'):
        m, rec = _seg('whole', seed, diffusion + '_sample', _scores, diffusion)
        m._sample(FEAT, META, **seedkw, **GIVEN[case])
        _check(rec, ((FEAT, META), _sent(case, ('class_prior',), seed, {'image_base': 9, 'call': 3})))


@pytest.mark.parametrize('seed', SEEDS)
def test_seg_slide_windows(seed, monkeypatch):
    """_slide: four 8 x 8 windows of the 16 x 16 image in one chunk; the class prior's rows tiled window-major, the chunk's index added
    to ``call``"""
    monkeypatch.setattr(engine, 'seg_slide_postprocess', lambda scores, *a, **k: scores)
    feat4 = torch.zeros(4, 256, 2, 2)
    for case in ('nothing', 'class_prior'):
        m, rec = _seg('slide', seed, '_sample', lambda: torch.zeros(4, 5, 2, 2))
        m.extract_feat = lambda img: [feat4]
        m._slide(IMG, META, False, 'scores', **({} if seed is None else dict(image_base=9, call=3)), **GIVEN[case])
        (args, kwargs), = rec.calls
        assert _same(args, (feat4, META))
        assert sorted(kwargs) == sorted(({'class_prior'} if case == 'class_prior' else set()) | (set() if seed is None else {'image_base', 'call'}))
        if seed is not None:
            assert (kwargs['image_base'], kwargs['call']) == (9, 3)
        if case == 'class_prior':
            assert torch.equal(kwargs['class_prior'], CP.repeat(4, 1)) and kwargs['class_prior'].dtype == torch.float32


# ---- depth --------------------------------------------------------------------------------------------------------------------------
DEPTH_ALL = ('nothing', 'hints', 'prior', 'prior_t', 't_start', 'on_device')


@pytest.mark.parametrize('case', DEPTH_ALL)
def test_depth_forward_test_hands_its_keywords_through(case):
    m, rec = _depth(None, 'simple_test', list)
    m.forward([IMG], [META], return_loss=False, **GIVEN[case])
    _check(rec, ((IMG, META), dict(GIVEN[case])))
    m, rec = _depth(None, 'aug_test', list)
    m.forward_test([IMG, IMG2], [META, META2], **GIVEN[case])
    _check(rec, (([IMG, IMG2], [META, META2]), dict(GIVEN[case])))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('case', DEPTH_ALL)
def test_depth_simple_test_inference_low_res(case, seed):
    m, rec = _depth(seed, 'inference', _depth_map)
    out = m.simple_test(IMG, META, **({} if seed is None else dict(image_base=9)), **GIVEN[case])
    _check(rec, ((IMG, META, True), _sent(case, DEPTH_ALL[:-1], seed, {'image_base': 9, 'call': 0})))
    assert len(out) == 1 and torch.is_tensor(out[0]) == (case == 'on_device')
    if case == 'on_device':
        return
    seedkw = {} if seed is None else dict(image_base=9, call=3)
    m, rec = _depth(seed, '_low_res', _depth_map)
    m.inference(IMG, META, True, **seedkw, **GIVEN[case])
    _check(rec, ((IMG, META), _sent(case, DEPTH_ALL[:-1], seed, {'image_base': 9, 'call': 3})))
    m, rec = _depth(seed, 'sample', _depth_map)
    m._low_res(IMG, META, **seedkw, **GIVEN[case])
    _check(rec, ((FEAT, META), _sent(case, DEPTH_ALL[:-1], seed, {'image_base': 9, 'call': 3})))


@pytest.mark.parametrize('seed', SEEDS)
def test_depth_encode_decode_whole_inference_aug_test(seed):
    seedkw = {} if seed is None else dict(image_base=9, call=3)
    sent = {} if seed is None else {'image_base': 9, 'call': 3}
    m, rec = _depth(seed, '_low_res', _depth_map)
    m.encode_decode(IMG, META, True, **seedkw)
    _check(rec, ((IMG, META), sent))
    m, rec = _depth(seed, 'encode_decode', _depth_map)
    m.whole_inference(IMG, META, True, **seedkw)
    _check(rec, ((IMG, META, True), sent))
    for case in ('nothing', 'on_device'):
        m, rec = _depth(seed, '_low_res', _depth_map)
        out = m.aug_test([IMG, IMG2], [META, META2], **({} if seed is None else dict(image_base=9)), **GIVEN[case])
        _check(rec, ((IMG, META), {} if seed is None else {'image_base': 9, 'call': 0}),
               ((IMG2, META2), {} if seed is None else {'image_base': 9, 'call': 1}))
        assert torch.is_tensor(out[0]) == (case == 'on_device')


# ---- the frame-bound refusals -------------------------------------------------------------------------------------------------------
SLIDE = {'score_prior': 'score_prior is not built for slide inference (one score prior map per sampler call, not per window)',
         'prior': 'prior / t_start are not built for slide inference (one prior map per sampler call, not per window)',
         'hints': 'hints are not built for slide inference (one hint map per sampler call, not per window)'}
AUG = {'score_prior': 'score_prior is not built for aug_test (every augmentation has its own frame)',
       'prior': 'prior / t_start are not built for aug_test (every augmentation has its own frame)',
       'hints': 'hints are not built for aug_test (every augmentation has its own frame)'}
# (what is given, whose message it raises): each alone, then two at a time - slide inference: score prior, prior / t_start, hints;
# aug_test: score prior, hints, prior / t_start
ALONE = [('score_prior', 'score_prior'), ('prior', 'prior'), ('prior_t', 'prior'), ('t_start', 'prior'), ('hints', 'hints')]
SLIDE_PAIRS = [(('score_prior', 'prior_t'), 'score_prior'), (('score_prior', 'hints'), 'score_prior'), (('t_start', 'hints'), 'prior'),
               (('prior_t', 'hints'), 'prior')]
AUG_PAIRS = [(('score_prior', 'prior_t'), 'score_prior'), (('score_prior', 'hints'), 'score_prior'), (('t_start', 'hints'), 'hints'),
             (('prior_t', 'hints'), 'hints')]


def _raises(message, call, *cases):
    kw = {}
    for c in cases:
        kw.update(GIVEN[c])
    with pytest.raises(ValueError) as e:
        call(**kw)
    assert str(e.value) == message


@pytest.mark.parametrize('cases,who', [((c,), w) for c, w in ALONE] + SLIDE_PAIRS)
def test_slide_refusals(cases, who):
    m, rec = _seg('slide', None, '_slide', _classes)
    _raises(SLIDE[who], lambda **kw: m.slide_inference(IMG, META, False, **kw), *cases)
    _raises(SLIDE[who], lambda **kw: m.simple_test(IMG, META, **kw), *cases)
    _raises(SLIDE[who], lambda **kw: m.forward([IMG], [META], **kw), *cases)
    # (nothing else was looked at: a model nobody set up raises the same)
    _raises(SLIDE[who], lambda **kw: SegDDP.slide_inference(object.__new__(SegDDP), None, None, False, **kw), *cases)
    assert rec.calls == []


@pytest.mark.parametrize('cases,who', [((c,), w) for c, w in ALONE] + AUG_PAIRS)
def test_aug_test_refusals(cases, who):
    for mode in ('whole', 'slide'):
        m, rec = _seg(mode, None, 'inference', _probs)
        _raises(AUG[who], lambda **kw: m.aug_test([IMG, IMG2], [META, META2], **kw), *cases)
        _raises(AUG[who], lambda **kw: m.forward([IMG, IMG2], [META, META2], **kw), *cases)
        assert rec.calls == []
    _raises(AUG[who], lambda **kw: SegDDP.aug_test(object.__new__(SegDDP), [None, None], [None, None], **kw), *cases)
    if 'score_prior' not in cases:
        m, rec = _depth(None, '_low_res', _depth_map)
        _raises(AUG[who], lambda **kw: m.aug_test([IMG, IMG2], [META, META2], **kw), *cases)
        _raises(AUG[who], lambda **kw: m.forward([IMG, IMG2], [META, META2], return_loss=False, **kw), *cases)
        _raises(AUG[who], lambda **kw: DepthDDP.aug_test(object.__new__(DepthDDP), [None, None], [None, None], **kw), *cases)
        assert rec.calls == []


# ---- the engine's rows --------------------------------------------------------------------------------------------------------------
# the literal rows, shared with the GPU test and tied to ``engine.CALLER_INPUTS`` by tests/test_score_prior_host.py::test_engine_surface
ROWS, PAIRS = CC.ROWS, CC.PAIRS
TASK_CASE = {'seg': 'seg_ddpm_acc', 'depth': 'depth_9x11_L2_r2', 'bev': 'bev_kc8_r2'}


@pytest.mark.parametrize('name,task', PAIRS)
def test_engine_rows(name, task):
    _, kwarg, flag, region, tasks, needs, _ = {r[0]: r for r in ROWS}[name]
    cfg = S.make_cfg(S.CASES[TASK_CASE[task]])
    total = 1 << 24                                        # (any size: the regions are carved back from the end)
    assert region not in caller_regions(cfg, total)
    eng = object.__new__(DDPEngine)
    eng.cfg = cfg
    for call in (getattr(eng, name + '_view'), getattr(eng, 'clear_' + name), lambda: getattr(eng, 'set_' + name)(torch.zeros(1))):
        with pytest.raises(_lib.DdpError) as e:
            call()
        assert str(e.value) == needs
    assert getattr(eng, 'clear_' + name)(_if_any=True) is None
    cfg.flags |= getattr(_lib, flag)
    regions = caller_regions(cfg, total)
    assert region in regions and list(regions)[-1] == region and sum(regions[region]) <= total


def test_engine_region_order():
    """all four flags: the caller-written regions in workspace order, each behind the rows the library derives from it"""
    cfg = S.make_cfg(S.CASES['seg_ddpm_acc'])
    for row in ROWS:
        cfg.flags |= getattr(_lib, row[2])
    assert list(caller_regions(cfg, 1 << 24)) == ['sprior_rows', 'sprior_map', 'cprior_rows', 'cprior_table', 'prior_start', 'prior_map',
                                                  'hint_rows', 'hint_map']


@pytest.mark.parametrize('first', range(len(ROWS)))
def test_fcn_loop_refusals(first):
    """each keyword alone; with every later row's keyword set as well, the earlier row's message wins"""
    message = ROWS[first][6]
    for given in ([ROWS[first]], ROWS[first:]):
        with pytest.raises(ValueError) as e:
            FcnSamplerEngine({}, None, h=4, w=4, **{r[1]: True for r in given})
        assert str(e.value) == message
