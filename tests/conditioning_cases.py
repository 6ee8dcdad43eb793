"""The caller-written inputs of DDPEngine, what the host and the GPU test of them share: the rows of ``ddp_amd.engine.CALLER_INPUTS`` as
literals (tests/test_conditioning_host.py runs on them, tests/test_score_prior_host.py ties the engine's table to them), and the four
device checks every row owes its caller, on every task it exists for (tests/test_conditioning_gpu.py):

  1  after construction the view holds the clear value
  2  ``set_*`` writes exactly the given tensor (the class prior: into the first num_classes columns, the others stay 0)
  3  ``set_geometry`` to another size clears it, and so does the way back
  4  ``SampleGraph.replay(<name>=v)`` leaves v in the view and gives the output of ``set_*(v)`` + ``sample()``, bit for bit

on the smallest cases of tests/prior_start_cases.py: seg 7 x 13, depth 5 x 10 with two noise replicas, bev 12 x 20, batch 2, two layers.
The engine is imported where it is used: the literals stand without it."""
import torch

import config_space_cases as S
import prior_start_cases as P

# (public name, constructor kwarg, flag, caller-written region, tasks, the words of view / set / clear on a flag-clear engine, of the
# FCN-head loop), in the order of caller_regions
ROWS = [('score_prior', 'score_prior', 'FLAG_SCORE_PRIOR', 'sprior_map', ('seg',), 'the score prior needs an engine built with score_prior=True',
         'score_prior is built for ddp_sample only (DDP_FLAG_SCORE_PRIOR): the FCN-head loop takes no score prior'),
        ('class_prior', 'class_prior', 'FLAG_CLASS_PRIOR', 'cprior_table', ('seg',), 'the class prior needs an engine built with class_prior=True',
         'class_prior is built for ddp_sample only (DDP_FLAG_CLASS_PRIOR): the FCN-head loop takes no class prior'),
        ('prior', 'prior_start', 'FLAG_PRIOR_START', 'prior_map', ('seg', 'depth', 'bev'),
         'the prior map and last_start() need an engine built with prior_start=True',
         'prior_start is built for ddp_sample only (DDP_FLAG_PRIOR_START): the FCN-head loop starts from noise'),
        ('hints', 'x0_hints', 'FLAG_X0_HINTS', 'hint_map', ('seg', 'depth'), 'hints need an engine built with x0_hints=True',
         'x0_hints is built for ddp_sample only (DDP_FLAG_X0_HINTS): the FCN-head loop takes no hints')]
PAIRS = [(row[0], task) for row in ROWS for task in row[4]]            # every row on every task it exists for

CASE = {'seg': 'seg_kc19_7x13', 'depth': 'depth_5x10_r2', 'bev': 'bev_kc8_r1'}


def _value(name, c, which, h=None, w=None):
    """a seeded value of the input for the case (``which``: two different ones), at another map size if given"""
    c = dict(c, h=c['h'] if h is None else h, w=c['w'] if w is None else w)
    g = torch.Generator().manual_seed(c['seed'] + 50 + which)
    B, K, h, w = c['B'], c['Kc'], c['h'], c['w']
    if name == 'prior':
        return P.prior(c, which)
    if name == 'hints' and c['task'] == 'seg':                          # classes, about half the pixels free
        v = torch.randint(0, K, (B, h, w), generator=g)
        return torch.where(torch.rand((B, h, w), generator=g) < 0.5, torch.full_like(v, 255), v).to(torch.uint8)
    if name == 'hints':                                                 # metric depth, about half the pixels free, one NaN
        v = torch.rand((B, h, w), generator=g) * (c['max_depth'] - 1.0) + 1.0
        v = torch.where(torch.rand((B, h, w), generator=g) < 0.5, torch.zeros_like(v), v)
        v.view(-1)[which] = float('nan')
        return v
    v = torch.randn((B, K) if name == 'class_prior' else (B, K, h, w), generator=g)
    v.view(-1)[3 + which] = float('-inf')
    return v


def _bits(t):
    return t.cpu().contiguous().numpy().tobytes()


def check(dev, name, task):
    """the four properties for the input ``name`` on ``task``"""
    from ddp_amd.engine import CALLER_INPUTS, DDPEngine
    row = {r.name: r for r in CALLER_INPUTS}[name]
    c = P.CASES[CASE[task]]
    B, K, h, w = c['B'], c['Kc'], c['h'], c['w']
    x, noise, sn = (None if t is None else t.to(dev) for t in S.inputs(c))
    flags = dict({row.kwarg: True}, **({'t_start': c['t_start']} if name == 'prior' else {}))       # (t_start = 1 drowns a prior in noise)
    eng = DDPEngine(P.state_dict(c), task, device=dev, **flags, **S.engine_kwargs(c))
    view, set_, clear = (getattr(eng, m) for m in (name + '_view', 'set_' + name, 'clear_' + name))
    blank = 255 if view().dtype == torch.uint8 else 0

    def written():                                                      # what set_* wrote, and nothing beside it
        if name != 'class_prior':
            return view()
        assert tuple(view().shape) == (B, 256) and bool((view()[:, K:] == 0).all())
        return view()[:, :K]
    # 1
    assert view().dtype == row.dtypes[eng.cfg.task] and tuple(view().shape) == row.shape(eng.cfg) and bool((view() == blank).all())
    # 2
    v1, v2 = _value(name, c, 0), _value(name, c, 1)
    assert _bits(v1) != _bits(v2)
    set_(v1.to(dev))
    assert written().dtype == v1.dtype and _bits(written()) == _bits(v1)
    # 3
    eng.set_geometry(batch=B, h=h + 1, w=w)
    assert tuple(view().shape) == row.shape(eng.cfg) and eng.geometry() == (B, h + 1, w) and bool((view() == blank).all())
    other = _value(name, c, 0, h=h + 1)
    set_(other.to(dev))
    assert _bits(written()) == _bits(other)
    eng.set_geometry(batch=B, h=h, w=w)
    assert tuple(view().shape) == row.shape(eng.cfg) and bool((view() == blank).all())
    # 4
    want = {}
    for i, v in enumerate((v1, v2)):
        set_(v.to(dev))
        want[i] = eng.sample(x, noise, sn).clone()
    assert not torch.equal(want[0], want[1])
    clear()
    graph = eng.capture(x, noise, sn)
    for i, v in ((0, v1), (1, v2), (0, v1)):
        out = graph.replay(**{name: v.to(dev)})
        torch.cuda.synchronize()
        assert _bits(written()) == _bits(v), (task, i)
        assert torch.equal(out, want[i]), (task, i)
    out = graph.replay()                                                # nothing given: what the view holds
    torch.cuda.synchronize()
    assert _bits(written()) == _bits(v1) and torch.equal(out, want[0]), task
