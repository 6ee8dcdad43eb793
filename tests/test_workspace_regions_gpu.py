"""Every caller-visible buffer of the workspace tail in ONE engine, at the smallest shape where every rounding matters.  Needs an
MI355X: ``pytest -m gpu``.  (CPU companion: tests/test_workspace_regions_host.py.)

B = 2, r = 2, h = 3, w = 5: the map bytes (30 / 120), the row bytes (60 / 240) and B N = 30 are no multiples of 256, and M0 = 60 != B N.
K = 2, L = 1, bf16x3.  seg (19 classes): record_steps, seeded_noise, x0_hints, prior_start and class_prior; depth: the same without the
class prior (seg only).  Each caller-written view is filled with a byte pattern of its own; after ``sample()`` the three still hold
theirs, the library-written buffers have the documented shapes, and all views lie inside the workspace, pairwise disjoint.  The
workspace is NaN-patterned with 4 KiB guards at both ends."""
import pytest
import torch

import config_space_cases as S
import support
from ddp_amd import _lib

pytestmark = pytest.mark.gpu

CASES = S.REGION_CASES
# one byte per caller-written view.  seg: 0xA5 / 0x5A are >= num_classes (a free pixel / the ignore row); depth: 0x41414141 = 12.08 and
# 0x40404040 = 3.004 are depths inside the range; 0x3C3C3C3C = 0.0115 is an ordinary class prior
FILL = dict(hints={'seg': 0xA5, 'depth': 0x41}, prior={'seg': 0x5A, 'depth': 0x40}, class_prior={'seg': 0x3C})


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


@pytest.mark.parametrize('task', ['seg', 'depth'])
def test_all_caller_regions_in_one_engine(task):
    from ddp_amd.engine import DDPEngine, step_disagreement_view, step_record_view
    dev = torch.device('cuda:0')
    c = CASES[task]
    seg = task == 'seg'
    eng = DDPEngine(S.state_dict(c), task, device=dev, gemm='bf16x3', record_steps=True, seeded_noise=True, x0_hints=True,
                    prior_start=True, class_prior=seg, **S.engine_kwargs(c))
    want = _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE | _lib.FLAG_X0_HINTS | _lib.FLAG_PRIOR_START
    want |= _lib.FLAG_CLASS_PRIOR if seg else 0
    assert eng.cfg.flags & want == want
    n = support.guard(eng).workspace.numel()
    written = dict(hints=eng.hints_view(), prior=eng.prior_view())
    if seg:
        written['class_prior'] = eng.class_prior_view()
    for k, v in written.items():
        _bytes(v).fill_(FILL[k][task])
    x = S.inputs(c)[0].to(dev)
    out = eng.sample(x, seed=2024)
    torch.cuda.synchronize()
    assert support.guards_ok(eng), 'workspace guards overwritten'
    assert bool(torch.isfinite(out).all())
    for k, v in written.items():
        assert bool((_bytes(v) == FILL[k][task]).all()), f'{task}: the {k} view lost its pattern'
    B, r, K, h, w = c['B'], c['r'], c['K'], c['h'], c['w']
    rec, dis, start = eng.step_record(), eng.step_disagreement(), eng.last_start()
    assert tuple(rec.shape) == (K, B, r, h, w) and rec.dtype == (torch.uint8 if seg else torch.float32)
    assert tuple(dis.shape) == (B, h, w) and dis.dtype == torch.float32
    assert tuple(start.shape) == (B, r, 256 if seg else 1, h, w) and start.dtype == torch.float32
    assert bool(torch.isfinite(dis).all()) and bool(torch.isfinite(start).all())
    assert int(rec.max()) < c['Kc'] if seg else bool(torch.isfinite(rec).all())
    assert tuple(written['hints'].shape) == tuple(written['prior'].shape) == (B, h, w)
    views = dict(written, start=start, record=step_record_view(eng.workspace, eng._step_base(), eng.cfg),
                 disagreement=step_disagreement_view(eng.workspace, eng._step_base(), eng.cfg))
    lo = eng.workspace.data_ptr()
    spans = sorted((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size(), k) for k, v in views.items())
    assert spans[0][0] >= lo and spans[-1][1] <= lo + n * 4, spans
    for (_, end, a), (begin, _, b) in zip(spans, spans[1:]):
        assert end <= begin, f'{task}: {a} overlaps {b}'
