"""The decoder under hostile activation and weight statistics, against the fp64 oracle.  Needs an MI355X: ``pytest -m gpu``.

Every case of tests/hostile_stats_cases.py (a benign seeded model and input plus one named mutation: feature scale, DC offset,
degenerate rows, LayerNorm affine, FiLM scale = -1, GELU tails, one-hot and tied attention softmax, near-cancelling head rows,
hostile sampler inputs, the depth head, the bev head) runs on every route it names -

  head   ``DDPEngine.head_forward`` against ``O.head_forward_seg`` / ``O.head_forward_depth`` / ``O.head_forward_bev`` (k_layer
         MODE 3 and MODE 0, the gather, k_fold_affine, the head GEMM; bev: the grid resampling and the sigmoid as well)
  step1  ``sample()`` with one step and no accumulation against ``O.ddim_sample_seg`` (MODE 7 from the caller's NCHW planes,
         MODE 0, the fused MODE 6 tail: the product path without feedback)
  tf2    two steps with accumulation, the fp32 oracle's decisions fed to both sides (DDP_FLAG_FORCE_X0): the MODE 4 u chain and
         the softmax accumulation, without the argmax discontinuity

- under five engine variants (the entries of tests/test_hip_parity.py VARIANTS of the same names): the fused layer kernel, the
LayerNorm epilogue of the unfused bf16x3 tile GEMMs, the unfused tail, the SB step head and the exact-product engine with its own
LayerNorm epilogue.

Asserted: outputs finite; err = max|out - r64| / max|r64| <= 4 x max(E_ref(case), E_ref(benign, same shape and route)), E_ref the
same figure of the fp32 oracle (computed here; capped at 1e-5 per case, so no bar exceeds 4e-5 - the suite's REL is 2e-4).  The
factor 4 is the margin of tests/test_hip_parity.py over the reference's own fp64 distance; nothing in the bar is measured on the
code under test.  Degenerate-row cases: the same on the constant / zero tokens alone.  Head family: argmax agreement with the fp32
oracle >= 0.999 wherever its top-2 gap exceeds bar x scale.  ``bf16x3`` and ``bf16x3-unfused-tail`` give the same bits.

Every engine runs on a workspace with 4 KiB guards, filled with a NaN pattern (tests/test_config_space_gpu.py).  One
``HOSTILE <case> <route> <variant> err E_ref ratio ...`` line per test is the record of a run; ``HOSTILE-PAIRS`` lines give
max|a - b| / max|r64| for every pair of variants (B bf16x3, L unfused layer, T unfused tail, S SB head, F f32)."""
import itertools

import pytest
import torch

import hostile_stats_cases as S
from support import VARIANTS as PARITY_VARIANTS, assert_guards, dev, guard  # noqa: F401

pytestmark = pytest.mark.gpu

VARIANT_IDS = ('bf16x3', 'bf16x3-unfused-layer', 'bf16x3-unfused-tail', 'bf16x3-sb-head', 'f32')
VARIANTS = {v: PARITY_VARIANTS[v] for v in VARIANT_IDS}
TRIPLES = [(n, r, v) for n, c in S.CASES.items() for r in c['routes'] for v in VARIANT_IDS]
PAIRS = [(n, r) for n, c in S.CASES.items() for r in c['routes']]

_OUT = {}


def _run(name, route, variant, dev):
    """the engine's output of (case, route, variant) on the CPU, computed once per process"""
    key = (name, route, variant)
    if key in _OUT:
        return _OUT[key]
    from ddp_amd.engine import DDPEngine
    c = S.CASES[name]
    eng = guard(DDPEngine(S.state_dict(c), c['task'], device=dev, **VARIANTS[variant], **S.engine_kwargs(c, route)))
    if route == 'head':
        feat, temb = S.head_inputs(c)
        out = eng.head_forward(feat.to(dev), temb.to(dev))
    else:
        x, noise = S.sampler_inputs(c)
        if route == 'tf2':
            eng.set_x0_decisions(S.oracle_pair(c, route)['decisions'])
        out = eng.sample(x.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    assert_guards(eng, f'{name} {route} {variant}')
    _OUT[key] = out.cpu()
    return _OUT[key]


def test_variants_are_the_parity_suite_s():
    assert VARIANTS == {'bf16x3': dict(gemm='bf16x3'), 'bf16x3-unfused-layer': dict(gemm='bf16x3', fused_layer=False),
                        'bf16x3-unfused-tail': dict(gemm='bf16x3', fused_tail=False), 'bf16x3-sb-head': dict(gemm='bf16x3', nchw_head=False),
                        'f32': dict(gemm='f32')}
    assert S.FACTOR == 4 and S.CAP == 1e-5


@pytest.mark.parametrize('name,route,variant', TRIPLES)
def test_case_matches_fp64_oracle(dev, name, route, variant):
    c = S.CASES[name]
    p = S.oracle_pair(c, route)
    bar, e_ref, e_benign = S.bar_of(c, route)
    assert e_ref <= S.CAP and e_benign <= S.CAP and bar <= 4 * S.CAP          # the condition on the case (not a measurement)
    out = _run(name, route, variant, dev)
    r64 = p['r64']
    assert out.shape == r64.shape, (out.shape, r64.shape)
    finite = bool(torch.isfinite(out).all())
    err = S.err_vs(out, r64) if finite else float('nan')
    line = f'HOSTILE {name} {route} {variant} err {err:.3e} E_ref {e_ref:.3e} ratio {err / e_ref:.2f} benign {e_benign:.3e} bar {bar:.3e}'
    checks = [(finite, 'non-finite output'), (finite and err <= bar, 'err above the bar')]
    mask = S.degenerate_mask(c)
    if mask is not None and finite:
        # the constant / zero tokens alone, normalised by their own largest value; E_ref restricted in the same way
        m64 = r64[..., mask]
        e_rows = float((out.double()[..., mask] - m64).abs().max() / m64.abs().max())
        e_ref_rows = float((p['r32'].double()[..., mask] - m64).abs().max() / m64.abs().max())
        bar_rows = S.FACTOR * max(e_ref_rows, e_benign)
        line += f' | degenerate tokens err {e_rows:.3e} E_ref {e_ref_rows:.3e} bar {bar_rows:.3e}'
        checks += [(e_ref_rows <= S.CAP, 'degenerate tokens: E_ref above the cap'), (e_rows <= bar_rows, 'degenerate tokens: err above the bar')]
    if c['family'] == 'head' and finite:
        clear = S.top2_gap(p['r32']) > bar * p['scale']
        agree = float((out.argmax(1)[0] == p['r32'].argmax(1)[0])[clear].float().mean())
        line += f' | argmax agreement {agree:.4f} on {int(clear.sum())} of {clear.numel()} clear pixels'
        checks += [(int(clear.sum()) > 0.5 * clear.numel(), 'too few pixels with a clear top-2 gap'), (agree >= 0.999, 'argmax agreement')]
    print(line)
    failed = [what for ok, what in checks if not ok]
    assert not failed, f'{name} {route} {variant}: {failed}'


@pytest.mark.parametrize('name,route', PAIRS)
def test_variant_agreement(dev, name, route):
    """``bf16x3`` against ``bf16x3-unfused-tail``: k_layer MODE 6 against MODE 0 + MODE 4 / 1 is the same arithmetic, bit for bit,
    under hostile statistics too (seg; include/ddp_mi355x.h).  The distance between every other pair of variants is reported."""
    c = S.CASES[name]
    outs = {v: _run(name, route, v, dev) for v in VARIANT_IDS}
    scale = S.oracle_pair(c, route)['scale']
    short = dict(zip(VARIANT_IDS, 'BLTSF'))        # B bf16x3, L unfused layer, T unfused tail, S SB head, F f32
    line = ' '.join(f'{short[a]}{short[b]} {float((outs[a] - outs[b]).abs().max()) / scale:.1e}' for a, b in itertools.combinations(VARIANT_IDS, 2))
    print(f'HOSTILE-PAIRS {name} {route} {line}')
    if c['task'] == 'seg':
        assert torch.equal(outs['bf16x3'], outs['bf16x3-unfused-tail'])
