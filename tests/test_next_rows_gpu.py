"""The rows around the sampling loop - FPN, MultiStageMerging, their chained entry, FCNHeadWithTime, the sampler loop around it
and the four post-loop epilogues - swept over the geometry their code branches on, each against the CPU oracle.  Needs an
MI355X: ``pytest -m gpu``.

The cases are those of tests/next_rows_cases.py; tests/test_next_rows_host.py shows on the CPU that the oracle is conditioned
well enough on every one of them for the suite bar (REL = 2e-4) to apply unchanged, that the oracle itself has no near-ties
where decisions are compared, and that the workspace sizes queried here are the sums of the buffers the layouts carve.

Every call of a workspace-taking entry (``ddp_neck_fpn``, ``ddp_neck_msm``, ``ddp_neck_fpn_msm``, ``ddp_fcn_head_forward``,
``ddp_prepare_fcn`` / ``ddp_sample_fcn``, ``ddp_msda_forward_lds``) runs through the C ABI on a workspace of EXACTLY the queried
size, cut from a buffer with 4 KiB guards at both ends and filled with a NaN pattern, interior included: the guards must come
back untouched and a kernel that reads workspace bytes nobody wrote shows as a NaN in the output.

Every comparison prints one ``NEXT-ROWS <family> <case>: ...`` line with the measured error."""
import ctypes as C

import pytest
import torch

import next_rows_cases as N
from ddp_amd import _lib
from golden_util import max_rel
from oracle import ddp_oracle as O
from support import REL, Guarded, assert_guards as _assert_guards, dev, finite as _finite, stream as _stream  # noqa: F401

pytestmark = pytest.mark.gpu

CHAIN_VS_MEMBERS = 1e-5      # tests/test_hip_parity.py::test_fpn_then_merging_chain_matches_oracle
PROB_BAR = 2e-6              # tests/test_hip_parity.py epilogue tests: probabilities and averaged scores
DEPTH_BAR = 2e-5             # x max_depth (test_depth_epilogue_golden)


def test_bar_is_the_suite_bar():
    assert N.REL == REL == 2e-4


# ---- necks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', N.neck_names())
def test_fpn_matches_oracle(dev, name):
    """ddp_neck_fpn: all four outputs against the fp32 oracle (max-rel < REL); two calls give equal bits; image b of the batched
    call equals the single-image call bit for bit; guards untouched"""
    c = N.NECK[name]
    sdf, _, xs, _ = N.neck_dev(c, dev)
    outs, _ = N.run_fpn(c, dev, sdf, xs)
    ref = N.neck_oracle(c)['fpn']
    errs = [max_rel(o.cpu(), r) for o, r in zip(outs, ref)]
    print(f'NEXT-ROWS neck {name}: ddp_neck_fpn routes {"/".join(r[0] for r in c["routes"])}{" all-32" if c["all32"] else ""}, max-rel per '
          f'level {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e})')
    assert [tuple(o.shape) for o in outs] == [tuple(r.shape) for r in ref] and max(errs) < REL
    again, _ = N.run_fpn(c, dev, sdf, xs, what='second call')
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), f'{name}: two calls differ'
    if c['B'] > 1:
        for b in range(c['B']):
            one, _ = N.run_fpn(c, dev, sdf, N.images(xs, b), what=f'image {b} alone')
            for l in range(4):
                assert torch.equal(one[l][0], outs[l][b]), f'{name}: level {l} of image {b} differs between the batched and the single call'


@pytest.mark.parametrize('name', N.neck_names())
def test_chain_matches_oracle_and_members(dev, name):
    """ddp_neck_fpn_msm: the merged map against the fp32 oracle chain (< REL) and against ddp_neck_fpn followed by ddp_neck_msm
    (< 1e-5); equal bits on a second call and, image by image, from single-image calls"""
    c = N.NECK[name]
    sdf, sdm, xs, _ = N.neck_dev(c, dev)
    out, _ = N.run_chain(c, dev, sdf, sdm, xs)
    ref = N.neck_oracle(c)['chain']
    err = max_rel(out.cpu(), ref)
    outs, _ = N.run_fpn(c, dev, sdf, xs)
    members, _ = N.run_msm(c, dev, sdm, outs, False)
    pair = max_rel(out.cpu(), members.cpu())
    print(f'NEXT-ROWS neck {name}: ddp_neck_fpn_msm max-rel {err:.3e} (bar {REL:.0e}), vs member-by-member {pair:.3e} (bar {CHAIN_VS_MEMBERS:.0e})')
    assert out.shape == ref.shape and err < REL and pair < CHAIN_VS_MEMBERS
    again, _ = N.run_chain(c, dev, sdf, sdm, xs, what='second call')
    assert torch.equal(out, again), f'{name}: two calls differ'
    if c['B'] > 1:
        for b in range(c['B']):
            one, _ = N.run_chain(c, dev, sdf, sdm, N.images(xs, b), what=f'image {b} alone')
            assert torch.equal(one[0], out[b]), f'{name}: image {b} differs between the batched and the single call'


@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('name', N.neck_names(msm_only=True))
def test_msm_alone_matches_oracle(dev, name, align):
    """ddp_neck_msm on four 256-channel NCHW levels (read in place by the stream GEMM), both align_corners"""
    c = N.NECK[name]
    _, sdm, _, lvls = N.neck_dev(c, dev)
    out, _ = N.run_msm(c, dev, sdm, lvls, align)
    ref = N.neck_oracle(c)['msm'][align]
    err = max_rel(out.cpu(), ref)
    print(f'NEXT-ROWS neck {name}: ddp_neck_msm align_corners={align} max-rel {err:.3e} (bar {REL:.0e})')
    assert out.shape == ref.shape and err < REL
    again, _ = N.run_msm(c, dev, sdm, lvls, align, what='second call')
    assert torch.equal(out, again)
    if c['B'] > 1:
        for b in range(c['B']):
            one, _ = N.run_msm(c, dev, sdm, N.images(lvls, b), align, what=f'image {b} alone')
            assert torch.equal(one[0], out[b]), f'{name}: image {b} differs between the batched and the single call'


@pytest.mark.parametrize('first,second', [('all32_min', 'flat_pyramid'), ('flat_pyramid', 'all32_min')])
def test_neck_weights_ready_survives_a_geometry_change(dev, first, second):
    """DDP_NECK_WEIGHTS_READY (include/ddp_mi355x.h): the weight region sits at offsets that do not depend on batch or map
    sizes.  Pack at ``first``, then run ``second`` (another batch, other map sizes, the other statistics routes) with the flag
    set in the same buffer, sized for the larger of the two - in both directions, for all three entries.  The flagged call is
    handed OTHER convolution weights (output channels rolled by one; the GroupNorm vectors, which are read at call time, stay):
    its result must be, bit for bit, that of a fresh run with the PACKED weights - the flag does skip the re-packing and the
    stage images survive the change of geometry - and differ from a fresh run with the weights it was handed."""
    lib = _lib.load()
    a, b = N.NECK[first], N.NECK[second]
    assert a['channels'] == b['channels'] and a['B'] != b['B']
    sdf = {k: v.to(dev).contiguous() for k, v in N.fpn_state(a).items()}
    sdm = {k: v.to(dev).contiguous() for k, v in N.msm_state(a).items()}
    sdm['w'] = sdm['down.conv.weight'].reshape(256, 1024).contiguous()
    other_f = {k: (v.roll(1, 0).contiguous() if k.endswith('conv.weight') else v) for k, v in sdf.items()}
    other_m = dict(sdm, w=sdm['w'].roll(1, 0).contiguous())
    xa, la = [t.to(dev) for t in N.backbone_levels(a)], [t.to(dev) for t in N.fpn_like_levels(a)]
    xb, lb = [t.to(dev) for t in N.backbone_levels(b)], [t.to(dev) for t in N.fpn_like_levels(b)]
    sizes = [max(p, q) for p, q in zip(N.neck_queries(lib, a), N.neck_queries(lib, b))]
    ready = _lib.NECK_WEIGHTS_READY
    # ddp_neck_fpn
    g = Guarded(sizes[0], dev)
    N.run_fpn(a, dev, sdf, xa, g=g, what='packing call')
    kept, _ = N.run_fpn(b, dev, other_f, xb, flags=ready, g=g, what='weights ready')
    fresh, _ = N.run_fpn(b, dev, sdf, xb)
    handed, _ = N.run_fpn(b, dev, other_f, xb)
    assert all(torch.equal(p, q) for p, q in zip(kept, fresh)) and not any(torch.equal(p, q) for p, q in zip(kept, handed))
    # ddp_neck_msm
    g = Guarded(sizes[1], dev)
    N.run_msm(a, dev, sdm, la, False, g=g, what='packing call')
    kept, _ = N.run_msm(b, dev, other_m, lb, False, flags=ready, g=g, what='weights ready')
    assert torch.equal(kept, N.run_msm(b, dev, sdm, lb, False)[0]) and not torch.equal(kept, N.run_msm(b, dev, other_m, lb, False)[0])
    # ddp_neck_fpn_msm
    g = Guarded(sizes[2], dev)
    N.run_chain(a, dev, sdf, sdm, xa, g=g, what='packing call')
    kept, _ = N.run_chain(b, dev, other_f, other_m, xb, flags=ready, g=g, what='weights ready')
    fresh, _ = N.run_chain(b, dev, sdf, sdm, xb)
    assert torch.equal(kept, fresh) and not torch.equal(kept, N.run_chain(b, dev, other_f, other_m, xb)[0])
    err = max_rel(fresh.cpu(), O.neck_multi_stage_merging(list(O.neck_fpn(N.backbone_levels(b), N.fpn_state(a))), N.msm_state(a)))
    print(f'NEXT-ROWS neck weights_ready: {second} after {first} in one buffer with the flag set and other weights handed in, bit-equal '
          f'to a fresh run with the packed weights; vs oracle {err:.3e}')
    assert err < REL


# ---- FCNHeadWithTime ------------------------------------------------------------------------------------------------------------
def _run_fcn(c, dev, head, feat, temb, what=''):
    """ddp_fcn_head_forward through the C ABI (the parameter arrays are the plugin class's) on a guarded, exactly sized workspace"""
    lib = _lib.load()
    maps = feat.shape[0]
    g = Guarded(N.fcn_query(lib, c, maps), dev)
    arr, keep = head.conv_array()
    wseg = head.conv_seg.weight.detach().reshape(c['classes'], 256).contiguous()
    out = torch.full((maps, c['classes'], c['h'], c['w']), float('nan'), device=dev)
    _lib.check(lib.ddp_fcn_head_forward(arr, c['num_convs'], c['dilation'], wseg.data_ptr(), head.conv_seg.bias.detach().data_ptr(),
                                        c['classes'], feat.data_ptr(), temb.data_ptr() if temb is not None else None, maps, c['h'], c['w'],
                                        out.data_ptr(), g.ptr(), _stream(dev)), lib)
    torch.cuda.synchronize()
    _assert_guards(g, f'fcn {c["name"]} {what}')
    _finite(out, f'fcn {c["name"]} {what}')
    return out


@pytest.mark.parametrize('name', list(N.FCN))
def test_fcn_head_matches_oracle(dev, name):
    """ddp_fcn_head_forward against the fp32 oracle (< REL).  Dilation 16 on 5 x 7: also against the oracle of the same head
    with every off-centre tap zeroed - what the borders must do, stated independently.  Three 10 x 10 maps: every map of the
    batched call equals its single-map call bit for bit (tap_ok is all that keeps a tap out of the neighbouring map)."""
    c = N.FCN[name]
    sd = N.fcn_state(c)
    head = N.fcn_head(c, sd, dev)
    feat, temb = N.fcn_inputs(c)
    feat = feat.to(dev)
    temb = temb[0].contiguous().to(dev) if temb is not None else None
    out = _run_fcn(c, dev, head, feat, temb)
    ref = N.fcn_oracle(c)
    err = max_rel(out.cpu(), ref)
    line = f'NEXT-ROWS fcn {name}: max-rel {err:.3e} (bar {REL:.0e})'
    assert out.shape == ref.shape
    if c['dilation'] == 16 and (c['h'], c['w']) == (5, 7):
        centre = max_rel(out.cpu(), N.fcn_oracle(c, centre=True))
        line += f', vs centre-tap-only head {centre:.3e}'
        print(line)
        assert centre < REL
    else:
        print(line)
    assert err < REL
    assert torch.equal(out, _run_fcn(c, dev, head, feat, temb, what='second call'))
    if c['maps'] == 3:
        for b in range(3):
            one = _run_fcn(c, dev, head, feat[b:b + 1].contiguous(), temb, what=f'map {b} alone')
            assert torch.equal(one[0], out[b]), f'{name}: map {b} differs between the batched and the single call'


# ---- sampler loop around the FCN head -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(N.LOOP))
def test_fcn_loop_matches_oracle(dev, name):
    """ddp_sample_fcn, B images in one call, each against its own run of the reference sampler around the reference head:
    max-rel < REL and argmax agreement > 0.999 per image; a call with DDP_FLAG_FCN_PREPARED after ddp_prepare_fcn gives the bits
    of the self-preparing call; the batched call gives the bits of per-image calls.

    ONE engine: this loop has no fp32-MFMA form.  ddp_sample_fcn validates cfg.gemm_mode and never reads it again (every GEMM
    of the loop is launch_b3_linear / launch_b3_sgemm; ddp_amd.engine.FcnSamplerEngine sets DDP_GEMM_BF16X3), so a second
    run under DDP_GEMM_F32_MFMA would repeat this one bit for bit and is not claimed as a second engine."""
    c = N.LOOP[name]
    gemm = 'bf16x3'
    x, noise, sn = [t.to(dev) if t is not None else None for t in N.loop_inputs(c)]
    loop = N.device_loop(c, dev, gemm)
    out = loop.sample(x, noise, sn, what='self-preparing')
    ref = N.loop_oracle(c)
    assert out.shape == ref.shape
    o = out.cpu()
    errs = [max_rel(o[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    agree = [float((o[b].argmax(0) == ref[b].argmax(0)).float().mean()) for b in range(c['B'])]
    print(f'NEXT-ROWS loop {name}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e}), argmax equal '
          f'{" ".join(f"{a:.4f}" for a in agree)}')
    assert max(errs) < REL and min(agree) > 0.999
    prepared = N.device_loop(c, dev, gemm)
    prepared.prepare()
    assert torch.equal(prepared.sample(x, noise, sn, what='prepared'), out), f'{name}: prepared and self-preparing calls differ'
    assert torch.equal(prepared.sample(x, noise, sn, what='prepared, second call'), out)
    one = N.device_loop(c, dev, gemm, batch=1)
    for b in range(c['B']):
        ob = one.sample(x[b:b + 1].contiguous(), noise[b:b + 1].contiguous(), sn[:, b:b + 1].contiguous() if sn is not None else None,
                        what=f'image {b} alone')
        assert torch.equal(ob[0], out[b]), f'{name}: image {b} differs between the batched and the single-image call'


# ---- post-loop epilogues --------------------------------------------------------------------------------------------------------
def _class_map_rule(name, got, ref_seg, margin):
    """the rule of test_post_epilogue_golden: no mismatch where the reference's top-2 margin is above 1e-5, fewer than 1e-3
    mismatches in all"""
    diff = got.long() != ref_seg.long()
    share, above = float(diff.float().mean()), int((diff & (margin > N.MARGIN)).sum())
    assert share < N.TIE_SHARE and above == 0, f'{name}: {share:.2e} of the class map differs, {above} pixels above the margin'
    return share


@pytest.mark.parametrize('name', N.epi_names('post'))
def test_seg_postprocess_matches_oracle(name):
    from ddp_amd.engine import seg_postprocess
    c = N.EPI[name]
    sc = N.post_scores(c)
    got = seg_postprocess(sc.cuda(), c['img'], c['crop'], c['out'], c['align'], c['flip'])
    torch.cuda.synchronize()
    p = N.post_probs(c, sc)
    ref = O.seg_postprocess(sc, c['img'], c['crop'], c['out'], c['align'], c['flip'])
    assert got.shape == ref.shape and got.dtype == torch.uint8
    share = _class_map_rule(name, got.cpu(), ref, N.top2_margin(p))
    print(f'NEXT-ROWS epilogue {name}: class map {tuple(got.shape)}, {c["K"]} classes, share of differing pixels {share:.2e}')
    if c['B'] > 1:
        one = seg_postprocess(sc[1:2].cuda(), c['img'], c['crop'], c['out'], c['align'], c['flip'])
        assert torch.equal(one[0], got[1])


def test_seg_aug_postprocess_at_max_augs():
    """exactly DDP_MAX_AUGS augmentations of mixed sizes, crops and flips"""
    from ddp_amd.engine import seg_aug_postprocess
    c = N.EPI['aug_16']
    scores, metas = N.aug_inputs(c)
    seg, p = seg_aug_postprocess([t.cuda() for t in scores], metas, c['out'], c['align'], return_prob=True)
    torch.cuda.synchronize()
    ref, rp = O.seg_aug_test(scores, metas, c['out'], c['align'])
    err = max_rel(p.cpu(), rp)
    share = _class_map_rule('aug_16', seg.cpu(), ref, N.top2_margin(rp))
    print(f'NEXT-ROWS epilogue aug_16: {len(scores)} augmentations, probabilities max-rel {err:.3e} (bar {PROB_BAR:.0e}), differing pixels {share:.2e}')
    assert err < PROB_BAR
    assert torch.equal(seg_aug_postprocess([t.cuda() for t in scores], metas, c['out'], c['align']), seg)


def test_seg_slide_postprocess_at_max_windows():
    """exactly DDP_MAX_WINDOWS windows (8 x 8), the three ``want`` modes"""
    from ddp_amd.engine import seg_slide_postprocess
    c = N.EPI['slide_64']
    ys, xs, crop = N.slide_grid(c)
    sc = torch.stack(N.slide_inputs(c)).cuda()
    args = (sc, ys, xs, crop, c['img'], c['keep'], c['out'], c['align'])
    seg = seg_slide_postprocess(*args, flip=c['flip'], want='seg').cpu()
    prob = seg_slide_postprocess(*args, flip=c['flip'], want='prob').cpu()
    raw = seg_slide_postprocess(*args, flip=None, want='scores').cpu()
    rraw, rp = N.slide_oracle(c)
    e_raw, e_p = max_rel(raw, rraw), max_rel(prob, rp)
    share = _class_map_rule('slide_64', seg, rp.argmax(1), N.top2_margin(rp))
    print(f'NEXT-ROWS epilogue slide_64: {sc.shape[0]} windows, scores max-rel {e_raw:.3e}, probabilities {e_p:.3e} (bar {PROB_BAR:.0e}), '
          f'differing pixels {share:.2e}')
    assert e_raw < PROB_BAR and e_p < PROB_BAR


@pytest.mark.parametrize('name', N.epi_names('depth'))
def test_depth_postprocess_matches_oracle(name):
    from ddp_amd.engine import depth_postprocess
    c = N.EPI[name]
    maps, flips = N.depth_inputs(c)
    got = depth_postprocess([m.cuda() for m in maps], flips, c['out'], N.MIN_DEPTH, N.MAX_DEPTH, c['align'])
    torch.cuda.synchronize()
    ref = O.depth_postprocess(maps, flips, c['out'], N.MIN_DEPTH, N.MAX_DEPTH, c['align'])
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = float((got.cpu() - ref).abs().max())
    print(f'NEXT-ROWS epilogue {name}: {len(maps)} augmentations -> {tuple(got.shape)}, max abs diff {err:.3e} (bar {DEPTH_BAR * N.MAX_DEPTH:.1e})')
    assert err <= DEPTH_BAR * N.MAX_DEPTH
    assert float(got.min()) >= N.MIN_DEPTH and float(got.max()) <= N.MAX_DEPTH


# ---- the deformable-attention core's own workspace ------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,r', [(5, 7, 2), (1, 37, 1), (8, 16, 3)])
def test_msda_forward_lds_on_a_guarded_workspace(dev, h, w, r):
    """ddp_msda_forward_lds through a workspace of exactly ddp_msda_forward_lds_workspace bytes, on the 'wild' sample table of
    test_msda_forward_lds (N(0, 3 px) offsets, every 7th token on pixel centres, every 11th far outside the map): guards
    untouched, the oracle's explicit-tap restatement to that test's bar (1e-5)"""
    lib = _lib.load()
    n = h * w
    gen = torch.Generator().manual_seed(1200 + h * 100 + w)
    value = torch.randn(r, n, 8, 32, generator=gen)
    off = torch.randn(r, n, 8, 4, 2, generator=gen) * 3.0
    off[:, ::7] = torch.round(off[:, ::7])
    off[:, 3::11] *= 20.0
    aw = torch.randn(r, n, 8, 4, generator=gen).softmax(-1)
    jj = torch.arange(w, dtype=torch.float32).repeat(h)
    ii = torch.arange(h, dtype=torch.float32).repeat_interleave(w)
    px = jj[None, :, None, None] + off[..., 0]
    py = ii[None, :, None, None] + off[..., 1]
    ref = O.msda_core_taps(value, h, w, px, py, aw)
    samp = torch.cat([torch.stack((px, py), -1).reshape(r * n, 64), aw.reshape(r * n, 32)], 1).contiguous().to(dev)
    dv = value.reshape(r, n, 256).contiguous().to(dev)
    nb = C.c_size_t(0)
    _lib.check(lib.ddp_msda_forward_lds_workspace(r * n, h, w, C.byref(nb)), lib)
    g = Guarded(nb.value, dev)
    out = torch.full((r * n, 256), float('nan'), device=dev)
    _lib.check(lib.ddp_msda_forward_lds(dv.data_ptr(), samp.data_ptr(), None, out.data_ptr(), r * n, h, w, g.ptr(), _stream(dev)), lib)
    torch.cuda.synchronize()
    _assert_guards(g, f'msda_lds {h}x{w} r={r}')
    _finite(out, f'msda_lds {h}x{w}')
    err = max_rel(out.cpu().reshape(r, n, 256), ref)
    print(f'NEXT-ROWS msda_lds {h}x{w}_r{r}: guarded workspace of {nb.value} bytes, max-rel {err:.3e} (bar 1e-05)')
    assert err < 1e-5
