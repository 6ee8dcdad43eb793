"""No output depends on what the workspace held before the call.  Needs an MI355X: ``pytest -m gpu``.  (CPU companion:
tests/test_workspace_history_host.py; targets, fills and polluters: tests/workspace_history_cases.py.)

Every oracle comparison of the suite has one history: a fresh engine, a workspace filled with the quiet NaN 0x7FC0BEEF, the first call.
A kernel that reads workspace words nobody wrote is meant to show as a NaN - but ``fmaxf(NaN, 0) = 0``, ``NaN > x`` is false and a NaN
hint is "no hint", so the clamp and decision kernels turn such a read into a finite, plausible value; and one fill and one call say nothing
about state an earlier call left behind (the zero borders of the padded value maps, the model region across ``set_geometry``, prepared
FCN / neck weights, the rows rebuilt per call from the caller's regions, the in-place depth chain).

Pinned here, by ``bytes ==`` on every output (the returned tensor, step record and disagreement map, start map, x0 trace, seeded noise):
  1  fill independence      a fresh engine on a workspace filled with any of six words gives the bits of the NaN-filled run - which is
                            itself compared with the case's existing oracle expectation at the suite's bar, so equal wrong answers fail
  2  history independence   polluter call(s) on the SAME engine and workspace (other inputs x 1e3 with every caller region dense, NaN /
                            inf inputs on the four routes that already run them, a larger and a smaller geometry and back, another
                            batch), caller regions restored, then the target call: the fresh engine's bits
  3  T, T, P, T, P', T      four equal results in one engine
  4  graph replay           a captured call replayed after plain calls with other inputs through the same workspace
  5  prepared constants     DDP_FLAG_FCN_PREPARED / DDP_NECK_WEIGHTS_READY results survive other calls; without the flag nothing of
                            the previously packed weights is read
  6  entry points           the stand-alone workspace-taking entries: every fill, and after a call at another geometry

The workspace sits between two 4 KiB guards that keep the suite's PATTERN and are asserted after every call."""
import ctypes as C

import pytest
import torch

import fcn_gn_cases as G
import next_rows_cases as N
import support
import workspace_history_cases as W
from ddp_amd import _lib
from golden_util import load_case, max_rel
from support import PATTERN, REL, Guarded, assert_guards as _assert_guards, dev  # noqa: F401

pytestmark = pytest.mark.gpu

MSDA_BAR = 1e-5          # the literal of tests/test_hip_parity.py::test_msda_forward_lds (it has no name there)
NAN = W.FILLS['nan']


@pytest.fixture(scope='module', autouse=True)
def _release_what_the_module_holds():
    """the caches below (packed weights, device inputs, reference bits, entry objects) end with the module: the files
    collected after this one start from the allocator and the memory they would have found without it"""
    yield
    import gc
    for d in (_PW, _IN, _FRESH, _LOOP_FRESH, _ENTRY, _ENTRY_FRESH, N.NECK_DEV, W._OwnNoise._cache):
        d.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _same(a, b):
    """both dicts (or lists) of outputs hold the same bits (NaN payloads included)"""
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and _bits(a[k]) == _bits(b[k]) for k in a)
    return len(a) == len(b) and all(x.shape == y.shape and _bits(x) == _bits(y) for x, y in zip(a, b))


def _differs(a, b):
    return [k for k in a if a[k].shape != b[k].shape or _bits(a[k]) != _bits(b[k])]


def _fill(ws, word):
    ws.view(torch.int32).fill_(W.i32(word))


# ---- sampler engines ---------------------------------------------------------------------------------------------------------------
_PW, _IN, _FRESH = {}, {}, {}


def _guarded(n, dev, word):
    buf, ws = support.guarded_buffer(n, dev)
    _fill(ws, word)
    return buf, ws


def _engine(t, vid, dev, word=NAN):
    """a fresh DDPEngine of the route on a guarded workspace of exactly the queried size whose interior holds ``word``.  The packed
    weights - a caller-owned input, no part of the workspace - are uploaded once per target and handed to every engine of it."""
    from ddp_amd.engine import DDPEngine
    gemm, flags = t.routes[vid]
    sd = t.state_dict() if t.id not in _PW else None           # (not read once the packed weights exist; no host copy is kept)
    eng = DDPEngine(sd, t.c['task'], device=dev, gemm=gemm, weights=_PW.get(t.id), **flags, **t.ekw, **t.engine_kwargs())
    _PW[t.id] = eng.weights
    assert W.S.cfg_bytes(eng.cfg) == W.S.cfg_bytes(W.cfg_of(t, vid)), 'engine and workspace_history_cases.cfg_of disagree'
    n = eng.workspace.numel()
    assert n * 4 == eng._workspace_bytes()
    eng.guarded, eng.workspace = _guarded(n, dev, word)
    eng.word = word
    return eng


def _to(inp, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items() if k != 'regions'} | \
        dict(regions={k: v.to(dev) for k, v in inp['regions'].items()})


def _target_inputs(t, dev):
    if t.id not in _IN:
        _IN[t.id] = _to(t.inputs(), dev)
    return _IN[t.id]


def _set_regions(eng, regions):
    """the caller's part of the contract: every region the engine has is written - the given map, or the engine's own clear"""
    f = eng.cfg.flags
    for name, bit in (('hints', _lib.FLAG_X0_HINTS), ('prior', _lib.FLAG_PRIOR_START), ('class_prior', _lib.FLAG_CLASS_PRIOR),
                      ('score_prior', _lib.FLAG_SCORE_PRIOR)):
        if f & bit:
            if name in regions:
                getattr(eng, 'set_' + name)(regions[name])
            else:
                getattr(eng, 'clear_' + name)()


def _outputs(eng, out):
    f = eng.cfg.flags
    o = dict(out=out.cpu())
    if f & _lib.FLAG_STEP_RECORD:
        o['step_record'], o['step_disagreement'] = eng.step_record().cpu(), eng.step_disagreement().cpu()
    if f & _lib.FLAG_PRIOR_START:
        o['last_start'] = eng.last_start().cpu().clone()
    elif f & _lib.FLAG_SEEDED_NOISE:
        o['last_noise'] = eng.last_noise().cpu().clone()
    if f & (_lib.FLAG_RECORD_X0 | _lib.FLAG_FORCE_X0):
        o['x0_trace'] = eng.x0_trace().cpu()
    return o


def _call(eng, inp, what):
    _set_regions(eng, inp['regions'])
    if inp['seed'] is not None:
        out = eng.sample(inp['x'], seed=inp['seed'])
    else:
        out = eng.sample(inp['x'], inp['noise'], inp['sn'])
    torch.cuda.synchronize()
    _assert_guards(eng, what)
    return _outputs(eng, out)


def _fresh(tid, vid, dev, fill='nan', check=False):
    """the outputs of the first call of a fresh engine on a workspace filled with ``fill`` (once per route, fill and process).  The
    NaN-fill run is compared with the case's existing oracle expectation at the suite's bar; ``check``: raise if that comparison
    failed (the 'nan' item of the fill tests does, so equal wrong answers do not pass and a miss is reported once per route, not by
    every test built on these bits)"""
    key = (tid, vid, fill)
    t = W.TARGETS[tid]
    if key not in _FRESH:
        o = _call(_engine(t, vid, dev, W.FILLS[fill]), _target_inputs(t, dev), f'{tid}[{vid}] fresh, fill {fill}')
        try:
            if fill == 'nan':
                t.check(o, f'{tid}[{vid}]')
            _FRESH[key] = (o, None)
        except AssertionError as e:
            _FRESH[key] = (o, e)
    o, err = _FRESH[key]
    if check and err is not None:
        raise AssertionError(f'{tid}[{vid}]: the NaN-fill reference misses its oracle expectation: {err}')
    return o


def _move(eng, geometry, dev):
    """``set_geometry`` with the guards kept: where the workspace has to grow, the regrow of DDPEngine.set_geometry (a larger buffer,
    the model region copied) is made here on a guarded buffer holding the engine's fill word, and set_geometry finds room"""
    n = _lib.DdpCfg.from_buffer_copy(eng.cfg)
    n.batch, n.h, n.w = geometry
    if eng.task != 'bev' and (eng.cfg.head_h, eng.cfg.head_w) == (eng.cfg.h, eng.cfg.w):
        n.head_h, n.head_w = n.h, n.w
    nbytes = C.c_size_t(0)
    _lib.check(eng.lib.ddp_query_workspace(C.byref(n), C.byref(nbytes)), eng.lib)
    need = nbytes.value // 4
    grew = need > eng.workspace.numel()
    if grew:
        buf, ws = _guarded(need, dev, eng.word)
        if eng._prepared:
            ws[:eng._const_floats].copy_(eng.workspace[:eng._const_floats])
        eng.guarded, eng.workspace = buf, ws
    ptr = eng.workspace.data_ptr()
    eng.set_geometry(*geometry)
    assert eng.workspace.data_ptr() == ptr and eng.geometry() == tuple(geometry)
    return grew


def _still_fill(eng):
    """share of the interior words outside the model region that still hold the fill word"""
    w = eng.workspace[eng._const_floats:].view(torch.int32)
    return float((w == W.i32(eng.word)).float().mean())


def _pollute(eng, t, polluter, dev, what):
    """one polluter on the engine -> (its outputs, share of the workspace still holding the fill afterwards); the engine is back at
    the target's geometry, its caller regions are whatever the polluter (or set_geometry) left"""
    if polluter in ('other_inputs', 'nan_inputs'):
        o = _call(eng, _to(t.inputs_at(t.geometry(), nan=polluter == 'nan_inputs'), dev), f'{what} {polluter}')
        return o, _still_fill(eng)
    g = t.polluter_geometry(polluter)
    _move(eng, g, dev)
    o = _call(eng, _to(t.inputs_at(g), dev), f'{what} {polluter} at {g}')
    share = _still_fill(eng)
    _move(eng, t.geometry(), dev)
    return o, share


def test_fills_hold_the_suite_pattern():
    assert W.FILLS['nan'] == PATTERN == 0x7FC0BEEF and W.REL == REL == 2e-4


@pytest.mark.parametrize('fill', list(W.FILLS))
@pytest.mark.parametrize('tid,vid', W.pairs())
def test_fill_independence(dev, tid, vid, fill):
    """1: a fresh engine on a workspace filled with ``fill``, the caller regions set as the contract says, one call: the bits of the
    NaN-fill run, which holds the oracle bar"""
    t = W.TARGETS[tid]
    want = _fresh(tid, vid, dev, check=fill == 'nan')
    if fill == 'nan':                                   # (a second fresh engine: the reference repeats itself)
        got = _call(_engine(t, vid, dev), _target_inputs(t, dev), f'{tid}[{vid}] fill nan, again')
    else:
        got = _fresh(tid, vid, dev, fill)
    assert _same(got, want), f'{tid}[{vid}]: outputs {_differs(got, want)} depend on the workspace fill {W.FILLS[fill]:#010x}'


@pytest.mark.parametrize('tid,vid,polluter,fill', W.history_items())
def test_history_independence(dev, tid, vid, polluter, fill):
    """2: the polluter, then the target call on the same engine and workspace: the bits of the fresh engine on the same fill (which
    test 1 ties to the NaN-fill run and the oracle).  NaN fill: whatever the polluter did not write stays loud.  Zero fill: the
    only thing that differs from the fresh engine is what the polluter left behind - a stale finite row where the library keeps a
    zero it wrote once would drown in the NaNs of the other fill."""
    t = W.TARGETS[tid]
    want = _fresh(tid, vid, dev, fill)
    eng = _engine(t, vid, dev, W.FILLS[fill])
    po, share = _pollute(eng, t, polluter, dev, f'{tid}[{vid}]')
    print(f'WS-HISTORY {tid}[{vid}] {polluter} fill {fill}: words_rewritten={1.0 - share:.4f} of the workspace behind the model region')
    assert share < 1.0, 'the polluter left nothing behind'
    assert po['out'].shape != want['out'].shape or _bits(po['out']) != _bits(want['out']), 'the polluter computed the target\'s result'
    got = _call(eng, _target_inputs(t, dev), f'{tid}[{vid}] after {polluter}')
    assert _same(got, want), f'{tid}[{vid}]: outputs {_differs(got, want)} depend on the {polluter} call in front'


@pytest.mark.parametrize('fill', W.HISTORY_FILLS)
@pytest.mark.parametrize('tid,vid', W.SEQUENCE_TARGETS)
def test_target_twice_then_polluter_then_target(dev, tid, vid, fill):
    """3: T, T, P, T, P', T in one engine - four equal results, equal to the fresh engine's on the same fill"""
    t = W.TARGETS[tid]
    want = _fresh(tid, vid, dev, fill)
    eng = _engine(t, vid, dev, W.FILLS[fill])
    inp = _target_inputs(t, dev)
    runs = [_call(eng, inp, f'{tid} T1'), _call(eng, inp, f'{tid} T2')]
    _pollute(eng, t, 'other_inputs', dev, tid)
    runs.append(_call(eng, inp, f'{tid} T3'))
    _pollute(eng, t, 'bigger_then_back', dev, tid)           # (the workspace regrows: the model region is copied)
    runs.append(_call(eng, inp, f'{tid} T4'))
    for i, r in enumerate(runs):
        assert _same(r, want), f'{tid}[{vid}]: call T{i + 1} of T, T, P, T, P\', T differs in {_differs(r, want)}'


@pytest.mark.parametrize('tid,vid', W.GRAPH_TARGETS)
def test_graph_replay_after_intervening_calls(dev, tid, vid):
    """4: capture and replay the target; three plain calls with other inputs through the same workspace; replay again with the
    target's inputs copied into the static buffers: the bits of the first replay and of the plain call"""
    t = W.TARGETS[tid]
    want = _fresh(tid, vid, dev)
    eng = _engine(t, vid, dev)
    inp = _target_inputs(t, dev)
    graph = eng.capture(inp['x'], inp['noise'], inp['sn'])
    first = graph.replay(inp['x'], inp['noise'], inp['sn']).clone()
    torch.cuda.synchronize()
    _assert_guards(eng, f'{tid} first replay')
    other = _to(t.inputs_at(t.geometry()), dev)
    for i in range(3):
        po = _call(eng, other, f'{tid} plain call {i}')
    assert _bits(po['out']) != _bits(want['out'])
    again = graph.replay(inp['x'], inp['noise'], inp['sn']).clone()
    torch.cuda.synchronize()
    _assert_guards(eng, f'{tid} second replay')
    assert _bits(first) == _bits(want['out']), f'{tid}[{vid}]: the replay differs from the plain call'
    assert _bits(again) == _bits(first), f'{tid}[{vid}]: the replay after intervening calls differs from the first replay'


# ---- the FCN-head loop -------------------------------------------------------------------------------------------------------------
_LOOP_FRESH = {}


def _loop(name, dev, batch=None):
    src, c = W.LOOPS[name]
    if src == 'next_rows_cases':
        return N.device_loop(c, dev, 'bf16x3', batch)
    return G.device_loop(c, G.loop_state(c), dev, batch)


def _loop_inputs(name, dev, other=False, batch=None):
    src, c = W.LOOPS[name]
    M = N if src == 'next_rows_cases' else G
    x, noise, sn = M.loop_inputs(dict(c, seed=c['seed'] + 4000) if other else c)
    if other:
        x, noise = x * 1e3, noise * 1e3
    if batch is not None:
        x, noise, sn = x[:batch], noise[:batch], None if sn is None else sn[:, :batch]
    return [None if v is None else v.contiguous().to(dev) for v in (x, noise, sn)]


def _loop_run(loop, name, dev, prepared, word, what):
    """fill the interior, (prepare,) one call"""
    _fill(loop.g.ws, word)
    if prepared:
        loop.prepare()
    return [loop.sample(*_loop_inputs(name, dev), what=what).cpu()]


def _loop_fresh(name, prepared, dev, check=False):
    key = (name, prepared)
    if key not in _LOOP_FRESH:
        src, c = W.LOOPS[name]
        out = _loop_run(_loop(name, dev), name, dev, prepared, NAN, 'fresh')
        ref = N.loop_oracle(c) if src == 'next_rows_cases' else G.loop_expect(c)[0]
        errs = [max_rel(out[0][b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
        agree = float((out[0].argmax(1) == ref.argmax(1)).float().mean())
        print(f'WS-HISTORY oracle loop {name} prepared={prepared}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} '
              f'(bar {REL:.0e}), argmax equal {agree:.4f}')
        _LOOP_FRESH[key] = (out, max(errs) < REL and agree > 0.999)
    out, ok = _LOOP_FRESH[key]
    assert ok or not check, f'loop {name}: the NaN-fill reference misses its oracle expectation'
    return out


@pytest.mark.parametrize('fill', list(W.FILLS))
@pytest.mark.parametrize('prepared', [False, True], ids=['self-preparing', 'prepared'])
@pytest.mark.parametrize('name', list(W.LOOPS))
def test_fcn_loop_fill_independence(dev, name, prepared, fill):
    """1 for ``ddp_sample_fcn``: BatchNorm and GroupNorm(32) heads, with and without DDP_FLAG_FCN_PREPARED"""
    want = _loop_fresh(name, prepared, dev, check=fill == 'nan')
    got = _loop_run(_loop(name, dev), name, dev, prepared, W.FILLS[fill], f'fill {fill}')
    assert _same(got, want), f'loop {name}: the output depends on the workspace fill {W.FILLS[fill]:#010x}'


@pytest.mark.parametrize('polluter', ['other_inputs', 'other_batch'])
@pytest.mark.parametrize('name', list(W.LOOPS))
def test_fcn_loop_history_independence(dev, name, polluter):
    """2 for the self-preparing loop: other inputs x 1e3, or a single-image call through the same buffer, then the target call"""
    want = _loop_fresh(name, False, dev)
    loop = _loop(name, dev)
    if polluter == 'other_inputs':
        po = loop.sample(*_loop_inputs(name, dev, other=True), what=polluter)
        assert _bits(po) != _bits(want[0])
    else:
        one = _loop(name, dev, batch=1)
        one.g = loop.g                               # the same buffer, the single-image layout underneath
        one.sample(*_loop_inputs(name, dev, other=True, batch=1), what=polluter)
    share = float((loop.g.ws.view(torch.int32) == PATTERN).float().mean())
    print(f'WS-HISTORY loop {name} {polluter}: words_rewritten={1.0 - share:.4f}')
    assert share < 1.0
    got = [loop.sample(*_loop_inputs(name, dev), what=f'after {polluter}').cpu()]
    assert _same(got, want), f'loop {name}: the output depends on the {polluter} call in front'


# ---- stand-alone entries -----------------------------------------------------------------------------------------------------------
def _roll(sd):
    """other convolution weights: output channels rolled by one (test_neck_weights_ready_survives_a_geometry_change's)"""
    return {k: (v.roll(1, 0).contiguous() if k.endswith('conv.weight') or k == 'w' else v) for k, v in sd.items()}


class _Entry:
    """One stand-alone entry on its target case and on another geometry: ``bytes(other)`` from the library's own query,
    ``run(g, other, flags, rolled, scale)`` -> list of output tensors (device), ``reference()`` -> (list of expectations, bar)."""

    def __init__(self, name, dev):
        self.name, self.dev, self.lib = name, dev, _lib.load()
        self.kind = name if not name.startswith('msda') else 'msda_lds'
        getattr(self, '_init_' + self.kind)()

    # necks
    def _neck(self, other):
        return N.NECK[W.NECK_OTHER if other else W.NECK_CASE]

    def _neck_tensors(self, other):
        c = self._neck(other)
        if other not in self.t:
            sdf = {k: v.to(self.dev).contiguous() for k, v in N.fpn_state(c).items()}
            sdm = {k: v.to(self.dev).contiguous() for k, v in N.msm_state(c).items()}
            sdm['w'] = sdm['down.conv.weight'].reshape(256, 1024).contiguous()
            self.t[other] = (sdf, sdm, [x.to(self.dev) for x in N.backbone_levels(c)], [x.to(self.dev) for x in N.fpn_like_levels(c)])
        return self.t[other]

    def _init_neck_fpn(self):
        self.t = {}
    _init_neck_msm = _init_neck_fpn_msm = _init_neck_fpn

    def _run_neck(self, g, other, flags, rolled, scale):
        c = self._neck(other)
        sdf, sdm, xs, lv = self._neck_tensors(other)
        if rolled:
            sdf, sdm = _roll(sdf), _roll(sdm)
        xs, lv = [x * scale for x in xs], [x * scale for x in lv]
        if self.kind == 'neck_fpn':
            return N.run_fpn(c, self.dev, sdf, xs, flags, g)[0]
        if self.kind == 'neck_msm':
            return [N.run_msm(c, self.dev, sdm, lv, False, flags, g)[0]]
        return [N.run_chain(c, self.dev, sdf, sdm, xs, False, flags, g)[0]]

    # FCN heads
    def _fcn(self, other):
        if self.kind == 'fcn_head_bn':
            return N.FCN[W.FCN_BN_OTHER if other else W.FCN_BN_CASE]
        return G.HEAD[W.FCN_GN_OTHER if other else W.FCN_GN_CASE]

    def _init_fcn_head_bn(self):
        self.t = {}
    _init_fcn_head_gn = _init_fcn_head_bn

    def _run_fcn(self, g, other, flags, rolled, scale):
        c = self._fcn(other)
        key = (other, rolled)
        if key not in self.t:
            bn = self.kind == 'fcn_head_bn'
            sd = N.fcn_state(c) if bn else G.head_state(c)
            if rolled:
                sd = _roll(sd)
            feat, temb = N.fcn_inputs(c) if bn else G.head_inputs(c)
            if bn:
                head = N.fcn_head(c, sd, self.dev)
                arr, keep = head.conv_array()
                keep = (keep, head)
            else:
                arr, keep = G.conv_array(sd, c, self.dev)
            wseg = sd['conv_seg.weight'].reshape(c['classes'], 256).contiguous().to(self.dev)
            bseg = sd['conv_seg.bias'].contiguous().to(self.dev)
            self.t[key] = (arr, keep, wseg, bseg, feat.to(self.dev), temb[0].contiguous().to(self.dev) if temb is not None else None)
        arr, _, wseg, bseg, feat, temb = self.t[key]
        feat = (feat * scale).contiguous()
        out = torch.full((c['maps'], c['classes'], c['h'], c['w']), float('nan'), device=self.dev)
        _lib.check(self.lib.ddp_fcn_head_forward(arr, c['num_convs'], c['dilation'], wseg.data_ptr(), bseg.data_ptr(), c['classes'],
                                                 feat.data_ptr(), temb.data_ptr() if temb is not None else None, c['maps'], c['h'], c['w'],
                                                 out.data_ptr(), g.ptr(), support.stream(self.dev)), self.lib)
        return [out]

    # the LDS gather
    def _init_msda_lds(self):
        _, _, table, *guess = self.name.split('_')
        self.table, self.guess, self.t = table, bool(guess), {}

    def _msda(self, other):
        h, w, r = W.MSDA_OTHER if other else W.MSDA_SHAPE
        if other not in self.t:
            value, samp, mean, ref = W.msda_inputs(h, w, r, self.table)
            self.t[other] = (value.contiguous().to(self.dev), samp.to(self.dev), mean.contiguous().to(self.dev), ref)
        return (h, w, r) + self.t[other]

    def _run_msda(self, g, other, flags, rolled, scale):
        h, w, r, value, samp, mean, _ = self._msda(other)
        value = (value * scale).contiguous()
        out = torch.full((r * h * w, 256), float('nan'), device=self.dev)
        _lib.check(self.lib.ddp_msda_forward_lds(value.data_ptr(), samp.data_ptr(), mean.data_ptr() if self.guess else None, out.data_ptr(),
                                                 r * h * w, h, w, g.ptr(), support.stream(self.dev)), self.lib)
        return [out]

    # the bf16x3 stream GEMM
    def _init_linear_b3(self):
        self.t = {}

    def _run_linear(self, g, other, flags, rolled, scale):
        m, n, k = W.LINEAR_B3_OTHER if other else W.LINEAR_B3_SHAPE
        if other not in self.t:
            self.t[other] = [v.to(self.dev) for v in W.linear_b3_inputs(m, n, k)[:3]]
        a, w, b = self.t[other]
        a = (a * scale).contiguous()
        out = torch.full((m, n), float('nan'), device=self.dev)
        _lib.check(self.lib.ddp_linear_b3(a.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, g.ptr(), support.stream(self.dev)),
                   self.lib)
        return [out]

    # DeformableHeadWithTime.forward
    def _init_head_forward(self):
        from oracle import ddp_oracle as O
        cfg, sd, _, _, _, gold = load_case(W.HEAD_FORWARD_CASE)
        self.eng = support.fixture_engine(cfg, sd, self.dev)
        self.feat = gold['feat_step0'].to(self.dev).contiguous()
        self.temb = O.time_mlp(O.alpha_cosine_log_snr(torch.tensor([1.0])), sd).to(self.dev)
        self.ref = gold['logits_steps'][0]
        self.home = self.eng.geometry()

    def _run_head(self, g, other, flags, rolled, scale):
        eng = self.eng
        eng.guarded, eng.workspace, eng.word = g.guarded, g.ws, NAN
        B, h, w = self.home
        geo = (B, h - 2, w - 3) if other else self.home
        if eng.geometry() != geo:
            _move(eng, geo, self.dev)
        feat = self.feat[:, :, :geo[1], :geo[2]].contiguous() * scale
        return [eng.head_forward(feat, self.temb)]

    def bytes(self, other=False):
        n = C.c_size_t(0)
        if self.kind.startswith('neck'):
            return N.neck_queries(self.lib, self._neck(other))[['neck_fpn', 'neck_msm', 'neck_fpn_msm'].index(self.kind)]
        if self.kind.startswith('fcn'):
            return N.fcn_query(self.lib, self._fcn(other))
        if self.kind == 'msda_lds':
            h, w, r = W.MSDA_OTHER if other else W.MSDA_SHAPE
            _lib.check(self.lib.ddp_msda_forward_lds_workspace(r * h * w, h, w, C.byref(n)), self.lib)
        elif self.kind == 'linear_b3':
            _lib.check(self.lib.ddp_linear_b3_workspace(*(W.LINEAR_B3_OTHER if other else W.LINEAR_B3_SHAPE), C.byref(n)), self.lib)
        else:
            B, h, w = self.home
            cfg = _lib.DdpCfg.from_buffer_copy(self.eng.cfg)
            if other:
                cfg.h, cfg.w, cfg.head_h, cfg.head_w = h - 2, w - 3, h - 2, w - 3
            _lib.check(self.lib.ddp_query_workspace(C.byref(cfg), C.byref(n)), self.lib)
        return n.value

    def run(self, g, other=False, flags=0, rolled=False, scale=1.0, what=''):
        fn = {'neck_fpn': self._run_neck, 'neck_msm': self._run_neck, 'neck_fpn_msm': self._run_neck, 'fcn_head_bn': self._run_fcn,
              'fcn_head_gn': self._run_fcn, 'msda_lds': self._run_msda, 'linear_b3': self._run_linear, 'head_forward': self._run_head}[self.kind]
        outs = fn(g, other, flags, rolled, scale)
        torch.cuda.synchronize()
        _assert_guards(g, f'{self.name} {what}')
        return [o.cpu() for o in outs]

    def reference(self):
        """the entry's existing oracle expectation and the bar its current test uses"""
        if self.kind == 'neck_fpn':
            return list(N.neck_oracle(self._neck(False))['fpn']), REL
        if self.kind == 'neck_msm':
            return [N.neck_oracle(self._neck(False))['msm'][False]], REL
        if self.kind == 'neck_fpn_msm':
            return [N.neck_oracle(self._neck(False))['chain']], REL
        if self.kind == 'fcn_head_bn':
            return [N.fcn_oracle(self._fcn(False))], REL
        if self.kind == 'fcn_head_gn':
            return [G.head_expect(self._fcn(False))], REL
        if self.kind == 'msda_lds':
            h, w, r, _, _, _, ref = self._msda(False)
            return [ref.reshape(r * h * w, 256)], MSDA_BAR
        if self.kind == 'linear_b3':
            return [W.linear_b3_inputs(*W.LINEAR_B3_SHAPE)[3]], REL
        return [self.ref], REL


_ENTRY, _ENTRY_FRESH = {}, {}


def _entry(name, dev):
    if name not in _ENTRY:
        _ENTRY[name] = _Entry(name, dev)
    return _ENTRY[name]


def _entry_fresh(name, dev, check=False):
    """the NaN-fill first call on a workspace of exactly the queried size, against the entry's existing expectation"""
    e = _entry(name, dev)
    if name not in _ENTRY_FRESH:
        out = e.run(Guarded(e.bytes(), dev), what='fresh')
        refs, bar = e.reference()
        errs = [max_rel(o.double(), r.double()) for o, r in zip(out, refs)]
        print(f'WS-HISTORY oracle entry {name}: max-rel {" ".join(f"{x:.3e}" for x in errs)} (bar {bar:.0e})')
        _ENTRY_FRESH[name] = (out, len(out) == len(refs) and all(torch.isfinite(o).all() for o in out) and max(errs) < bar)
    out, ok = _ENTRY_FRESH[name]
    assert ok or not check, f'{name}: the NaN-fill reference misses its oracle expectation'
    return out


@pytest.mark.parametrize('fill', list(W.FILLS))
@pytest.mark.parametrize('name', W.ENTRIES)
def test_entry_points_fill_and_history(dev, name, fill):
    """6: the entry on a workspace of exactly the queried size whose interior holds ``fill``; then, through one buffer sized for both,
    a call at another geometry (inputs x 1e3) followed by the target call - the bits of the NaN-fill first call both times"""
    e = _entry(name, dev)
    want = _entry_fresh(name, dev, check=fill == 'nan')
    g = Guarded(e.bytes(), dev)
    _fill(g.ws, W.FILLS[fill])
    assert _same(e.run(g, what=f'fill {fill}'), want), f'{name}: the output depends on the workspace fill {W.FILLS[fill]:#010x}'
    g = Guarded(max(e.bytes(), e.bytes(other=True)), dev)
    _fill(g.ws, W.FILLS[fill])
    e.run(g, other=True, scale=1e3, what=f'other geometry, fill {fill}')
    assert _same(e.run(g, what=f'after the other geometry, fill {fill}'), want), f'{name}: the output depends on the call in front'


@pytest.mark.parametrize('name', list(W.LOOPS) + ['neck_fpn', 'neck_msm', 'neck_fpn_msm'])
def test_prepared_constants_survive(dev, name):
    """5, first sequence: prepared once (``ddp_prepare_fcn``; a packing call for DDP_NECK_WEIGHTS_READY), then T, P (other inputs
    x 1e3), T with the flag set: equal bits, the fresh run's"""
    if name in W.LOOPS:
        want = _loop_fresh(name, True, dev)
        loop = _loop(name, dev)
        loop.prepare()
        a = loop.sample(*_loop_inputs(name, dev), what='T').cpu()
        p = loop.sample(*_loop_inputs(name, dev, other=True), what='P').cpu()
        b = loop.sample(*_loop_inputs(name, dev), what='T after P').cpu()
        assert _bits(p) != _bits(a) and _same([a], want) and _same([b], want), f'loop {name}: prepared constants did not survive'
        return
    e = _entry(name, dev)
    want = _entry_fresh(name, dev)
    g = Guarded(e.bytes(), dev)
    ready = _lib.NECK_WEIGHTS_READY
    e.run(g, what='packing call')
    a = e.run(g, flags=ready, rolled=True, what='T, weights ready')              # (handed other weights: the flag must skip the packing)
    p = e.run(g, flags=ready, rolled=True, scale=1e3, what='P, weights ready')
    b = e.run(g, flags=ready, rolled=True, what='T after P, weights ready')
    assert not _same(p, a) and _same(a, want) and _same(b, want), f'{name}: packed weights did not survive'


@pytest.mark.parametrize('name', ['neck_fpn', 'neck_msm', 'neck_fpn_msm', 'fcn_head_bn', 'fcn_head_gn'])
def test_unflagged_call_reads_nothing_of_the_previous_weights(dev, name):
    """5, second sequence: weights A through the workspace with no flag, then weights B with no flag: a fresh run of B"""
    e = _entry(name, dev)
    want = _entry_fresh(name, dev)
    g = Guarded(e.bytes(), dev)
    a = e.run(g, rolled=True, what='weights A')
    assert not _same(a, want)
    assert _same(e.run(g, what='weights B after A'), want), f'{name}: a call without the flag read planes packed from other weights'
