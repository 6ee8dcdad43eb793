"""CPU companion of tests/test_workspace_history_gpu.py: the case table of tests/workspace_history_cases.py is deterministic, names
existing cases with a loadable oracle expectation and existing routes, every polluter geometry is a workspace the library accepts and
that differs from the target's, every path of the table is among the generated items - and the arithmetic that lets a read of
uninitialised workspace pass as a plausible value, which is why the fills exist."""
import collections
import importlib

import numpy as np
import pytest
import torch

import config_space_cases as S
import support
import workspace_history_cases as W
from support import lib  # noqa: F401


def test_fills_hold_the_suite_pattern():
    assert W.PATTERN == support.PATTERN == 0x7FC0BEEF and W.FILLS['nan'] == support.PATTERN
    assert sorted(W.FILLS.values()) == sorted([0x7FC0BEEF, 0x00000000, 0x3F800000, 0x7F800000, 0xFF7FFFFF, 0x41414141])
    as_float = {k: float(np.array([v], dtype=np.uint32).view(np.float32)[0]) for k, v in W.FILLS.items()}
    assert np.isnan(as_float['nan']) and as_float['zero'] == 0.0 and as_float['one'] == 1.0 and as_float['inf'] == float('inf')
    assert as_float['neg_flt_max'] == -float(np.finfo(np.float32).max) and abs(as_float['x41'] - 12.08) < 0.01
    assert all(np.array([W.i32(v)], dtype=np.int32).view(np.uint32)[0] == v for v in W.FILLS.values())


def test_the_table_is_deterministic_and_complete():
    before = (list(W.TARGETS), W.pairs(), W.history_items(), W.smallest_per_path())
    m = importlib.reload(W)                                              # (built a second time, in place)
    assert (list(m.TARGETS), m.pairs(), m.history_items(), m.smallest_per_path()) == before
    assert set(W.smallest_per_path()) == {c['path'] for c in S.CASES.values() if 'path' in c}      # every path of the sweep has a target
    got = {(W.TARGETS[tid].path, vid) for tid, vid in W.pairs()}
    missing = [p for p in W.REQUIRED if p not in got]
    assert not missing, f'paths of the case table without a generated item: {missing}'
    per = collections.Counter(p for _, _, p, _ in W.history_items())
    tasks = {p: {W.TARGETS[tid].c['task'] for tid, _, q, _ in W.history_items() if q == p} for p in W.POLLUTERS}
    print('WS-HISTORY items: ' + ', '.join(f'{p} {per[p]}' for p in W.POLLUTERS) + f'; fill items {len(W.pairs()) * len(W.FILLS)}')
    for p in W.POLLUTERS:
        assert tasks[p] >= ({'seg'} if p == 'nan_inputs' else {'seg', 'depth', 'bev'}), (p, tasks[p])
    # nan_inputs: only the four routes tests/test_hip_parity.py::test_nan_input_does_not_fault already runs
    nan = {(W.TARGETS[tid].c['sampler'], vid) for tid, vid, p, _ in W.history_items() if p == 'nan_inputs'}
    assert nan == {('ddim', 'bf16x3'), ('ddim', 'f32'), ('ddim', 'unfused-layer'), ('ddpm', 'bf16x3')}
    assert all(W.TARGETS[tid].c['B'] > 1 for tid, _, p, _ in W.history_items() if p == 'other_batch')
    for tid, vid in W.SEQUENCE_TARGETS + W.GRAPH_TARGETS:
        assert vid in W.TARGETS[tid].routes


@pytest.mark.parametrize('tid', list(W.TARGETS))
def test_target_names_an_existing_case_with_its_routes_and_expectation(tid):
    t = W.TARGETS[tid]
    src = importlib.import_module(t.source)
    cases = getattr(src, 'ALL', None) or src.CASES
    base = t.c['name'].split('/')[0]
    names = {(c[0] if isinstance(c, tuple) else c)['name'] for c in cases.values()}
    assert base in names or t.c['name'] in names, f'{tid}: {t.c["name"]} is no case of {t.source}'
    table = W.ROUTE_TABLES[t.source](t)
    for vid, (gemm, _) in t.routes.items():
        assert (vid, gemm) in table, f'{tid}: route {vid} is not in the route table of {t.source}'
    e = t.expectation()
    if e is None:                                                        # formed from the call's own start noise: the oracle must run on the case
        x, noise, _ = S.inputs(t.c)
        e = S.oracle_image(t.c, t.state_dict(), x, noise, None, 0)
    for v in (e.values() if isinstance(e, dict) else e if isinstance(e, (tuple, list)) else [e]):
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all()
    a, b = t.inputs_at(t.geometry()), t.inputs_at(t.geometry())
    assert all(torch.equal(a['regions'][k], b['regions'][k]) for k in a['regions']) and torch.equal(a['x'], b['x'])
    assert not torch.equal(a['x'], t.inputs()['x'])
    assert (a['seed'] is None) == (t.seed is None) and (t.seed is None or a['seed'] != t.seed)
    bad = t.inputs_at(t.geometry(), nan=True)
    assert torch.isnan(bad['x']).any() and torch.isinf(bad['x']).any()


@pytest.mark.parametrize('tid,vid', W.pairs())
def test_polluter_geometries_are_accepted_and_differ(lib, tid, vid):
    t = W.TARGETS[tid]
    rc, home = W.query(lib, W.cfg_of(t, vid))
    assert rc == 0, lib.ddp_last_error().decode()
    line = f'WS-HISTORY workspace {tid}[{vid}] {t.geometry()}: {home} B'
    for p in sorted(set(t.polluters(vid)) - {'other_inputs', 'nan_inputs'}):
        g = t.polluter_geometry(p)
        rc, n = W.query(lib, W.cfg_of(t, vid, g))
        assert rc == 0, f'{tid}[{vid}] {p} {g}: {lib.ddp_last_error().decode()}'
        line += f'; {p} {g}: {n} B'
        assert g != t.geometry() and n != home, f'{tid}[{vid}]: the {p} workspace has the target\'s size'
        if p == 'bigger_then_back':
            assert n > home
    print(line)


# ---- why the fills exist: a NaN read from the workspace becomes a plausible value (numpy restatement of the kernels' arithmetic) -----
def test_depth_update_turns_a_nan_tap_into_min_depth():
    """k_depth_update / k_layer MODE 3: ``fmaxf(sacc, 0) + eps``, x0 normalised and clamped with fminf / fmaxf as in
    oracle.ddp_oracle.sample_depth - fed a NaN tap the result is finite: min_depth exactly, x0 = -bit_scale"""
    f = np.float32
    min_depth, max_depth, bit = f(1e-3), f(80.0), f(0.1)
    for sacc in (f('nan'), f(0.25)):
        pred = np.fmax(sacc, f(0)) + min_depth                                        # relu + eps, as fmaxf does it
        x0 = ((pred - min_depth) / (max_depth - min_depth) * f(2) - f(1)) * bit
        x0 = np.fmin(np.fmax(x0, -bit), bit)
        assert np.isfinite(pred) and np.isfinite(x0)
    assert np.fmax(f('nan'), f(0)) + min_depth == min_depth
    with torch.no_grad():                                                             # ... while the oracle's relu keeps the NaN
        assert torch.isnan(torch.relu(torch.tensor(float('nan'))) + 1e-3)


def test_strict_greater_argmax_never_picks_a_nan():
    row = np.array([0.5, np.nan, 2.0, 1.0, np.nan], dtype=np.float32)
    best, arg = row[0], 0
    for k in range(1, len(row)):
        if row[k] > best:                                                             # the kernels' strict '>'
            best, arg = row[k], k
    assert arg == 2 and best == 2.0
    hv, pred = np.float32('nan'), np.float32(3.5)
    assert (hv if hv > 0 else pred) == pred                                           # a NaN hint is "no hint"
    assert not (np.float32('nan') > np.float32(0.5))                                  # the BEV threshold: "absent"
    assert np.fmax(np.float32(-1.0), np.float32('nan')) == -1.0                       # fmaxf reductions skip it
