"""tests/support.py on the CPU: the one guard writer and its readback, the refusal check, round256 and the float64 measure.
The guard tests run on a stand-in engine whose workspace is host memory; no GPU and no library is involved."""
import pytest
import torch

import support
from support import GUARD, PATTERN


class _Engine:
    """what guard() touches of an engine: device, workspace, _workspace_bytes()"""

    def __init__(self, n=300, slack=0):
        self.device = torch.device('cpu')
        self.workspace = torch.zeros(n + slack)
        self._n = n

    def _workspace_bytes(self):
        return self._n * 4


@pytest.fixture(autouse=True)
def _aligned_host_memory(monkeypatch):
    """host allocations are 64-byte aligned; the device's are multiples of 256 bytes, which guard() asserts of the interior"""
    def alloc(n, dev):
        raw = torch.empty(n + 64, dtype=torch.float32, device=dev)
        skip = (-raw.data_ptr() % 256) // 4
        return raw[skip:skip + n]
    monkeypatch.setattr(support, '_alloc', alloc)


def _words(t):
    return t.view(torch.int32)


def test_guard_fills_interior_and_guards_and_keeps_the_size():
    eng = support.guard(_Engine())
    assert eng.workspace.numel() == 300 and eng.guarded.numel() == 300 + 2 * GUARD
    assert eng.workspace.data_ptr() == eng.guarded.data_ptr() + 4 * GUARD and eng.workspace.data_ptr() % 256 == 0
    assert bool((_words(eng.guarded) == PATTERN).all()) and bool(torch.isnan(eng.workspace).all())
    assert support.guards_ok(eng)
    support.assert_guards(eng, 'fresh')


def test_guard_exact_and_explicit_size():
    support.guard(_Engine(), exact=True)
    with pytest.raises(AssertionError):
        support.guard(_Engine(slack=64), exact=True)
    eng = support.guard(_Engine(slack=64), floats=300)                   # (FcnSamplerEngine: 64 floats of slack, the size is named)
    assert eng.workspace.numel() == 300 and support.guards_ok(eng)


def test_unaligned_interior_is_refused(monkeypatch):
    def alloc(n, dev):
        raw = torch.empty(n + 128, dtype=torch.float32, device=dev)
        skip = (-raw.data_ptr() % 256) // 4 + 16                         # 64 bytes off a multiple of 256
        return raw[skip:skip + n]
    monkeypatch.setattr(support, '_alloc', alloc)
    with pytest.raises(AssertionError):
        support.guard(_Engine())


@pytest.mark.parametrize('at,front,back', [(0, 1, 0), (GUARD - 1, 1, 0), (-GUARD, 0, 1), (-1, 0, 1)],
                         ids=['front-first', 'front-last', 'back-first', 'back-last'])
def test_one_word_at_each_guard_edge_is_seen(at, front, back):
    eng = support.guard(_Engine())
    _words(eng.guarded)[at] = 0
    assert not support.guards_ok(eng)
    with pytest.raises(AssertionError, match=f'edge: {front} words written in front of the workspace, {back} behind it'):
        support.assert_guards(eng, 'edge')


def test_interior_edges_are_not_guards():
    eng = support.guard(_Engine())
    eng.workspace[0] = 1.0
    eng.workspace[-1] = 2.0
    assert _words(eng.guarded)[GUARD] != PATTERN and _words(eng.guarded)[-GUARD - 1] != PATTERN
    assert support.guards_ok(eng)
    support.assert_guards(eng, 'interior')


def test_guarded_is_the_buffer_level_form():
    g = support.Guarded(4 * 77, torch.device('cpu'))
    assert g.ws.numel() == 77 and g.ptr() == g.ws.data_ptr() == g.guarded.data_ptr() + 4 * GUARD and support.guards_ok(g)
    _words(g.guarded)[-1] = 7
    with pytest.raises(AssertionError, match='0 words written in front of the workspace, 1 behind it'):
        support.assert_guards(g, 'buffer')
    with pytest.raises(AssertionError):
        support.Guarded(6, torch.device('cpu'))                         # not a whole number of floats


class _Lib:
    """both workspace queries refuse with ``rc`` and leave ``message`` as the last error"""

    def __init__(self, message, rc=-1):
        self.message, self.rc, self.calls = message, rc, 0

    def _query(self, cfg, n):
        self.calls += 1
        return self.rc

    ddp_query_workspace = ddp_query_const_workspace = _query

    def ddp_last_error(self):
        return self.message


def test_refused_wants_the_code_and_every_word():
    import ctypes as C
    cfg = C.c_int(0)
    stub = _Lib(b'DDP_FLAG_X0_HINTS: bev has no hints')
    support.refused(stub, cfg, 'DDP_FLAG_X0_HINTS', 'bev')
    assert stub.calls == 2                                               # both queries were asked
    support.refused(stub, cfg)
    with pytest.raises(AssertionError):
        support.refused(stub, cfg, 'DDP_FLAG_X0_HINTS', 'depth')         # one word missing
    with pytest.raises(AssertionError):
        support.refused(_Lib(b'DDP_FLAG_X0_HINTS: bev has no hints', rc=0), cfg, 'bev')      # accepted: not a refusal


def test_round256():
    assert [support.round256(n) for n in (0, 1, 255, 256, 257)] == [0, 256, 256, 256, 512]


def test_max_rel64_is_its_formula_in_float64():
    a = torch.tensor([1.0, 1.0 + 2.0 ** -23, 3.0], dtype=torch.float32)
    b = torch.tensor([1.0, 1.0, 3.0 + 2.0 ** -22], dtype=torch.float32)
    want = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    in_f32 = float((a - b).abs().max() / b.abs().max())
    assert support.max_rel64(a, b) == want and want != in_f32
    assert support.max_rel64(b, b) == 0.0


def test_constants():
    assert GUARD == 1024 and PATTERN == 0x7FC0BEEF and support.REL == 2e-4
    assert torch.isnan(torch.tensor([PATTERN], dtype=torch.int32).view(torch.float32)).all()
