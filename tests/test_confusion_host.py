"""CPU side of the device-side confusion matrix (tests/test_confusion_gpu.py runs the cases on an MI355X): the fixture recorded from
the reference's own ``calculate_confusion_matrix`` equals the numpy restatement of tests/confusion_cases.py; the case conditions
and the tally identity hold; the matrix contains the pre_eval counters; the library is a library of its own (its hash, its
exports, the other two untouched); every refusal happens before any launch; the host layer and the keyword surface.  No GPU
compute is invoked."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import confusion_cases as CC
import device_eval_cases as V
from ddp_amd import _cm_lib as M
from ddp_amd import _eval_lib as E
from ddp_amd import apis, build
from ddp_amd import confusion as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'device_eval')


@pytest.fixture(scope='module')
def cm_fix():
    return np.load(os.path.join(GOLDEN, 'cm_cases.npz'))


# ---- fixture = restatement -----------------------------------------------------------------------------------------------------------
def test_fixture_equals_the_restatement(cm_fix):
    cfg = json.loads(str(cm_fix['config']))
    cases = CC.in_range_cases()
    assert sorted(cfg) == sorted(cases) and len(cases) == 12
    for name, c in cases.items():
        assert cfg[name] == dict(K=c['K'], ignore_index=c['ignore_index'], n=len(c['preds']))
        for i, (p, l) in enumerate(zip(c['preds'], c['labels'])):
            assert np.array_equal(cm_fix[f'{name}/{i}/pred'], p) and np.array_equal(cm_fix[f'{name}/{i}/label'], l)
        ref = cm_fix[f'{name}/ref']
        m, t = CC.cm_case_expect(c)
        assert ref.dtype == np.float64 and ref.shape == (c['K'], c['K']) and str(cm_fix[f'{name}/ref_dtype']) == 'float64'
        assert np.array_equal(ref, m.astype(np.float64)), name
        assert t[2] == t[3] == 0 and t[0] == t[1] + m.sum()


def test_case_conditions():
    cases = CC.in_range_cases()
    assert sorted(cases) == sorted(f'k{K}_{kind}' for K in (2, 19, 150, 256) for kind in ('rand', 'block', 'mix'))
    assert (37 * 53) % 16 != 0 and 100 * 101 > CC.CM_TILE and 1 * 17 > 16 > 3 * 5
    for name, c in cases.items():
        K = c['K']
        assert [p.shape for p in c['preds']] == [(1, 1), (1, 17), (3, 5), (37, 53), (100, 101)] == [l.shape for l in c['labels']]
        assert c['ignore_index'] == 255 and c['reduce_zero_label'] is False
        lab = np.concatenate([l.reshape(-1) for l in c['labels']])
        prd = np.concatenate([p.reshape(-1) for p in c['preds']])
        # (a prediction copied from an ignored label is 255 itself: masked with its pixel)
        assert ((lab < K) | (lab == 255)).all() and (prd[lab != 255] < K).all() and (lab == 255).any()
        assert (lab != prd).any() and (lab == prd).any()
    # piecewise constant: the large map of a block case is made of 8 x 8 blocks
    l = cases['k19_block']['labels'][4]
    assert all((l[y:y + 8, x:x + 8] == l[y, x]).all() for y in range(0, 100, 8) for x in range(0, 101, 8))
    a = CC.all_keys()
    assert a['K'] == 256 and a['ignore_index'] == -1 and a['preds'][0].shape == (256, 256) and a['preds'][0].dtype == np.uint8
    assert (a['labels'][0] == np.arange(256)[:, None]).all() and (a['preds'][0] == np.arange(256)[None, :]).all()
    m, t = CC.cm_case_expect(a)
    assert (m == 1).all() and m.shape == (256, 256) and t.tolist() == [65536, 0, 0, 0]
    assert 256 * 256 // CC.CM_TILE == 8                  # eight blocks, each with CM_TILE distinct keys


def test_tally_identity_on_every_case():
    cases = dict(V.seg_cases(), **CC.in_range_cases(), all_keys=CC.all_keys())
    seen = np.zeros(4, dtype=np.int64)
    for name, c in cases.items():
        for p, l in zip(c['preds'], c['labels']):
            m, t = CC.cm_expect(p, l, c['K'], c['ignore_index'], c['reduce_zero_label'])
            assert t[0] == p.size == t[1] + t[2] + t[3] + m.sum() and (m >= 0).all() and (t >= 0).all(), name
            seen += t
    assert (seen > 0).all()                              # every kind of pixel occurs somewhere
    c = V.seg_cases()['all_ignored']
    m, t = CC.cm_case_expect(c)
    assert not m.any() and t[1] == t[0] == 37 * 53
    assert CC.cm_case_expect(V.seg_cases()['label_ge_k'])[1][2] > 100 and CC.cm_case_expect(V.seg_cases()['pred_ge_k'])[1][3] > 100
    m, t = CC.cm_case_expect(V.big_single_class())
    assert m[5, 5] == 2097152 == m.sum() == t[0]


def test_matrix_contains_the_pre_eval_counters():
    """diagonal = area_intersect, column sums = area_pred_label, row sums = area_label, wherever nothing is dropped"""
    for name, c in CC.in_range_cases().items():
        K = c['K']
        for p, l in zip(c['preds'], c['labels']):
            m, t = CC.cm_expect(p, l, K, c['ignore_index'], c['reduce_zero_label'])
            e = V.seg_expect(p, l, K, c['ignore_index'], c['reduce_zero_label'])
            assert np.array_equal(np.diag(m), e[0, :K]) and np.array_equal(m.sum(0), e[1, :K]) and np.array_equal(m.sum(1), e[2, :K]), name
    # and where pixels are dropped the column / row sums fall short by exactly those pixels
    c = V.seg_cases()['label_ge_k']
    m, t = CC.cm_case_expect(c)
    e = V.seg_case_expect(c)[0]
    assert e[1].sum() - m.sum() == t[2] > 0 and np.array_equal(np.diag(m), e[0, :19])


# ---- the library's own (what every side library shares: tests/test_build_host.py) ------------------------------------------------------
def test_binding_matches_the_header():
    build.SIDE['cm'].start(verbose=False)()
    header = open(os.path.join(ROOT, 'include', 'ddp_cm_mi355x.h')).read()
    # four functions and the item struct: the five names the header declares
    assert re.findall(r'typedef struct (\w+)', header) == ['ddp_cm_item'] and len(M.EXPORTS) + 1 == 5
    assert '#define DDP_CM_MAX_ITEMS 64' in header and M.MAX_ITEMS == 64 and '#define DDP_CM_TALLY 4' in header and M.TALLY == 4
    assert C.sizeof(M.Item) == 24 == C.sizeof(E.SegItem)
    assert (M.E_BADCFG, M.E_ALIGN, M.E_LAUNCH, M.E_NULL) == (E.E_BADCFG, E.E_ALIGN, E.E_LAUNCH, E.E_NULL)


def test_stale_or_missing_library_raises(tmp_path, monkeypatch):
    with pytest.raises(M.DdpCmError, match='not found'):
        M.load(str(tmp_path / 'libddp_cm.so'))
    monkeypatch.setattr(M._binding, 'libs', {})
    with monkeypatch.context() as m:
        m.setattr(build.SIDE['cm'], 'built_hash', lambda: 'feedfeedfeedfeed')
        with pytest.raises(M.DdpCmError, match='is stale'):
            M.load()
    monkeypatch.setattr(M._binding, 'abi_version', M.ABI_VERSION + 1)
    with pytest.raises(M.DdpCmError, match='ABI mismatch: library 1 vs binding 2') as e:
        M.load()
    assert e.value.code is None and isinstance(e.value, RuntimeError) and not M._binding.libs


FAKE = 0x1000     # a non-NULL "device pointer": every call below is refused before anything is enqueued


def _refused(rc, code, words):
    msg = M.load().ddp_cm_last_error().decode()
    assert rc == code and words in msg, (rc, msg)


def test_refusals_happen_before_any_launch():
    lib = M.load()
    one = (M.Item * 1)(M.Item(FAKE, FAKE, 4, 4))
    seg = lambda items, n, K=19, matrix=FAKE, tally=FAKE, acc=0: lib.ddp_cm_seg(items, n, K, 255, 0, acc, matrix, tally, None, None)
    for acc in (0, 1):
        _refused(seg(one, 1, K=1, acc=acc), M.E_BADCFG, 'num_classes 1 out of range [2,256]')
        _refused(seg(one, 1, K=257, acc=acc), M.E_BADCFG, 'num_classes 257')
        _refused(seg(one, 0, acc=acc), M.E_BADCFG, 'n_items 0')
        _refused(seg((M.Item * 65)(), 65, acc=acc), M.E_BADCFG, 'n_items 65')
        _refused(seg(None, 1, acc=acc), M.E_NULL, 'items is NULL')
        _refused(seg(one, 1, matrix=None, acc=acc), M.E_NULL, 'd_matrix')
        _refused(seg((M.Item * 1)(M.Item(FAKE, None, 4, 4)), 1, acc=acc), M.E_NULL, 'item 0')
        _refused(seg((M.Item * 2)(M.Item(FAKE, FAKE, 4, 4), M.Item(None, FAKE, 4, 4)), 2, acc=acc), M.E_NULL, 'item 1')
        for h, w in ((1 << 15, 1 << 16), (46341, 46341), (0, 5), (5, -1)):         # h * w >= 2^31; empty
            _refused(seg((M.Item * 1)(M.Item(FAKE, FAKE, h, w)), 1, acc=acc), M.E_BADCFG, 'h*w < 2^31')
        _refused(seg(one, 1, matrix=FAKE + 4, acc=acc), M.E_ALIGN, '8-byte')
        _refused(seg(one, 1, tally=FAKE + 4, acc=acc), M.E_ALIGN, '8-byte')
    nbytes = C.c_size_t(77)
    for K in (2, 19, 150, 256):
        assert lib.ddp_cm_workspace(K, C.byref(nbytes)) == 0 and nbytes.value == 0          # the block tables live in LDS
    _refused(lib.ddp_cm_workspace(1, C.byref(nbytes)), M.E_BADCFG, 'num_classes 1')
    _refused(lib.ddp_cm_workspace(257, C.byref(nbytes)), M.E_BADCFG, 'num_classes 257')
    _refused(lib.ddp_cm_workspace(19, None), M.E_NULL, 'bytes is NULL')
    with pytest.raises(M.DdpCmError, match='num_classes 1 out of range') as e:
        M.check(seg(one, 1, K=1), lib)
    assert e.value.code == M.E_BADCFG


# ---- host layer ----------------------------------------------------------------------------------------------------------------------
def test_normalized_and_totals_equal_numpy():
    c = CC.in_range_cases()['k19_mix']
    m, _ = CC.cm_case_expect(c)
    m = m.astype(np.float64)
    m[7] = 0                                             # a class without ground truth: a NaN row, as in the tool
    cm = cf.ConfusionMatrix(19)
    assert np.array_equal(cm.result(), np.zeros((19, 19))) and cm.result().dtype == np.float64 and cm.tally().tolist() == [0, 0, 0, 0]
    per_label_sums = m.sum(axis=1)[:, np.newaxis]        # confusion_matrix.py:89-91
    with np.errstate(invalid='ignore'):
        want = m.astype(np.float32) / per_label_sums * 100
    got = cm.normalized(m)
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and np.isnan(got[7]).all() and not np.isnan(got[:7]).any()
    assert np.array_equal(cf.normalize(m), want, equal_nan=True)
    i, u, p, l = cm.pre_eval_totals(m)
    assert np.array_equal(i, np.diag(m)) and np.array_equal(p, m.sum(0)) and np.array_equal(l, m.sum(1)) and np.array_equal(u, p + l - i)
    # on an in-range case they are the summed pre_eval entries
    m, _ = CC.cm_case_expect(c)
    e = V.seg_case_expect(c).sum(0)
    i, u, p, l = cf.totals_from_matrix(m)
    assert np.array_equal(i, e[0, :19]) and np.array_equal(p, e[1, :19]) and np.array_equal(l, e[2, :19]) and np.array_equal(u, (e[1] + e[2] - e[0])[:19])
    assert 'tally()[2] == tally()[3] == 0' in cf.ConfusionMatrix.pre_eval_totals.__doc__
    # the methods read the accumulator when no matrix is given
    cm.result = lambda: m.astype(np.float64)
    assert np.array_equal(cm.normalized(), cf.normalize(m), equal_nan=True) and np.array_equal(cm.pre_eval_totals()[0], i)


def test_input_checks_are_device_free():
    ok = np.zeros((4, 5), dtype=np.uint8)
    cm = cf.ConfusionMatrix(19, ignore_index=255, reduce_zero_label=True)
    assert (cm.num_classes, cm.ignore_index, cm.reduce_zero_label) == (19, 255, True)
    with pytest.raises(ValueError, match='outside the integers 0..255'):
        cm.update([ok], [np.full((4, 5), 300, dtype=np.int64)])
    with pytest.raises(ValueError, match='differ in shape'):
        cm.update([ok], [np.zeros((5, 4), dtype=np.uint8)])
    with pytest.raises(ValueError, match='1 predictions for 2'):
        cm.update([ok], [ok, ok])
    assert cm.update([], []) is cm and cm.tally().tolist() == [0, 0, 0, 0]
    cm.reset()
    for K in (1, 257):
        with pytest.raises(ValueError, match='out of range'):
            cf.ConfusionMatrix(K)


def test_keyword_surface():
    p = inspect.signature(apis.single_gpu_test).parameters
    assert p['confusion'].default is None and list(p)[-1] == 'confusion'
    assert 'confusion' not in inspect.signature(apis.multi_gpu_test).parameters and 'DistributedSampler' in apis.multi_gpu_test.__doc__
    p = inspect.signature(cf.seg_confusion).parameters
    assert list(p) == ['preds', 'labels', 'num_classes', 'ignore_index', 'reduce_zero_label', 'accumulate', 'out', 'tally']
    assert (p['ignore_index'].default, p['reduce_zero_label'].default, p['accumulate'].default, p['out'].default, p['tally'].default) == (255, False, False, None, None)
    p = inspect.signature(cf.ConfusionMatrix.__init__).parameters
    assert list(p)[1:] == ['num_classes', 'ignore_index', 'reduce_zero_label', 'device'] and p['ignore_index'].default == 255
    cm = cf.ConfusionMatrix(3)
    for kw in (dict(), dict(pre_eval=True), dict(format_only=True)):
        with pytest.raises(ValueError, match='confusion= requires device_eval=True'):
            apis.single_gpu_test(None, None, confusion=cm, **kw)
    with pytest.raises(ValueError, match='device_eval=True requires pre_eval=True'):
        apis.single_gpu_test(None, None, device_eval=True, confusion=cm)


def test_post_device_feeds_the_matrix_from_the_loaded_labels(monkeypatch):
    """device-free: with ``confusion=None`` the call is what it was; with a matrix, the labels are loaded once and both reductions
    get the same tensors"""
    from ddp_amd import evaluation as ev
    loads, seen = [], {}

    class DS:
        CLASSES = tuple('abc')
        ignore_index = 255
        reduce_zero_label = True

        def get_gt_seg_map_by_idx(self, i):
            loads.append(i)
            return np.full((2, 2), 10 + i, dtype=np.uint8)

    def fake_seg(preds, labels, k, ign, rzl):
        seen['pre_eval'] = labels
        return [('seg', int(p[0, 0]), int(l[0, 0])) for p, l in zip(preds, labels)]

    class FakeMatrix:
        num_classes, ignore_index, reduce_zero_label = 3, 255, True

        def update(self, preds, labels):
            seen['confusion'] = (preds, labels)

    monkeypatch.setattr(ev, 'seg_pre_eval', fake_seg)
    res = [torch.full((2, 2), j, dtype=torch.uint8) for j in range(3)]
    want = [('seg', 0, 14), ('seg', 1, 15), ('seg', 2, 16)]
    assert apis._post_device(DS(), res, [4, 5, 6], None) == want and loads == [4, 5, 6] and 'confusion' not in seen
    assert all(isinstance(l, np.ndarray) for l in seen['pre_eval'])              # confusion=None: the labels go on as they were loaded
    assert apis._post_device(DS(), res, [4, 5, 6], None, FakeMatrix()) == want and loads == [4, 5, 6, 4, 5, 6]
    preds, labels = seen['confusion']
    assert all(a is b for a, b in zip(preds, res)) and all(a is b for a, b in zip(labels, seen['pre_eval']))
    assert all(torch.is_tensor(l) and l.dtype == torch.uint8 for l in labels)
    other = FakeMatrix()
    other.num_classes = 4
    with pytest.raises(ValueError, match='the matrix was made for'):
        apis._post_device(DS(), res, [4, 5, 6], None, other)
    with pytest.raises(ValueError, match='no confusion matrix for depth'):
        apis._post_device(DS(), [torch.zeros(1, 2, 2)], [0], lambda ds, i: dict(gt=None, min_depth=0, max_depth=1), FakeMatrix())
