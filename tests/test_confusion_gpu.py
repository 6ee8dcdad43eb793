"""The device-side confusion matrix on an MI355X (include/ddp_cm_mi355x.h, ddp_amd/confusion.py): matrix and tally are exact - equal
to the numpy restatement of tests/confusion_cases.py - on every case of the evaluation library's seg kernel, on the full-size
single-class map, on ``all_keys`` (every bin of the 256 x 256 matrix once: each block overflows its table) and on the fixture
cases, where they equal what the reference's own ``calculate_confusion_matrix`` returned.  Every output buffer is exactly sized
and guarded.  Accumulation, reproducibility, item order, a replayed graph, the evaluation library's counters inside the matrix,
and the harness end to end."""
import json
import os

import numpy as np
import pytest
import torch

import confusion_cases as CC
import device_eval_cases as V
from ddp_amd import _cm_lib as M
from ddp_amd import confusion as cf
from ddp_amd import evaluation as ev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'device_eval')
SEG_NAMES = list(V.seg_cases())
IN_RANGE_NAMES = list(CC.in_range_cases())
SENTINEL = -7
GUARD, _seg_dev, _Backbone = V.GUARD, V.seg_dev, V.PerImageBackbone


def _guarded(n_elem):
    buf = torch.full((n_elem + 2 * GUARD,), SENTINEL, dtype=torch.int64, device='cuda')
    return buf, buf[GUARD:GUARD + n_elem]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _run(case, P=None, L=None, accumulate=False, into=None):
    """one call into exactly sized, guarded buffers -> (matrix, tally) int64 arrays; ``into``: the (mbuf, m, tbuf, t) of an
    earlier call, to accumulate on"""
    if P is None:
        P, L = _seg_dev(case)
    K = case['K']
    mbuf, m, tbuf, t = into or (_guarded(K * K) + _guarded(M.TALLY))
    out = cf.seg_confusion(P, L, K, case['ignore_index'], case['reduce_zero_label'], accumulate=accumulate, out=m.view(K, K), tally=t)
    assert out.data_ptr() == m.data_ptr() and out.dtype == torch.int64 and out.shape == (K, K)
    torch.cuda.synchronize()
    assert _guards_intact(mbuf) and _guards_intact(tbuf)
    return m.view(K, K).cpu().numpy(), t.cpu().numpy()


def _assert_exact(got, want, what):
    (gm, gt), (wm, wt) = got, want
    assert gm.shape == wm.shape and np.array_equal(gm, wm), (what, np.argwhere(gm != wm)[:8])
    assert np.array_equal(gt, wt), (what, gt, wt)
    assert gt[0] == gt[1] + gt[2] + gt[3] + gm.sum()


# ---- exactness -----------------------------------------------------------------------------------------------------------------------
def test_every_eval_seg_case_is_exact():
    """all 24 K x ignore x rzl combinations, the small shapes, all_ignored, label_ge_k, pred_ge_k, mix64, alignment, bands: one
    test for all of them (every case is a few launches on small maps); a failure names its case"""
    assert len(SEG_NAMES) == 24 + 8
    for name in SEG_NAMES:
        case = V.seg_cases()[name]
        _assert_exact(_run(case), CC.cm_case_expect(case), name)


def test_single_class_full_size():
    case = V.big_single_class()
    m, t = _run(case)
    _assert_exact((m, t), CC.cm_case_expect(case), 'big_single_class')
    assert m[5, 5] == 2097152 == m.sum() and t.tolist() == [2097152, 0, 0, 0]


def test_all_keys_overflows_every_block_table_and_stays_exact():
    case = CC.all_keys()
    m, t = _run(case)
    assert (m == 1).all() and t.tolist() == [65536, 0, 0, 0]
    _assert_exact((m, t), CC.cm_case_expect(case), 'all_keys')


def test_calls_large_enough_for_the_wider_tiles():
    """more than 2048 blocks: the tile is 2 x, 4 x, 8 x; the same full-size pair (its head 5 bytes off a 16-byte boundary) given
    9, 17 and 33 times, and once alone"""
    p, l, wm, wt = CC.full_size_mix()
    case = dict(preds=[p], labels=[l], K=150, ignore_index=255, reduce_zero_label=True, offsets=[(5, 21)])
    P, L = _seg_dev(case)
    assert (P[0].data_ptr() % 16, L[0].data_ptr() % 16) == (5, 5)
    _assert_exact(_run(case, P, L), (wm, wt), 'alone')
    for n in CC.SCALED_ITEMS:
        assert (n - 1) * p.size // CC.CM_TILE <= CC.CM_BLOCKS_FULL * (n - 1) // 8 < n * p.size // CC.CM_TILE
        _assert_exact(_run(case, P * n, L * n), (n * wm, n * wt), n)


def test_fixture_cases_equal_the_reference():
    fix = np.load(os.path.join(GOLDEN, 'cm_cases.npz'))
    cfg = json.loads(str(fix['config']))
    assert len(IN_RANGE_NAMES) == 12
    for name in IN_RANGE_NAMES:
        case = CC.in_range_cases()[name]
        assert cfg[name]['K'] == case['K']
        m, t = _run(case)
        _assert_exact((m, t), CC.cm_case_expect(case), name)
        ref = fix[f'{name}/ref']
        assert np.array_equal(m.astype(np.float64), ref), name             # what calculate_confusion_matrix returned
        assert t[2] == t[3] == 0 and t[0] == sum(p.size for p in case['preds']), name


def test_no_tally_and_an_allocated_matrix():
    case = CC.in_range_cases()['k150_mix']
    P, L = _seg_dev(case)
    out = cf.seg_confusion(P, L, 150, 255)
    assert out.dtype == torch.int64 and out.shape == (150, 150) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), CC.cm_case_expect(case)[0])


# ---- accumulation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['k19_mix', 'k150_block', 'k256_rand'])
def test_three_accumulating_calls_equal_one_call_and_the_sum_of_three(name):
    case = CC.in_range_cases()[name]
    P, L = _seg_dev(case)
    parts = [(0, 2), (2, 3), (3, 5)]
    one = _run(case, P, L)
    bufs = _guarded(case['K'] ** 2) + _guarded(M.TALLY)
    for i, (a, b) in enumerate(parts):
        acc = _run(case, P[a:b], L[a:b], accumulate=i > 0, into=bufs)       # the first call zeroes the sentinel-filled buffers
    zeroing = [_run(case, P[a:b], L[a:b]) for a, b in parts]
    _assert_exact(acc, one, name)
    _assert_exact((sum(m for m, _ in zeroing), sum(t for _, t in zeroing)), one, name)
    _assert_exact(one, CC.cm_case_expect(case), name)
    # and an accumulating call on top of a full one doubles it
    twice = _run(case, P, L, accumulate=True, into=bufs)
    assert np.array_equal(twice[0], 2 * one[0]) and np.array_equal(twice[1], 2 * one[1])


def test_a_zeroing_call_overwrites_a_buffer_of_ff_bytes():
    case = V.seg_cases()['mix64']
    K = case['K']
    bufs = _guarded(K * K) + _guarded(M.TALLY)
    for b in (bufs[1], bufs[3]):
        b.view(torch.uint8).fill_(0xFF)
    _assert_exact(_run(case, into=bufs), CC.cm_case_expect(case), 'mix64')


def test_counters_pass_2_to_the_32():
    """64-bit counters: accumulate onto a bin that already holds 2^32 - 1"""
    case = V.big_single_class()
    P, L = _seg_dev(case)
    bufs = _guarded(19 * 19) + _guarded(M.TALLY)
    bufs[1].zero_()
    bufs[3].zero_()
    bufs[1][5 * 19 + 5] = 2 ** 32 - 1
    bufs[3][0] = 2 ** 32 - 1
    m, t = _run(case, P, L, accumulate=True, into=bufs)
    assert m[5, 5] == 2 ** 32 - 1 + 2097152 and m.sum() == m[5, 5] and t.tolist() == [2 ** 32 - 1 + 2097152, 0, 0, 0]


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------
def test_reruns_are_bit_identical_and_item_order_does_not_matter():
    for case in (V.seg_cases()['mix64'], CC.all_keys(), CC.in_range_cases()['k256_mix']):
        P, L = _seg_dev(case)
        a, b = _run(case, P, L), _run(case, P, L)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        perm = np.random.default_rng(3).permutation(len(P))
        c = _run(case, [P[i] for i in perm], [L[i] for i in perm])
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_a_replayed_graph_follows_the_rewritten_maps():
    case = V.seg_cases()['shapes_block']
    P, L = _seg_dev(case)
    K = case['K']
    mbuf, m = _guarded(K * K)
    tbuf, t = _guarded(M.TALLY)

    def enqueue():      # a zeroing call and an accumulating one: twice the matrix
        cf.seg_confusion(P, L, K, case['ignore_index'], case['reduce_zero_label'], out=m.view(K, K), tally=t)
        cf.seg_confusion(P, L, K, case['ignore_index'], case['reduce_zero_label'], accumulate=True, out=m.view(K, K), tally=t)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    wm, wt = CC.cm_case_expect(case)
    assert np.array_equal(m.view(K, K).cpu().numpy(), 2 * wm) and np.array_equal(t.cpu().numpy(), 2 * wt)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    P[3].copy_(P[3].flip(0)), L[3].copy_(L[3].flip(1)), L[4].fill_(255)
    m.fill_(-1), t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    now = dict(case, preds=[p.cpu().numpy() for p in P], labels=[l.cpu().numpy() for l in L])
    nm, nt = CC.cm_case_expect(now)
    assert not np.array_equal(nm, wm) and nt[1] > wt[1]
    assert np.array_equal(m.view(K, K).cpu().numpy(), 2 * nm) and np.array_equal(t.cpu().numpy(), 2 * nt)
    assert _guards_intact(mbuf) and _guards_intact(tbuf)


# ---- the evaluation library's counters are inside the matrix ------------------------------------------------------------------------
def test_diagonal_and_sums_equal_ddp_eval_seg():
    for name in IN_RANGE_NAMES:
        case = CC.in_range_cases()[name]
        K = case['K']
        P, L = _seg_dev(case)
        m, t = _run(case, P, L)
        counts = ev.seg_counts(P, L, K, case['ignore_index'], case['reduce_zero_label']).cpu().numpy().astype(np.int64).sum(0)
        assert np.array_equal(np.diag(m), counts[0, :K]) and np.array_equal(m.sum(0), counts[1, :K]) and np.array_equal(m.sum(1), counts[2, :K]), name
        i, u, p, l = cf.totals_from_matrix(m)
        assert np.array_equal(u, (counts[1] + counts[2] - counts[0])[:K]), name


# ---- host layer ----------------------------------------------------------------------------------------------------------------------
def test_confusion_matrix_accumulates_in_chunks_from_host_labels():
    case = V.seg_cases()['mix64']
    P = [torch.from_numpy(p).cuda() for p in case['preds']]
    # labels as a loader hands them over: host arrays, every other one an int64 tensor
    L = [l if i % 2 else torch.from_numpy(l.astype(np.int64)) for i, l in enumerate(case['labels'])]
    cm = cf.ConfusionMatrix(150, 255, True)
    assert cm.update(P + P[:7], L + L[:7]) is cm                         # 71 images: two calls
    wm, wt = CC.cm_case_expect(case)
    em, et = CC.cm_case_expect(dict(case, preds=case['preds'][:7], labels=case['labels'][:7]))
    res = cm.result()
    assert res.dtype == np.float64 and res.shape == (150, 150) and np.array_equal(res, (wm + em).astype(np.float64))
    assert cm.tally().dtype == np.int64 and np.array_equal(cm.tally(), wt + et)
    cm.update(P[:7], L[:7])
    assert np.array_equal(cm.result(), (wm + 2 * em).astype(np.float64))
    assert np.array_equal(cm.normalized(), cf.normalize((wm + 2 * em).astype(np.float64)), equal_nan=True)
    cm.reset()
    assert not cm.result().any() and not cm.tally().any()
    cm.update(P[:7], L[:7])
    assert np.array_equal(cm.result(), em.astype(np.float64)) and np.array_equal(cm.tally(), et)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _calculate_confusion_matrix(n, ignore_index, gt_maps, results):
    """segmentation/tools/confusion_matrix.py:53-68, restated"""
    confusion_matrix = np.zeros(shape=[n, n])
    for gt_segm, res_segm in zip(gt_maps, results):
        gt_segm = gt_segm.astype(int)
        gt_segm, res_segm = gt_segm.flatten(), res_segm.flatten()
        to_ignore = gt_segm == ignore_index
        gt_segm, res_segm = gt_segm[~to_ignore], res_segm[~to_ignore]
        inds = n * gt_segm + res_segm
        mat = np.bincount(inds, minlength=n**2).reshape(n, n)
        confusion_matrix += mat
    return confusion_matrix


def test_harness_accumulates_the_matrix_of_the_host_path():
    from golden_util import load_case
    from support import seg_model as _seg_model
    from ddp_amd import apis
    cfg, sd, x, _, _, _ = load_case('seg_ade_k3')
    model = _seg_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    model.backbone = _Backbone(x.cuda())
    H, W = cfg['h'] * 4, cfg['w'] * 4
    K = cfg['num_classes']
    oris = [(H + 5, W + 3), (H - 7, W + 9), (H, W), (2 * H + 1, W - 5), (H + 5, W + 3)]
    metas = [dict(img_shape=(H - (i % 2) * 2, W - (i % 3) * 4, 3), ori_shape=o + (3,), flip=i % 2 == 1, flip_direction='horizontal')
             for i, o in enumerate(oris)]
    rng = np.random.default_rng(5)

    class DS(torch.utils.data.Dataset):
        CLASSES = tuple(f'c{i}' for i in range(K))
        ignore_index = 255
        reduce_zero_label = True
        labels = [V.block_map(rng, o[0], o[1], list(range(K + 1)) + [255]) for o in oris]

        def __len__(self):
            return 5

        def __getitem__(self, i):
            return i

        def get_gt_seg_map_by_idx(self, i):
            return self.labels[i]

    def collate(idx):
        return dict(img=[torch.zeros(len(idx), 3, H, W)], img_metas=[[metas[i] for i in idx]])

    loader = torch.utils.data.DataLoader(DS(), batch_size=2, shuffle=False, collate_fn=collate)
    torch.manual_seed(3)
    host = apis.single_gpu_test(model, loader)                           # the maps the tool unpickles
    torch.manual_seed(3)
    plain = apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True)
    cm = cf.ConfusionMatrix(K, 255, True)
    torch.manual_seed(3)
    with_cm = apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True, confusion=cm)
    assert len(host) == len(plain) == len(with_cm) == 5
    for a, b in zip(plain, with_cm):                                     # the returned pre_eval list: unchanged
        assert len(a) == len(b) == 4 and all(s.dtype == t.dtype and torch.equal(s, t) for s, t in zip(a, b))
    # the tool on the host path's results; its loader hands over labels with reduce_zero_label applied
    reduced = [np.where((l == 0) | (l == 255), 255, l.astype(np.int64) - 1) for l in DS.labels]
    want = _calculate_confusion_matrix(K, 255, reduced, host)
    got = cm.result()
    assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want) and got.sum() > 0
    em = sum(CC.cm_expect(h.astype(np.uint8), l, K, 255, True)[0] for h, l in zip(host, DS.labels))
    assert np.array_equal(got, em.astype(np.float64))
    t = cm.tally()
    assert t[0] == sum(l.size for l in DS.labels) == t[1] + got.sum() and t[2] == t[3] == 0
    # and its totals are the summed pre_eval entries
    for k, tot in enumerate(cm.pre_eval_totals()):
        assert np.array_equal(tot, sum(e[k].numpy().astype(np.float64) for e in plain)), k
    with pytest.raises(ValueError, match='the matrix was made for'):
        apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True, confusion=cf.ConfusionMatrix(K, 255, False))
