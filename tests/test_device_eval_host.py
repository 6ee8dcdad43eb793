"""CPU side of the device-side pre_eval statistics (tests/test_device_eval_gpu.py runs the cases on an MI355X): the fixtures recorded
from the reference's own functions equal the numpy restatements of tests/device_eval_cases.py; the case conditions hold; the
evaluation library is a library of its own (its hash, its exports, the product library untouched); every refusal happens before
any launch; the crop rectangles, the finalisation rules and the keyword surface.  No GPU compute is invoked."""
import ctypes as C
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

import device_eval_cases as V
from ddp_amd import _eval_lib as E
from ddp_amd import apis, build
from ddp_amd import evaluation as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'device_eval')
# the reference's float32 metrics against their fp64 values: pairwise float32 sums ((log2 n + 2) * 2^-24 of sum |term|, n <= 2^13)
# over terms that carry one float32 rounding of ln / log10 each, amplified by |ln g| / |ln g - ln p| <= 2^8 under the 2 % rule of
# the cases: 2^-24 * 2^8 * 2 = 2^-15 of the metric's scale
REF32_REL = 2.0 ** -15


@pytest.fixture(scope='module')
def seg_fix():
    return np.load(os.path.join(GOLDEN, 'eval_seg_cases.npz'))


@pytest.fixture(scope='module')
def depth_fix():
    return np.load(os.path.join(GOLDEN, 'eval_depth_cases.npz'))


# ---- fixtures = restatement ----------------------------------------------------------------------------------------------------------
def test_seg_fixtures_equal_the_restatement(seg_fix):
    cfg = json.loads(str(seg_fix['config']))
    cases = V.seg_cases()
    assert sorted(cfg) == sorted(cases)
    for name, c in cases.items():
        assert cfg[name] == dict(K=c['K'], ignore_index=c['ignore_index'], reduce_zero_label=c['reduce_zero_label'], n=len(c['preds']))
        exp = V.seg_case_expect(c)
        for i, (p, l) in enumerate(zip(c['preds'], c['labels'])):
            assert np.array_equal(seg_fix[f'{name}/{i}/pred'], p) and np.array_equal(seg_fix[f'{name}/{i}/label'], l)
            ref = seg_fix[f'{name}/{i}/ref'].astype(np.int64)              # intersect, union, pred, label of intersect_and_union
            K = c['K']
            assert np.array_equal(ref[0], exp[i, 0, :K]) and np.array_equal(ref[2], exp[i, 1, :K]) and np.array_equal(ref[3], exp[i, 2, :K]), (name, i)
            assert np.array_equal(ref[1], exp[i, 1, :K] + exp[i, 2, :K] - exp[i, 0, :K])
            assert not exp[i, :, K:].any()


def test_depth_fixtures_equal_the_restatement(depth_fix):
    cfg = json.loads(str(depth_fix['config']))
    cases = V.depth_cases()
    assert sorted(cfg) == sorted(V.FIXTURE_DEPTH) == sorted(cases)
    for name in V.FIXTURE_DEPTH:
        c = cases[name]
        assert cfg[name]['crops'] == [None if r is None else list(r) for r in c['crops']]
        for i, (p, g, crop) in enumerate(zip(c['preds'], c['gts'], c['crops'])):
            assert np.array_equal(depth_fix[f'{name}/{i}/pred'], p, equal_nan=True) and np.array_equal(depth_fix[f'{name}/{i}/gt'], g)
            ref = depth_fix[f'{name}/{i}/ref']
            # the line-by-line restatement of calculate() on float32 IS the reference (same numpy expressions)
            np.testing.assert_allclose(np.array(V.depth_ref32(p, g, crop)), ref, rtol=1e-6, atol=0, equal_nan=True, err_msg=f'{name}/{i}')
            # the header's columns, finalised in fp64, against the reference's float32 values
            cols, _ = V.depth_expect64(p, g, crop)
            fin = np.array(ev.depth_finalize(list(cols) + [0.0] * 6), dtype=np.float64)
            if cols[0] == 0:
                assert np.isnan(ref).all() and np.isnan(fin).all()
                continue
            assert np.array_equal(fin[:3], ref[:3]), (name, i)         # a1..a3: counts of fp32 comparisons, exact
            if name == 'nonpositive_pred':
                assert np.array_equal(np.isfinite(fin), np.isfinite(ref)) and np.array_equal(fin[np.isfinite(fin)] > 0, ref[np.isfinite(ref)] > 0)
                continue
            scales = V.depth_metric_scales(p, g, crop)
            for k, s in zip(range(3, 9), scales):
                if not math.isfinite(s):         # a single valid pixel: silog is the square root of a rounding residue (NaN -> 0 or ~0)
                    assert cols[0] == 1 and k == 7
                    continue
                assert abs(fin[k] - ref[k]) <= REF32_REL * s, (name, i, k, fin[k], ref[k])


def _evaluate_map(results, class_names):
    """bev/mmdet3d/datasets/nuscenes_dataset.py:492-524, restated (the module itself needs packages that are not installed)"""
    thresholds = torch.tensor([0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65])
    num_classes = len(class_names)
    num_thresholds = len(thresholds)
    tp = torch.zeros(num_classes, num_thresholds)
    fp = torch.zeros(num_classes, num_thresholds)
    fn = torch.zeros(num_classes, num_thresholds)
    for result in results:
        pred = result['masks_bev']
        label = result['gt_masks_bev']
        pred = pred.detach().reshape(num_classes, -1)
        label = label.detach().bool().reshape(num_classes, -1)
        pred = pred[:, :, None] >= thresholds
        label = label[:, :, None]
        tp += (pred & label).sum(dim=1)
        fp += (pred & ~label).sum(dim=1)
        fn += (~pred & label).sum(dim=1)
    ious = tp / (tp + fp + fn + 1e-7)
    metrics = {}
    for index, name in enumerate(class_names):
        metrics[f'map/{name}/iou@max'] = ious[index].max().item()
        for threshold, iou in zip(thresholds, ious[index]):
            metrics[f'map/{name}/iou@{threshold.item():.2f}'] = iou.item()
    metrics['map/mean/iou@max'] = ious.max(dim=1).values.mean().item()
    return metrics


def test_bev_restatement_and_metrics_equal_evaluate_map():
    c = V.bev_cases()['k6_p63_t7']
    names = ['drivable_area', 'ped_crossing', 'walkway', 'stop_line', 'carpark_area', 'divider']
    ref = _evaluate_map([dict(masks_bev=torch.from_numpy(p), gt_masks_bev=torch.from_numpy(g)) for p, g in zip(c['probs'], c['gts'])], names)
    counts = [V.bev_expect(p, g, c['thresholds']) for p, g in zip(c['probs'], c['gts'])]
    assert ev.bev_metrics(counts, names) == ref
    assert ev.BEV_THRESHOLDS == V.BEV_DEFAULT
    for c in V.bev_cases().values():
        for p, g in zip(c['probs'], c['gts']):
            e = V.bev_expect(p, g, c['thresholds'])
            n_lab = (g.reshape(g.shape[0], -1) != 0).sum(1)
            assert (e[..., 0] + e[..., 2] == n_lab[:, None]).all() and e.shape == (p.shape[0], len(c['thresholds']), 3)


# ---- the case conditions -------------------------------------------------------------------------------------------------------------
def test_seg_case_conditions():
    cs = V.seg_cases()
    assert V.SEG_PARAMS == [(K, i, r) for K in (2, 19, 150, 256) for i in (0, 200, 255) for r in (False, True)] and len(V.SEG_PARAMS) == 24
    assert 'k256_ign255_rzl0' in cs
    for kind in ('rand', 'block'):
        assert [p.shape for p in cs[f'shapes_{kind}']['preds']] == [(1, 1), (1, 17), (3, 5), (37, 53), (64, 64)]
    assert (37 * 53) % 16 != 0 and 1 * 17 > 16 > 3 * 5
    c = cs['all_ignored']
    assert (c['labels'][0] == c['ignore_index']).all() and not V.seg_case_expect(c).any()
    c = cs['label_ge_k']
    ge = (c['labels'][0] >= c['K']) & (c['labels'][0] != c['ignore_index'])
    assert ge.sum() > 100
    e = V.seg_case_expect(c)[0]
    assert e[1].sum() == (c['labels'][0] != 255).sum() > e[2].sum()        # such a pixel still counts its prediction
    c = cs['pred_ge_k']
    assert (c['preds'][0] >= c['K']).sum() > 100
    c = cs['mix64']
    assert len(c['preds']) == 64 == E.MAX_ITEMS and len({p.shape for p in c['preds']}) > 40 and c['reduce_zero_label']
    # piecewise constant means: 8 x 8 blocks
    b = V.block_map(np.random.default_rng(0), 24, 40, range(19))
    assert all((b[y:y + 8, x:x + 8] == b[y, x]).all() for y in range(0, 24, 8) for x in range(0, 40, 8))
    c = cs['alignment']
    assert c['offsets'] == [(0, 0), (5, 21), (3, 8), (15, 15)] and c['preds'][0].shape[1] % 2 == 1
    assert 5 % 16 == 21 % 16 and 3 % 16 != 8 % 16 and 100 * 101 + 5 > V.SEG_TILE        # a shared head across a block border; a disagreement
    c = cs['bands']
    assert c['preds'][0].shape == (40, 1024) and 40 * 1024 == 5 * V.SEG_TILE
    big = V.big_single_class()
    assert big['preds'][0].shape == (1024, 2048) and V.seg_case_expect(big)[0, :, 5].tolist() == [2097152] * 3
    # every parameter case holds all label kinds it has room for: classes, the ignore value, values >= K that are not ignored
    for K, ign, rzl in V.SEG_PARAMS:
        lab = np.concatenate([l.reshape(-1) for l in cs[f'k{K}_ign{ign}_rzl{int(rzl)}']['labels']])
        assert (lab == ign).any() and (lab < K).any()
        if K < 254:
            assert ((lab >= K) & (lab != ign)).any()


def test_depth_case_conditions():
    cs = dict(V.depth_cases(), kitti=V.kitti_case())
    assert [p.shape for p in cs['small_full']['preds']] == [(1, 1), (7, 9)] and cs['small_garg']['crops'] == [V.garg(7, 9)]
    assert cs['kitti']['preds'][0].shape == (352, 1216) and cs['kitti']['crops'] == [None, (143, 349, 43, 1172)]
    assert len({p.shape for p in cs['mixed_sizes']['preds']}) == 5 and 100 * 41 > V.DEPTH_TILE
    for name, c in cs.items():
        for p, g, crop in zip(c['preds'], c['gts'], c['crops']):
            gv, pv = V.depth_valid(p, g, crop)
            if name in ('empty_rect', 'all_invalid'):
                assert gv.size == 0
                continue
            assert gv.size > 0
            if name == 'nonpositive_pred':
                assert (pv <= 0).sum() == 2
                continue
            # every valid pred is bitwise its gt or >= 2 % away from it (what bounds |ln g| / |ln g - ln p| in the tolerance)
            same = pv.view(np.uint32) == gv.view(np.uint32)
            assert (same | (np.abs(pv.astype(np.float64) - gv) >= 0.02 * gv)).all(), name
            if gv.size > 50:
                assert same.any() and not same.all()
    p, g = cs['boundary']['preds'][0], cs['boundary']['gts'][0]
    r = np.maximum(g / p, p / g)[0]
    for b in V.RATIO_BOUNDS:
        b = np.float32(b)
        for v in (np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(4))):
            assert (r == v).sum() == 2
    assert np.float32(1.25) ** 2 == np.float32(1.5625) == 1.25 ** 2 and np.float32(1.953125) == 1.25 ** 3


def test_bev_case_conditions():
    cs = V.bev_cases()
    assert {c['probs'][0].shape[0] for c in cs.values()} == {1, 6, 32}
    assert {c['probs'][0][0].size for c in cs.values()} == {1, 63, 40000}
    assert {len(c['thresholds']) for c in cs.values()} == {1, 7, 16}
    t = cs['k32_p63_t16']['thresholds']
    assert list(t) != sorted(t) and list(t) != sorted(t, reverse=True)
    assert cs['k1_p1_t1']['probs'][0].reshape(-1)[0] == np.float32(0.35) and V.bev_expect(cs['k1_p1_t1']['probs'][0], cs['k1_p1_t1']['gts'][0], (0.35,)).tolist() == [[[1, 0, 0]]]
    assert float(np.float32(0.35)) != 0.35               # the comparison is a float32 one: thresholds are rounded first
    for c in cs.values():
        for p in c['probs']:
            for thr in np.asarray(c['thresholds'], dtype=np.float32)[:p[0].size]:
                assert (p == thr).any()


# ---- the library's own (what every side library shares: tests/test_build_host.py) ------------------------------------------------------
def test_binding_matches_the_header():
    build.SIDE['eval'].start(verbose=False)()
    header = open(os.path.join(ROOT, 'include', 'ddp_eval_mi355x.h')).read()
    assert '#define DDP_EVAL_MAX_ITEMS 64' in header and E.MAX_ITEMS == 64
    assert (C.sizeof(E.SegItem), C.sizeof(E.DepthItem), C.sizeof(E.BevItem)) == (24, 40, 16)


def test_stale_or_missing_library_raises(tmp_path, monkeypatch):
    with pytest.raises(E.DdpEvalError, match='not found'):
        E.load(str(tmp_path / 'libddp_eval.so'))
    monkeypatch.setattr(E._binding, 'libs', {})
    with monkeypatch.context() as m:
        m.setattr(build.SIDE['eval'], 'built_hash', lambda: 'feedfeedfeedfeed')
        with pytest.raises(E.DdpEvalError, match='is stale'):
            E.load()
    monkeypatch.setattr(E._binding, 'abi_version', E.ABI_VERSION + 1)
    with pytest.raises(E.DdpEvalError, match='ABI mismatch: library 1 vs binding 2') as e:
        E.load()
    assert e.value.code is None and isinstance(e.value, RuntimeError) and not E._binding.libs


FAKE = 0x1000     # a non-NULL "device pointer": every call below is refused before anything is enqueued


def _refused(rc, code, words):
    msg = E.load().ddp_eval_last_error().decode()
    assert rc == code and words in msg, (rc, msg)


def test_refusals_happen_before_any_launch():
    lib = E.load()
    one = (E.SegItem * 1)(E.SegItem(FAKE, FAKE, 4, 4))
    _refused(lib.ddp_eval_seg(one, 1, 1, 255, 0, FAKE, None), E.E_BADCFG, 'num_classes 1 out of range [2,256]')
    _refused(lib.ddp_eval_seg(one, 1, 257, 255, 0, FAKE, None), E.E_BADCFG, 'num_classes 257')
    _refused(lib.ddp_eval_seg(one, 0, 19, 255, 0, FAKE, None), E.E_BADCFG, 'n_items 0')
    _refused(lib.ddp_eval_seg((E.SegItem * 65)(), 65, 19, 255, 0, FAKE, None), E.E_BADCFG, 'n_items 65')
    _refused(lib.ddp_eval_seg(None, 1, 19, 255, 0, FAKE, None), E.E_NULL, 'items is NULL')
    _refused(lib.ddp_eval_seg(one, 1, 19, 255, 0, None, None), E.E_NULL, 'd_counts')
    _refused(lib.ddp_eval_seg((E.SegItem * 1)(E.SegItem(FAKE, None, 4, 4)), 1, 19, 255, 0, FAKE, None), E.E_NULL, 'item 0')
    for h, w in ((1 << 15, 1 << 16), (46341, 46341), (0, 5), (5, -1)):         # h * w >= 2^31; empty
        _refused(lib.ddp_eval_seg((E.SegItem * 1)(E.SegItem(FAKE, FAKE, h, w)), 1, 19, 255, 0, FAKE, None), E.E_BADCFG, 'h*w < 2^31')
    d = lambda *a: (E.DepthItem * 1)(E.DepthItem(FAKE, FAKE, *a))
    nbytes = C.c_size_t(0)
    assert lib.ddp_eval_depth_workspace(d(352, 1216, 0, 352, 0, 1216), 1, C.byref(nbytes)) == 0 and nbytes.value == 418 * 10 * 8
    assert ev.depth_workspace_bytes([(1, 1), (64, 64), (64, 65)]) == (1 + 4 + 5) * 80
    _refused(lib.ddp_eval_depth_workspace(d(1 << 15, 1 << 16, 0, 1, 0, 1), 1, C.byref(nbytes)), E.E_BADCFG, 'h*w < 2^31')
    _refused(lib.ddp_eval_depth(d(1 << 15, 1 << 16, 0, 1, 0, 1), 1, 1e-3, 80, FAKE, FAKE, None), E.E_BADCFG, 'h*w < 2^31')
    _refused(lib.ddp_eval_depth(d(7, 9, 0, 8, 0, 9), 1, 1e-3, 80, FAKE, FAKE, None), E.E_BADCFG, 'rectangle')
    _refused(lib.ddp_eval_depth(d(7, 9, 3, 2, 0, 9), 1, 1e-3, 80, FAKE, FAKE, None), E.E_BADCFG, 'rectangle')
    _refused(lib.ddp_eval_depth(d(7, 9, 0, 7, 0, 9), 1, 1e-3, 80, FAKE, None, None), E.E_NULL, 'd_workspace')
    _refused(lib.ddp_eval_depth(d(7, 9, 0, 7, 0, 9), 1, 1e-3, 80, FAKE + 4, FAKE, None), E.E_ALIGN, '8-byte')
    b = (E.BevItem * 1)(E.BevItem(FAKE, FAKE))
    thr = (C.c_float * 17)(*([0.5] * 17))
    _refused(lib.ddp_eval_bev(b, 1, 6, 40000, thr, 17, FAKE, None), E.E_BADCFG, 'n_thr 17')
    _refused(lib.ddp_eval_bev(b, 1, 6, 40000, thr, 0, FAKE, None), E.E_BADCFG, 'n_thr 0')
    _refused(lib.ddp_eval_bev(b, 1, 0, 40000, thr, 7, FAKE, None), E.E_BADCFG, 'num_classes 0')
    _refused(lib.ddp_eval_bev(b, 1, 6, 0, thr, 7, FAKE, None), E.E_BADCFG, 'n_pix 0')
    _refused(lib.ddp_eval_bev(b, 1, 6, 40000, None, 7, FAKE, None), E.E_NULL, 'thresholds')
    with pytest.raises(E.DdpEvalError, match='num_classes 1 out of range') as e:
        E.check(lib.ddp_eval_seg(one, 1, 1, 255, 0, FAKE, None), lib)
    assert e.value.code == E.E_BADCFG


# ---- host layer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(352, 1216), (375, 1242), (7, 9), (100, 41)])
def test_crops_equal_the_reference_slices(h, w):
    gt_height, gt_width = h, w
    garg, eigen = np.zeros((h, w)), np.zeros((h, w))
    garg[int(0.40810811 * gt_height):int(0.99189189 * gt_height), int(0.03594771 * gt_width):int(0.96405229 * gt_width)] = 1      # kitti.py:246-247
    eigen[int(0.3324324 * gt_height):int(0.91351351 * gt_height), int(0.0359477 * gt_width):int(0.96405229 * gt_width)] = 1       # kitti.py:250-251
    for fn, ref in ((ev.garg_crop, garg), (ev.eigen_crop, eigen)):
        y0, y1, x0, x1 = fn(h, w)
        m = np.zeros((h, w))
        m[y0:y1, x0:x1] = 1
        assert np.array_equal(m, ref) and 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w
    assert ev.garg_crop(h, w) == V.garg(h, w)


def test_finalisation_rules():
    assert all(math.isnan(v) for v in ev.depth_finalize([0.0] * 16)) and len(ev.depth_finalize([0.0] * 16)) == 9
    # one pixel: mean(err^2) - mean(err)^2 is a rounding residue; a negative one gives NaN in the reference -> 0
    row = [1.0, 1, 1, 1, 0.1, 0.01, 0.05, 0.3 ** 2 * (1 - 2 ** -50), -0.3, 0.001] + [0.0] * 6
    out = ev.depth_finalize(row)
    assert out[7] == 0 and out[:3] == (1.0, 1.0, 1.0) and out[3] == 0.1 and out[4] == math.sqrt(0.01) and out[8] == 0.001
    row = [4.0, 4, 3, 2, 0.4, 1.0, 0.2, 0.5, -0.4, 0.08] + [0.0] * 6
    assert ev.depth_finalize(row) == (1.0, 0.75, 0.5, 0.1, 0.5, 0.05, math.sqrt(0.125), math.sqrt(0.125 - 0.01) * 100, 0.02)
    nan = ev.depth_finalize([2.0, 0, 0, 0, 1.0, 1.0, float('nan'), float('nan'), float('nan'), 1.0] + [0.0] * 6)
    assert math.isnan(nan[5]) and math.isnan(nan[6]) and nan[7] == 0


def test_input_checks_are_device_free():
    ok = np.zeros((4, 5), dtype=np.uint8)
    with pytest.raises(ValueError, match='outside the integers 0..255'):
        ev.seg_pre_eval([ok], [np.full((4, 5), 300, dtype=np.int64)], 19)
    with pytest.raises(ValueError, match='outside the integers 0..255'):
        ev.seg_pre_eval([torch.full((4, 5), -1, dtype=torch.int32)], [ok], 19)
    with pytest.raises(ValueError, match='differ in shape'):
        ev.seg_pre_eval([ok], [np.zeros((5, 4), dtype=np.uint8)], 19)
    with pytest.raises(ValueError, match='1 predictions for 2'):
        ev.seg_pre_eval([ok], [ok, ok], 19)
    with pytest.raises(ValueError, match='differ in shape'):
        ev.depth_pre_eval([np.zeros((1, 4, 5), dtype=np.float32)], [np.zeros((4, 6), dtype=np.float32)], 1e-3, 80)
    with pytest.raises(ValueError, match='float32'):
        ev.depth_pre_eval([np.zeros((4, 5))], [np.zeros((4, 5), dtype=np.float32)], 1e-3, 80)
    assert ev.seg_pre_eval([], [], 19) == [] and ev.depth_pre_eval([], [], 1e-3, 80) == [] and ev.bev_pre_eval([], []) == []


def test_keyword_surface():
    from ddp_amd.depther.ddp import DDP as DepthDDP
    from ddp_amd.segmentors.ddp import DDP as SegDDP
    for cls, names in ((SegDDP, ('simple_test', 'aug_test', 'forward')), (DepthDDP, ('simple_test', 'aug_test'))):
        for n in names:
            p = inspect.signature(getattr(cls, n)).parameters
            assert p['on_device'].default is False, (cls, n)
    for fn in (apis.single_gpu_test, apis.multi_gpu_test):
        p = inspect.signature(fn).parameters
        assert p['device_eval'].default is False and p['gt_loader'].default is None and p['pre_eval'].default is False
    # the default return value: int64 host arrays; on_device: the uint8 maps themselves
    seg = torch.arange(24, dtype=torch.uint8).reshape(2, 3, 4)
    host = SegDDP._deliver(seg, False)
    assert len(host) == 2 and all(isinstance(a, np.ndarray) and a.dtype == np.int64 and a.shape == (3, 4) for a in host)
    dev = SegDDP._deliver(seg, True)
    assert len(dev) == 2 and all(torch.is_tensor(t) and t.dtype == torch.uint8 and t.data_ptr() == seg[i].data_ptr() for i, t in enumerate(dev))
    assert SegDDP._deliver(seg.to(torch.int64), True)[1].dtype == torch.uint8


def test_device_eval_requires_pre_eval():
    for fn in (apis.single_gpu_test, apis.multi_gpu_test):
        with pytest.raises(ValueError, match='device_eval=True requires pre_eval=True'):
            fn(None, None, device_eval=True)
        with pytest.raises(ValueError, match='device_eval=True requires pre_eval=True'):
            fn(None, None, format_only=True, device_eval=True)


def test_post_device_routes_by_ground_truth(monkeypatch):
    """device-free: the harness fetches the ground truth per index, groups by configuration and keeps dataset order"""
    calls = []

    def fake_seg(preds, labels, k, ign, rzl):
        calls.append((k, ign, rzl, [int(l[0, 0]) for l in labels]))
        return [('seg', int(p[0, 0]), int(l[0, 0])) for p, l in zip(preds, labels)]

    monkeypatch.setattr(ev, 'seg_pre_eval', fake_seg)

    class DS:
        CLASSES = tuple('abc')
        ignore_index = 255
        reduce_zero_label = True

        def get_gt_seg_map_by_idx(self, i):
            return np.full((2, 2), 10 + i, dtype=np.uint8)

    res = [torch.full((2, 2), j, dtype=torch.uint8) for j in range(3)]
    assert apis._post_device(DS(), res, [4, 5, 6], None) == [('seg', 0, 14), ('seg', 1, 15), ('seg', 2, 16)]
    assert calls == [(3, 255, True, [14, 15, 16])]
    assert apis.seg_gt_loader(DS(), 2)['num_classes'] == 3
    with pytest.raises(ValueError, match='needs gt_loader'):
        apis._post_device(DS(), [torch.zeros(1, 2, 2)], [0], None)
    with pytest.raises(TypeError, match='on_device'):
        apis._post_device(DS(), [np.zeros((2, 2))], [0], None)
    seen = []

    def fake_depth(preds, gts, lo, hi, crops=None):
        seen.append((lo, hi, crops))
        return [('depth', float(g[0, 0])) for g in gts]

    monkeypatch.setattr(ev, 'depth_pre_eval', fake_depth)
    loader = lambda ds, i: dict(gt=np.full((2, 2), float(i), dtype=np.float32), crop=(0, 1, 0, 2) if i else None, min_depth=1e-3, max_depth=80 if i < 2 else 10)
    out = apis._post_device(DS(), [torch.zeros(1, 2, 2) for _ in range(3)], [0, 1, 2], loader)
    assert out == [('depth', 0.0), ('depth', 1.0), ('depth', 2.0)] and seen == [(1e-3, 80.0, [None, (0, 1, 0, 2)]), (1e-3, 10.0, [(0, 1, 0, 2)])]
