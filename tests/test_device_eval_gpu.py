"""The device-side pre_eval statistics on an MI355X (include/ddp_eval_mi355x.h, ddp_amd/evaluation.py): the cases of
tests/device_eval_cases.py.  seg and bev counters are exact; depth counts are exact and the fp64 sums are within
2^-40 * sum |term| of numpy's fp64 evaluation (a few fp64 ulps per term, amplified by at most |ln g| / |ln g - ln p| <= 2^8 under
the 2 % rule of the cases, plus a tree sum over <= 2^21 terms); the final metrics obey the triangle inequality with the
reference's own float32 distance from fp64.  Reproducibility, guarded buffers, a replayed graph, and the harness end to end.
(DESIGN.md "Device evaluation" records the largest observed ratio of a depth sum.)"""
import os

import numpy as np
import pytest
import torch

import device_eval_cases as V
from ddp_amd import evaluation as ev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'device_eval')
SEG_NAMES = list(V.seg_cases())
DEPTH_NAMES = V.FIXTURE_DEPTH + ['kitti']
BEV_NAMES = list(V.bev_cases())
GUARD, _seg_dev, _Backbone = V.GUARD, V.seg_dev, V.PerImageBackbone


def _seg_run(case, P=None, L=None, out=None):
    if P is None:
        P, L = _seg_dev(case)
    return ev.seg_counts(P, L, case['K'], case['ignore_index'], case['reduce_zero_label'], out=out)


def _depth_case(name):
    return V.kitti_case() if name == 'kitti' else V.depth_cases()[name]


def _depth_dev(case):
    return [torch.from_numpy(p).cuda() for p in case['preds']], [torch.from_numpy(g).cuda() for g in case['gts']]


def _depth_run(case, **kw):
    P, G = _depth_dev(case)
    return ev.depth_sums(P, G, V.MIN_DEPTH, V.MAX_DEPTH, case['crops'], **kw)


def _bev_dev(case):
    return [torch.from_numpy(p).cuda() for p in case['probs']], [torch.from_numpy(g).cuda() for g in case['gts']]


# ---- seg ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SEG_NAMES)
def test_seg_counters_are_exact(name):
    case = V.seg_cases()[name]
    got = _seg_run(case).cpu().numpy().astype(np.int64)
    exp = V.seg_case_expect(case)
    assert got.shape == exp.shape and np.array_equal(got, exp), np.argwhere(got != exp)[:8]


def test_seg_single_class_full_size():
    case = V.big_single_class()
    got = _seg_run(case).cpu().numpy().astype(np.int64)
    assert np.array_equal(got, V.seg_case_expect(case)) and got[0, :, 5].tolist() == [2097152] * 3 and got.sum() == 3 * 2097152


def test_seg_pre_eval_returns_the_reference_tuples():
    fix = np.load(os.path.join(GOLDEN, 'eval_seg_cases.npz'))
    for name in ('k150_ign255_rzl1', 'k256_ign255_rzl0', 'k19_ign0_rzl1', 'mix64'):
        case = V.seg_cases()[name]
        P = [torch.from_numpy(p).cuda() for p in case['preds']]
        # labels as the loader hands them over: host arrays (uploaded); one as an int64 tensor
        L = [l if i % 2 else torch.from_numpy(l.astype(np.int64)) for i, l in enumerate(case['labels'])]
        res = ev.seg_pre_eval(P, L, case['K'], case['ignore_index'], case['reduce_zero_label'])
        assert len(res) == len(P)
        for i, tup in enumerate(res):
            ref = fix[f'{name}/{i}/ref']
            assert len(tup) == 4 and all(t.dtype == torch.float32 and t.device.type == 'cpu' and t.shape == (case['K'],) for t in tup)
            assert all(np.array_equal(t.numpy(), r) for t, r in zip(tup, ref)), (name, i)
    # more than 64 images: chunks, one counter block
    case = V.seg_cases()['mix64']
    P = [torch.from_numpy(p).cuda() for p in case['preds']]
    res = ev.seg_pre_eval(P + P[:7], case['labels'] + case['labels'][:7], 150, 255, True)
    assert len(res) == 71 and all(torch.equal(a, b) for j in range(7) for a, b in zip(res[64 + j], res[j]))


# ---- depth -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', DEPTH_NAMES)
def test_depth_counts_sums_and_metrics(name):
    case = _depth_case(name)
    got = _depth_run(case).cpu().numpy()
    fix = np.load(os.path.join(GOLDEN, 'eval_depth_cases.npz')) if name != 'kitti' else None
    assert got.shape == (len(case['preds']), 16) and not got[:, 10:].any()
    worst = 0.0
    for i, (p, g, crop) in enumerate(zip(case['preds'], case['gts'], case['crops'])):
        cols, mags = V.depth_expect64(p, g, crop)
        print(f'{name}/{i}: n {cols[0]:.0f} counts {cols[1:4]}')
        assert np.array_equal(got[i, :4], cols[:4]), (name, i, got[i, :4], cols[:4])             # n and the ratio counts: exact
        for k in range(6):
            d, e = got[i, 4 + k], cols[4 + k]
            if not np.isfinite(e):
                assert (np.isnan(d) and np.isnan(e)) or d == e, (name, i, k, d, e)         # the NaN / inf the reference gives
                continue
            ratio = abs(d - e) / mags[k] if mags[k] else abs(d - e)
            print(f'{name}/{i} column {4 + k}: device {d!r} fp64 {e!r} |diff| / sum|term| {ratio:.3e}')
            worst = max(worst, ratio)
            assert abs(d - e) <= V.SUM_REL * mags[k], (name, i, k, d, e, mags[k])
        # the final metrics against the reference's float32 values
        fin = ev.depth_finalize(got[i])
        ref = fix[f'{name}/{i}/ref'] if fix is not None else np.array(V.depth_ref32(p, g, crop))
        if cols[0] == 0:
            assert all(np.isnan(v) for v in fin) and np.isnan(ref).all()
            continue
        assert tuple(fin[:3]) == tuple(ref[:3]), (name, i)                                        # a1..a3 equal the reference's
        if name == 'nonpositive_pred':
            assert np.array_equal(np.isfinite(fin), np.isfinite(ref))
            continue
        r64 = V.depth_ref64(p, g, crop)
        for k, s in zip(range(3, 9), V.depth_metric_scales(p, g, crop)):
            if not np.isfinite(s):
                continue               # one valid pixel: silog is the square root of a rounding residue on either side
            print(f'{name}/{i} metric {k}: device {fin[k]!r} reference {ref[k]!r} fp64 {r64[k]!r}')
            assert abs(fin[k] - ref[k]) <= abs(ref[k] - r64[k]) + V.SUM_REL * s, (name, i, k, fin[k], ref[k], r64[k])
    print(f'{name}: largest |device - fp64| / sum|term| = {worst:.3e}')


def test_depth_pre_eval_host_layer():
    case = V.depth_cases()['mixed_sizes']
    P = [torch.from_numpy(p).cuda()[None] for p in case['preds']]           # (1, H, W), as simple_test(on_device=True) returns them
    res = ev.depth_pre_eval(P, case['gts'], V.MIN_DEPTH, V.MAX_DEPTH, crops=case['crops'])
    raw = _depth_run(case).cpu().numpy()
    assert res == [ev.depth_finalize(r) for r in raw] and all(len(t) == 9 for t in res)
    empty = V.depth_cases()['empty_rect']
    res = ev.depth_pre_eval([torch.from_numpy(p).cuda() for p in empty['preds']], empty['gts'], V.MIN_DEPTH, V.MAX_DEPTH, crops=empty['crops'])
    assert all(np.isnan(v) for t in res for v in t)


# ---- bev ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', BEV_NAMES)
def test_bev_counters_are_exact(name):
    case = V.bev_cases()[name]
    P, G = _bev_dev(case)
    got = ev.bev_counts(P, G, case['thresholds']).cpu().numpy().astype(np.int64)
    exp = np.stack([V.bev_expect(p, g, case['thresholds']) for p, g in zip(case['probs'], case['gts'])])
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:8]
    res = ev.bev_pre_eval(P, [torch.from_numpy(g != 0) for g in case['gts']], case['thresholds'])           # bool masks from the host
    assert all(r.dtype == torch.int64 and np.array_equal(r.numpy(), e) for r, e in zip(res, exp))


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    seg = V.seg_cases()['mix64']
    P, L = _seg_dev(seg)
    assert torch.equal(_seg_run(seg, P, L), _seg_run(seg, P, L))
    dep = V.kitti_case()
    a, b = _depth_run(dep), _depth_run(dep)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    bev = V.bev_cases()['k6_p40000_t7']
    Pb, Gb = _bev_dev(bev)
    assert torch.equal(ev.bev_counts(Pb, Gb, bev['thresholds']), ev.bev_counts(Pb, Gb, bev['thresholds']))


def test_an_item_alone_equals_the_item_as_number_37_of_64():
    mixed = V.depth_cases()['mixed_sizes']
    kitti = V.kitti_case()
    target = dict(preds=[kitti['preds'][1]], gts=[kitti['gts'][1]], crops=[kitti['crops'][1]])
    alone = _depth_run(target)
    n = len(mixed['preds'])
    order = [j % n for j in range(64)]
    many = dict(preds=[mixed['preds'][j] for j in order], gts=[mixed['gts'][j] for j in order], crops=[mixed['crops'][j] for j in order])
    for k in ('preds', 'gts', 'crops'):
        many[k][36] = target[k][0]
    full = _depth_run(many)
    assert torch.equal(full[36].view(torch.int64), alone[0].view(torch.int64))
    assert torch.equal(full[5].view(torch.int64), full[5 + n].view(torch.int64))                   # and a small item at two positions
    seg = V.seg_cases()['mix64']
    P, L = _seg_dev(seg)
    full = _seg_run(seg, P, L)
    assert torch.equal(full[36:37], _seg_run(seg, P[36:37], L[36:37]))


def test_a_replayed_graph_sees_the_rewritten_maps():
    seg, dep, bev = V.seg_cases()['shapes_block'], V.depth_cases()['mixed_sizes'], V.bev_cases()['k6_p63_t7']
    P, L = _seg_dev(seg)
    DP, DG = _depth_dev(dep)
    BP, BG = _bev_dev(bev)
    seg_out = torch.empty((len(P), 3, 256), dtype=torch.int32, device='cuda')
    dep_out = torch.empty((len(DP), 16), dtype=torch.float64, device='cuda')
    dep_ws = torch.empty(ev.depth_workspace_bytes([p.shape for p in DP]) // 8, dtype=torch.float64, device='cuda')
    bev_out = torch.empty((len(BP), 6, 7, 3), dtype=torch.int32, device='cuda')

    def enqueue():
        ev.seg_counts(P, L, seg['K'], seg['ignore_index'], seg['reduce_zero_label'], out=seg_out)
        ev.depth_sums(DP, DG, V.MIN_DEPTH, V.MAX_DEPTH, dep['crops'], out=dep_out, workspace=dep_ws)
        ev.bev_counts(BP, BG, bev['thresholds'], out=bev_out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = (seg_out.clone(), dep_out.clone(), bev_out.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    # rewrite the maps in place: the items of every task change places (reversed content where the sizes allow: same-size swaps)
    P[3].copy_(P[3].flip(0)), L[3].copy_(L[3].flip(1))
    DP[2].copy_(DP[2] * 1.5)
    BP[0].copy_(1 - BP[0])
    for t in (seg_out, dep_out, bev_out):
        t.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    want_seg = V.seg_expect(P[3].cpu().numpy(), L[3].cpu().numpy(), seg['K'], seg['ignore_index'], seg['reduce_zero_label'])
    assert np.array_equal(seg_out[3].cpu().numpy(), want_seg) and not torch.equal(seg_out[3], first[0][3])
    assert torch.equal(seg_out[:3], first[0][:3])
    cols, mags = V.depth_expect64(DP[2].cpu().numpy(), dep['gts'][2], dep['crops'][2])
    got = dep_out[2].cpu().numpy()
    assert np.array_equal(got[:4], cols[:4]) and (np.abs(got[4:10] - cols[4:]) <= V.SUM_REL * mags).all()
    assert not torch.equal(dep_out[2], first[1][2]) and torch.equal(dep_out[:2].view(torch.int64), first[1][:2].view(torch.int64))
    assert np.array_equal(bev_out[0].cpu().numpy(), V.bev_expect(BP[0].cpu().numpy(), bev['gts'][0], bev['thresholds']))
    assert torch.equal(bev_out[1], first[2][1]) and not torch.equal(bev_out[0], first[2][0])


# ---- buffer safety -----------------------------------------------------------------------------------------------------------------
def _guarded(n_elem, dtype, sentinel):
    buf = torch.full((n_elem + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n_elem]


def test_exactly_sized_buffers_keep_their_guards():
    seg = V.seg_cases()['mix64']
    buf, out = _guarded(64 * 3 * 256, torch.int32, -7)
    _seg_run(seg, out=out.view(64, 3, 256))
    assert (buf[:GUARD] == -7).all() and (buf[-GUARD:] == -7).all() and np.array_equal(out.view(64, 3, 256).cpu().numpy(), V.seg_case_expect(seg))
    dep = V.depth_cases()['mixed_sizes']
    n = len(dep['preds'])
    ws_elems = ev.depth_workspace_bytes([p.shape for p in dep['preds']]) // 8
    assert ws_elems == 10 * sum(-(-p.size // V.DEPTH_TILE) for p in dep['preds'])
    sbuf, sums = _guarded(n * 16, torch.float64, -7.0)
    wbuf, ws = _guarded(ws_elems, torch.float64, -7.0)
    _depth_run(dep, out=sums.view(n, 16), workspace=ws)
    torch.cuda.synchronize()
    for b in (sbuf, wbuf):
        assert (b[:GUARD] == -7).all() and (b[-GUARD:] == -7).all()
    assert (ws != -7).all() and torch.equal(sums.view(n, 16).view(torch.int64), _depth_run(dep).view(torch.int64))
    bev = V.bev_cases()['k32_p63_t16']
    P, G = _bev_dev(bev)
    bbuf, bout = _guarded(1 * 32 * 16 * 3, torch.int32, -7)
    ev.bev_counts(P, G, bev['thresholds'], out=bout.view(1, 32, 16, 3))
    assert (bbuf[:GUARD] == -7).all() and (bbuf[-GUARD:] == -7).all()
    assert np.array_equal(bout.view(32, 16, 3).cpu().numpy(), V.bev_expect(bev['probs'][0], bev['gts'][0], bev['thresholds']))


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _intersect_and_union(pred_label, label, num_classes, ignore_index, reduce_zero_label):
    """segmentation/mmseg/core/evaluation/metrics.py:58-87 (label_map empty): the host path ``dataset.pre_eval`` runs today"""
    pred_label = torch.from_numpy(pred_label)
    label = torch.from_numpy(label.copy())
    if reduce_zero_label:
        label[label == 0] = 255
        label = label - 1
        label[label == 254] = 255
    mask = (label != ignore_index)
    pred_label = pred_label[mask]
    label = label[mask]
    intersect = pred_label[pred_label == label]
    area_intersect = torch.histc(intersect.float(), bins=(num_classes), min=0, max=num_classes - 1)
    area_pred_label = torch.histc(pred_label.float(), bins=(num_classes), min=0, max=num_classes - 1)
    area_label = torch.histc(label.float(), bins=(num_classes), min=0, max=num_classes - 1)
    area_union = area_pred_label + area_label - area_intersect
    return area_intersect, area_union, area_pred_label, area_label


def test_harness_device_eval_equals_the_host_path():
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

        def pre_eval(self, preds, indices):
            return [_intersect_and_union(p, self.labels[i], K, self.ignore_index, self.reduce_zero_label) for p, i in zip(preds, indices)]

    def collate(idx):
        return dict(img=[torch.zeros(len(idx), 3, H, W)], img_metas=[[metas[i] for i in idx]])

    loader = torch.utils.data.DataLoader(DS(), batch_size=2, shuffle=False, collate_fn=collate)
    torch.manual_seed(3)
    host = apis.single_gpu_test(model, loader, pre_eval=True)
    torch.manual_seed(3)
    dev = apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True)
    assert len(host) == len(dev) == 5
    for i, (a, b) in enumerate(zip(host, dev)):
        assert len(a) == len(b) == 4
        for s, t in zip(a, b):
            assert s.dtype == t.dtype == torch.float32 and s.shape == t.shape == (K,) and torch.equal(s, t), i
    assert sum(float(t[3].sum()) for t in dev) > 0
    torch.manual_seed(3)
    multi = apis.multi_gpu_test(model, loader, pre_eval=True, device_eval=True)
    assert all(torch.equal(s, t) for a, b in zip(multi, dev) for s, t in zip(a, b))
    # the entry points themselves: on_device=True returns the epilogue's uint8 device maps, equal to the default return value
    img = torch.zeros(2, 3, H, W, device='cuda')
    for call in (lambda **k: model.simple_test(img, [metas[0], metas[1]], rescale=True, **k),
                 lambda **k: model([img], [[metas[0], metas[1]]], return_loss=False, **k),
                 lambda **k: model.aug_test([img, img], [[metas[0], metas[0]], [dict(metas[0], flip=True), dict(metas[0], flip=True)]], **k),
                 lambda **k: model([img, img], [[metas[2], metas[2]], [dict(metas[2], flip=True), dict(metas[2], flip=True)]], return_loss=False, **k)):
        torch.manual_seed(9)
        default = call()
        torch.manual_seed(9)
        on_dev = call(on_device=True)
        assert len(default) == len(on_dev) == 2
        for d, t in zip(default, on_dev):
            assert isinstance(d, np.ndarray) and d.dtype == np.int64
            assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2
            assert np.array_equal(t.cpu().numpy().astype('int64'), d)


def test_slide_mode_on_device_equals_the_default():
    from golden_util import load_case
    from support import seg_model as _seg_model
    cfg, sd, x, _, _, _ = load_case('seg_city_r2')
    model = _seg_model(dict(cfg, randsteps=1))
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    model.test_cfg = dict(mode='slide', crop_size=(32, 48), stride=(20, 30))

    class CropBackbone(torch.nn.Module):
        def forward(self, img):
            return [torch.nn.functional.avg_pool2d(img, 4).repeat(1, 86, 1, 1)[:, :256].contiguous()]
    model.backbone = CropBackbone()
    H, W = 56, 100
    img = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    meta = [dict(img_shape=(H - 2, W - 3, 3), ori_shape=(H + 5, W + 9, 3), flip=True, flip_direction='horizontal')]
    for call in (lambda **k: model.simple_test(img, meta, rescale=True, **k),
                 lambda **k: model([img, img], [meta, [dict(meta[0], flip=False)]], return_loss=False, **k)):
        torch.manual_seed(21)
        default = call()
        torch.manual_seed(21)
        on_dev = call(on_device=True)
        assert len(default) == len(on_dev) == 1 and on_dev[0].dtype == torch.uint8 and on_dev[0].is_cuda
        assert np.array_equal(on_dev[0].cpu().numpy().astype('int64'), default[0]) and default[0].shape == (H + 5, W + 9)


def test_depther_on_device_and_harness():
    from ddp_amd import apis
    from ddp_amd.utils import synthetic
    from support import depth_model as _depth_model
    model = _depth_model({}, synthetic.make_state_dict('depth', 1, 6, 256, seed=0))
    model.extract_feat = lambda img: [None]
    H, W = 44, 152
    g = torch.Generator().manual_seed(4)
    model.sample = lambda x, img_metas=None, noise=None: torch.rand(len(img_metas), 1, H // 4, W // 4, generator=g).mul(60).add(1).cuda()
    img = torch.zeros(2, 3, H, W, device='cuda')
    meta = [dict(img_shape=(H, W, 3), ori_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False, flip_direction='horizontal')] * 2
    flip = [dict(m, flip=True) for m in meta]
    for call in (lambda **k: model.simple_test(img, meta, **k), lambda **k: model.aug_test([img, img], [meta, flip], **k),
                 lambda **k: model(return_loss=False, img=[img, img], img_metas=[meta, flip], **k)):
        g.manual_seed(4)
        default = call()
        g.manual_seed(4)
        on_dev = call(on_device=True)
        assert len(default) == len(on_dev) == 2
        for d, t in zip(default, on_dev):
            assert isinstance(d, np.ndarray) and d.dtype == np.float32 and d.shape == (1, H, W)
            assert torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), d)
    # the harness: 5 images, 2 per batch, ground truth and the Garg rectangle from a caller-given loader
    case = V.depth_cases()['quarter_kitti']
    gts = [case['gts'][0] * s for s in (1.0, 0.5, 0.9, 0.25, 0.75)]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 5

        def __getitem__(self, i):
            return i

    def collate(idx):
        return dict(img=[torch.zeros(len(idx), 3, H, W)], img_metas=[[meta[0]] * len(idx)])

    def gt_loader(dataset, i):
        return dict(gt=gts[i], crop=ev.garg_crop(H, W) if i % 2 else None, min_depth=V.MIN_DEPTH, max_depth=V.MAX_DEPTH)

    loader = torch.utils.data.DataLoader(DS(), batch_size=2, shuffle=False, collate_fn=collate)
    g.manual_seed(4)
    preds = apis.single_gpu_test(model, loader)
    g.manual_seed(4)
    res = apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True, gt_loader=gt_loader)
    assert len(res) == len(preds) == 5
    crops = [ev.garg_crop(H, W) if i % 2 else None for i in range(5)]
    # the harness adds nothing of its own: per image exactly what depth_pre_eval gives for that image's map, ground truth and rectangle
    # (an item's row does not depend on the call it is in), and a1..a3 are the reference's
    direct = ev.depth_pre_eval([torch.from_numpy(p).cuda() for p in preds], gts, V.MIN_DEPTH, V.MAX_DEPTH, crops=crops)
    assert res == direct and all(len(t) == 9 and not any(np.isnan(v) for v in t) for t in res)
    for i, (tup, p) in enumerate(zip(res, preds)):
        assert tup[:3] == V.depth_ref32(p[0], gts[i], crops[i])[:3], i
    with pytest.raises(ValueError, match='needs gt_loader'):
        apis.single_gpu_test(model, loader, pre_eval=True, device_eval=True)
