"""Cases of the device-side pre_eval statistics (include/ddp_eval_mi355x.h, ddp_amd/evaluation.py) and their expectations.

Every case is built from a seed by numpy alone; the expectations are numpy restatements of the header's §seg / §depth / §bev.
tests/test_device_eval_host.py checks the restatements against what the reference's own functions returned (the fixtures
tests/golden/device_eval/eval_*.npz, written by tests/golden/gen_eval_golden.py) and that the case conditions hold;
tests/test_device_eval_gpu.py runs the cases on an MI355X.  The shapes are the smallest at which the kernels can go wrong:
shorter than one 16-byte vector, flat lengths that are no multiple of 16, more than one block (8192 seg / 1024 depth / 2048 bev
pixels), a head that is not 16-byte aligned, two maps that disagree in alignment (bytewise path), whole waves of one key."""
import functools

import numpy as np
import torch

BINS = 256
SEG_TILE, DEPTH_TILE, BEV_TILE = 8192, 1024, 2048
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0
RATIO_BOUNDS = (1.25, 1.5625, 1.953125)          # 1.25 ** 1, 2, 3: exact in fp32
SUM_REL = 2.0 ** -40                             # depth fp64 sums: |device - numpy fp64| <= SUM_REL * sum |term|
BEV_DEFAULT = (0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)


# ---- seg ---------------------------------------------------------------------------------------------------------------------------
def rand_map(rng, h, w, values):
    return rng.choice(np.asarray(values, dtype=np.uint8), size=(h, w))


def block_map(rng, h, w, values, bs=8):
    """piecewise constant: bs x bs blocks of one value each"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=((h + bs - 1) // bs, (w + bs - 1) // bs))
    return np.ascontiguousarray(np.kron(small, np.ones((bs, bs), dtype=np.uint8))[:h, :w])


def _pred_for(rng, label, values, kind):
    """a prediction that agrees with the label on about two thirds of the pixels (blocks)"""
    h, w = label.shape
    other = (block_map if kind == 'block' else rand_map)(rng, h, w, values)
    keep = (block_map(rng, h, w, [0, 1, 1]) if kind == 'block' else rand_map(rng, h, w, [0, 1, 1])).astype(bool)
    return np.where(keep, label, other).astype(np.uint8)


def _pair(rng, h, w, kind, label_values, pred_values):
    if kind == 'mix':                             # upper half piecewise constant, lower half random
        hh = max(h // 2, 1)
        a = _pair(rng, hh, w, 'block', label_values, pred_values)
        if h == hh:
            return a
        b = _pair(rng, h - hh, w, 'rand', label_values, pred_values)
        return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    label = (block_map if kind == 'block' else rand_map)(rng, h, w, label_values)
    return _pred_for(rng, label, pred_values, kind), label


def _label_values(K, ign):
    """classes, the ignore value, and two values >= K that are NOT the ignore value (where uint8 has room for them)"""
    v = list(range(K)) + [ign]
    v += [x for x in (K, 254, 255) if K <= x <= 255 and x != ign][:2]
    return sorted(set(v))


SEG_PARAMS = [(K, ign, rzl) for K in (2, 19, 150, 256) for ign in (0, 200, 255) for rzl in (False, True)]
SMALL_SHAPES = [(1, 1), (1, 17), (3, 5), (37, 53), (64, 64)]


def _seg_param_case(K, ign, rzl, seed):
    rng = np.random.default_rng(seed)
    lv, pv = _label_values(K, ign), list(range(K))
    pairs = [_pair(rng, 3, 5, 'rand', lv, pv), _pair(rng, 37, 53, 'rand', lv, pv), _pair(rng, 24, 40, 'block', lv, pv)]
    return dict(preds=[p for p, _ in pairs], labels=[l for _, l in pairs], K=K, ignore_index=ign, reduce_zero_label=rzl)


@functools.lru_cache(maxsize=None)
def seg_cases():
    """name -> dict(preds, labels, K, ignore_index, reduce_zero_label[, offsets]); ``offsets`` = per item the byte offsets
    (pred, label) of the maps from a 256-byte aligned allocation (default (0, 0))."""
    cs = {}
    for i, (K, ign, rzl) in enumerate(SEG_PARAMS):
        cs[f'k{K}_ign{ign}_rzl{int(rzl)}'] = _seg_param_case(K, ign, rzl, 100 + i)
    rng = np.random.default_rng(7)
    # the five small shapes in one call, random and piecewise constant
    for kind in ('rand', 'block'):
        pairs = [_pair(rng, h, w, kind, _label_values(19, 255), range(19)) for h, w in SMALL_SHAPES]
        cs[f'shapes_{kind}'] = dict(preds=[p for p, _ in pairs], labels=[l for _, l in pairs], K=19, ignore_index=255, reduce_zero_label=False)
    # content cases
    p, l = _pair(rng, 37, 53, 'rand', [255], range(19))
    cs['all_ignored'] = dict(preds=[p], labels=[l], K=19, ignore_index=255, reduce_zero_label=False)
    p, l = rand_map(rng, 37, 53, range(19)), rand_map(rng, 37, 53, range(256))      # every prediction a class, most labels none
    cs['label_ge_k'] = dict(preds=[p], labels=[l], K=19, ignore_index=255, reduce_zero_label=False)
    p, l = _pair(rng, 37, 53, 'rand', _label_values(19, 255), range(256))
    cs['pred_ge_k'] = dict(preds=[p], labels=[l], K=19, ignore_index=255, reduce_zero_label=False)
    # 64 items of different sizes in one call: piecewise constant, random and their mixture
    pairs = [_pair(rng, 1 + (7 * i) % 45, 1 + (13 * i) % 67, ('block', 'rand', 'mix')[i % 3], _label_values(150, 255), range(150))
             for i in range(64)]
    cs['mix64'] = dict(preds=[p for p, _ in pairs], labels=[l for _, l in pairs], K=150, ignore_index=255, reduce_zero_label=True)
    # alignment: an aligned base with an odd width; a shared misalignment (vector path with a head) across a block border;
    # two maps that disagree (bytewise path)
    pairs = [_pair(rng, 33, 47, 'mix', _label_values(19, 255), range(19)), _pair(rng, 100, 101, 'mix', _label_values(19, 255), range(19)),
             _pair(rng, 100, 101, 'block', _label_values(19, 255), range(19)), _pair(rng, 3, 5, 'rand', _label_values(19, 255), range(19))]
    cs['alignment'] = dict(preds=[p for p, _ in pairs], labels=[l for _, l in pairs], K=19, ignore_index=255, reduce_zero_label=False,
                           offsets=[(0, 0), (5, 21), (3, 8), (15, 15)])
    # whole waves of one key (a wave owns 1024 consecutive pixels): bands of rows, with a key change between waves, an ignored
    # band, a band where the prediction is wrong, and one ragged row
    lab = np.repeat(np.array([1, 1, 1, 2, 2, 255, 255, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4], dtype=np.uint8), 2)[:, None] * np.ones((1, 1024), np.uint8)
    prd = lab.copy()
    prd[prd == 255] = 7
    prd[14:20] = 9
    prd[30, 100:300] = 2
    cs['bands'] = dict(preds=[prd], labels=[np.ascontiguousarray(lab)], K=19, ignore_index=255, reduce_zero_label=False)
    return cs


def big_single_class():
    """one 1024 x 2048 item of a single class: one bin of 2 097 152 (the worst contention; 256 blocks flush into it)"""
    m = np.full((1024, 2048), 5, dtype=np.uint8)
    return dict(preds=[m], labels=[m.copy()], K=19, ignore_index=255, reduce_zero_label=False)


def seg_expect(pred, label, K, ignore_index, reduce_zero_label):
    """(3, 256) int64 [intersect, pred, label] by the header's restatement, pixel rule by pixel rule"""
    p = pred.reshape(-1).astype(np.int64)
    l = label.reshape(-1).astype(np.int64)
    if reduce_zero_label:
        l = np.where((l == 0) | (l == 255), 255, l - 1)
    keep = l != ignore_index
    p, l = p[keep], l[keep]
    out = np.zeros((3, BINS), dtype=np.int64)
    out[1] = np.bincount(p[p < K], minlength=BINS)
    out[2] = np.bincount(l[l < K], minlength=BINS)
    out[0] = np.bincount(p[(p == l) & (p < K)], minlength=BINS)
    return out


def seg_case_expect(case):
    return np.stack([seg_expect(p, l, case['K'], case['ignore_index'], case['reduce_zero_label'])
                     for p, l in zip(case['preds'], case['labels'])])


# ---- depth -------------------------------------------------------------------------------------------------------------------------
def garg(h, w):
    return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)


def _depth_pair(rng, h, w):
    """gt in (0, 90) with a fifth of the pixels 0 (no measurement) and some beyond max_depth; pred = gt on a tenth of the pixels,
    else gt * f with f in [0.5, 0.97] or [1.03, 2] (>= 2 % away after fp32 rounding)"""
    gt = rng.uniform(0.5, 90.0, size=(h, w)).astype(np.float32)
    gt[rng.random((h, w)) < 0.2] = 0.0
    f = np.where(rng.random((h, w)) < 0.5, rng.uniform(0.5, 0.97, size=(h, w)), rng.uniform(1.03, 2.0, size=(h, w)))
    f[rng.random((h, w)) < 0.1] = 1.0
    pred = (gt.astype(np.float64) * f).astype(np.float32)
    pred[gt == 0] = rng.uniform(1.0, 80.0, size=int((gt == 0).sum())).astype(np.float32)
    return pred, gt


def _boundary_pair():
    """g/p and p/g exactly at 1.25, 1.5625, 1.953125 and one fp32 ulp either side (p or g = 2: the quotient is exact)"""
    vals = []
    for b in RATIO_BOUNDS:
        b = np.float32(b)
        vals += [np.nextafter(b, np.float32(0)), b, np.nextafter(b, np.float32(4))]
    r = np.array(vals, dtype=np.float32)
    two = np.full_like(r, 2.0)
    gt = np.concatenate([r * 2, two])[None]         # g / p = r   |   p / g = r
    pred = np.concatenate([two, r * 2])[None]
    return np.ascontiguousarray(pred), np.ascontiguousarray(gt)


@functools.lru_cache(maxsize=None)
def depth_cases():
    """name -> dict(preds, gts, crops (per item (y0, y1, x0, x1) or None))"""
    rng = np.random.default_rng(11)
    cs = {}
    small = [_depth_pair(rng, 1, 1), _depth_pair(rng, 7, 9)]
    small[0][1][0, 0] = 10.0
    small[0][0][0, 0] = 12.5
    cs['small_full'] = dict(preds=[p for p, _ in small], gts=[g for _, g in small], crops=[None, None])
    cs['small_garg'] = dict(preds=[small[1][0]], gts=[small[1][1]], crops=[garg(7, 9)])
    p, g = _depth_pair(rng, 44, 152)
    cs['quarter_kitti'] = dict(preds=[p, p], gts=[g, g], crops=[None, garg(44, 152)])
    p, g = _boundary_pair()
    cs['boundary'] = dict(preds=[p], gts=[g], crops=[None])
    p, g = _depth_pair(rng, 7, 9)
    cs['empty_rect'] = dict(preds=[p, p], gts=[g, g], crops=[(3, 3, 0, 9), (0, 7, 4, 4)])
    cs['all_invalid'] = dict(preds=[p, p], gts=[np.zeros_like(g), np.full_like(g, 80.0)], crops=[None, None])
    sizes = [(1, 1), (7, 9), (33, 65), (100, 41), (5, 1000)]
    pairs = [_depth_pair(rng, h, w) for h, w in sizes]
    cs['mixed_sizes'] = dict(preds=[p for p, _ in pairs], gts=[g for _, g in pairs],
                             crops=[None, garg(7, 9), None, garg(100, 41), (1, 4, 17, 983)])
    p, g = _depth_pair(rng, 7, 9)
    p[2, 3], p[4, 4] = 0.0, -1.5                    # nothing is special-cased: inf / NaN as in the reference
    g[2, 3], g[4, 4] = 10.0, 20.0
    cs['nonpositive_pred'] = dict(preds=[p], gts=[g], crops=[None])
    return cs


FIXTURE_DEPTH = ['small_full', 'small_garg', 'quarter_kitti', 'boundary', 'empty_rect', 'all_invalid', 'mixed_sizes', 'nonpositive_pred']


@functools.lru_cache(maxsize=None)
def kitti_case():
    """352 x 1216, the full map and the Garg rectangle (too large for a fixture: its reference is ``depth_ref32``)"""
    p, g = _depth_pair(np.random.default_rng(12), 352, 1216)
    return dict(preds=[p, p], gts=[g, g], crops=[None, garg(352, 1216)])


def depth_valid(pred, gt, crop):
    """the valid pixels in row-major order -> (g, p) float32"""
    h, w = gt.shape
    y0, y1, x0, x1 = crop or (0, h, 0, w)
    g, p = gt[y0:y1, x0:x1].reshape(-1), pred[y0:y1, x0:x1].reshape(-1)
    m = (g > np.float32(MIN_DEPTH)) & (g < np.float32(MAX_DEPTH))
    return g[m], p[m]


def depth_expect64(pred, gt, crop):
    """-> (cols, mags): the ten columns in numpy (counts from fp32 quotients, sums in fp64 from the fp32 inputs) and, for the six
    sums, sum |term| (what the tolerance scales with)"""
    g, p = depth_valid(pred, gt, crop)
    with np.errstate(all='ignore'):
        t = np.maximum(g / p, p / g)                 # float32 / float32: correctly rounded
        cols = [float(g.size)] + [float((t < np.float32(b)).sum()) for b in RATIO_BOUNDS]
        g, p = g.astype(np.float64), p.astype(np.float64)
        terms = [np.abs(g - p) / g, (g - p) ** 2, np.abs(np.log10(g) - np.log10(p)), (np.log(g) - np.log(p)) ** 2, np.log(p) - np.log(g),
                 (g - p) ** 2 / g]
        return np.array(cols + [float(x.sum()) for x in terms]), np.array([float(np.abs(x).sum()) for x in terms])


def calculate(gt, pred):
    """depth/depth/core/evaluation/metrics.py:7-32, restated line by line (run on float32 it is the reference, on float64 the
    exact value it approximates)"""
    if gt.shape[0] == 0:
        return (np.nan,) * 9
    with np.errstate(all='ignore'):
        thresh = np.maximum((gt / pred), (pred / gt))
        a1 = (thresh < 1.25).mean()
        a2 = (thresh < 1.25 ** 2).mean()
        a3 = (thresh < 1.25 ** 3).mean()
        abs_rel = np.mean(np.abs(gt - pred) / gt)
        sq_rel = np.mean(((gt - pred) ** 2) / gt)
        rmse = np.sqrt(((gt - pred) ** 2).mean())
        rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
        err = np.log(pred) - np.log(gt)
        silog = np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100
        if np.isnan(silog):
            silog = 0
        log_10 = (np.abs(np.log10(gt) - np.log10(pred))).mean()
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel


def depth_ref32(pred, gt, crop):
    g, p = depth_valid(pred, gt, crop)
    return tuple(float(v) for v in calculate(g, p))


def depth_ref64(pred, gt, crop):
    g, p = depth_valid(pred, gt, crop)
    return tuple(float(v) for v in calculate(g.astype(np.float64), p.astype(np.float64)))


def depth_metric_scales(pred, gt, crop):
    """per final metric (abs_rel, rmse, log_10, rmse_log, silog, sq_rel - indices 3..8 of the nine-tuple) what SUM_REL multiplies:
    a sum S of n terms is off by at most SUM_REL * sum |term|, so
      a mean of non-negative terms is off by SUM_REL * itself;   sqrt(mean) by half of that, relative (taken whole);
      silog = 100 sqrt(m2 - m1^2): d silog = 100 (d m2 + 2 |m1| d m1) / (2 sqrt(m2 - m1^2)), d m2 <= SUM_REL m2, d m1 <= SUM_REL mean |err|."""
    g, p = depth_valid(pred, gt, crop)
    if g.size == 0:
        return (0.0,) * 6
    r = depth_ref64(pred, gt, crop)
    with np.errstate(all='ignore'):
        err = np.log(p.astype(np.float64)) - np.log(g.astype(np.float64))
        m2, m1, mabs = np.mean(err ** 2), np.mean(err), np.mean(np.abs(err))
        var = m2 - m1 ** 2
        silog = 100 * (m2 + 2 * abs(m1) * mabs) / (2 * np.sqrt(var)) if var > 0 else float('inf')
    return abs(r[3]), abs(r[4]), abs(r[5]), abs(r[6]), float(silog), abs(r[8])


# ---- bev ---------------------------------------------------------------------------------------------------------------------------
def _bev_item(rng, K, shape, thr):
    prob = rng.random((K,) + shape).astype(np.float32)
    flat = prob.reshape(K, -1)
    t32 = np.asarray(thr, dtype=np.float32)
    for k in range(K):                               # probabilities exactly equal to a threshold (>= counts them as hits)
        for j, t in enumerate(t32):
            if j < flat.shape[1]:
                flat[k, (j * 3 + k) % flat.shape[1]] = t
    gt = (rng.random((K,) + shape) < 0.4).astype(np.uint8)
    gt[gt > 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=int((gt > 0).sum()))     # label = (gt != 0)
    return prob, gt


@functools.lru_cache(maxsize=None)
def bev_cases():
    """name -> dict(probs, gts, thresholds)"""
    rng = np.random.default_rng(13)
    t16 = tuple(float(x) for x in rng.permutation(np.linspace(0.05, 0.95, 16)))          # unsorted
    cs = {}
    for name, K, shape, thr, n in [('k1_p1_t1', 1, (1, 1), (0.35,), 1), ('k6_p63_t7', 6, (7, 9), BEV_DEFAULT, 2),
                                   ('k32_p63_t16', 32, (63,), t16, 1), ('k6_p40000_t7', 6, (200, 200), BEV_DEFAULT, 2),
                                   ('k1_p40000_t16', 1, (200, 200), t16, 1), ('k32_p1_t7', 32, (1, 1), BEV_DEFAULT[::-1], 3)]:
        items = [_bev_item(rng, K, shape, thr) for _ in range(n)]
        cs[name] = dict(probs=[p for p, _ in items], gts=[g for _, g in items], thresholds=thr)
    cs['k1_p1_t1']['probs'][0][...] = np.float32(0.35)
    cs['k1_p1_t1']['gts'][0][...] = 1
    return cs


def bev_expect(prob, gt, thresholds):
    """(K, T, 3) int64 tp / fp / fn: nuscenes_dataset.py:506-514 in numpy"""
    K = prob.shape[0]
    pred = prob.reshape(K, -1)[:, :, None] >= np.asarray(thresholds, dtype=np.float32)
    label = (gt.reshape(K, -1) != 0)[:, :, None]
    return np.stack([(pred & label).sum(1), (pred & ~label).sum(1), (~pred & label).sum(1)], axis=-1).astype(np.int64)


# ---- what the two GPU files share (tests/test_device_eval_gpu.py, tests/test_confusion_gpu.py) -----------------------------------
GUARD = 64           # elements on either side of every output buffer a guarded test hands to the libraries


def flat_at(arr, off, dtype):
    """``arr`` on the device, ``off`` bytes into a 256-byte aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.empty(off + t.numel() * t.element_size() + 16, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + t.numel() * t.element_size()].view(dtype).reshape(arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return view


def seg_dev(case):
    offs = case.get('offsets') or [(0, 0)] * len(case['preds'])
    P = [flat_at(p, o[0], torch.uint8) for p, o in zip(case['preds'], offs)]
    L = [flat_at(l, o[1], torch.uint8) for l, o in zip(case['labels'], offs)]
    return P, L


class PerImageBackbone(torch.nn.Module):
    """stands in for the frozen backbone + neck: the fixture's feature map, once per image of the batch"""

    def __init__(self, x):
        super().__init__()
        self.x = x

    def forward(self, img):
        return [self.x.expand(img.shape[0], -1, -1, -1).contiguous()]
