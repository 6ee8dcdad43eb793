"""Cases of the device-side confusion matrix (include/ddp_cm_mi355x.h, ddp_amd/confusion.py) and their expectation.

``cm_expect`` is the numpy restatement of the header's pixel rule.  The cases of tests/device_eval_cases.py (``seg_cases()``,
``big_single_class()``) are cases here too: same maps, same (K, ignore_index, reduce_zero_label).  Added are the in-range cases,
on which the rule is ``calculate_confusion_matrix`` of the reference's tools/confusion_matrix.py literally (labels from the
classes and the ignore value only, reduce_zero_label off) - tests/golden/gen_cm_golden.py records what the reference returned for
them in tests/golden/device_eval/cm_cases.npz - and ``all_keys``, the smallest input that hits every bin of the largest matrix."""
import functools

import numpy as np

import device_eval_cases as V

TALLY = 4
CM_TILE = 8192                                   # pixels per block of the kernel ...
CM_BLOCKS_FULL = 2048                            # ... doubled (up to 8 x) while a call would have more blocks than this
SCALED_ITEMS = (9, 17, 33)                       # full-size items per call at which the tile is 2 x, 4 x, 8 x
IN_RANGE_K = (2, 19, 150, 256)
IN_RANGE_KINDS = ('rand', 'block', 'mix')
IN_RANGE_SHAPES = [(1, 1), (1, 17), (3, 5), (37, 53), (100, 101)]
IN_RANGE_IGNORE = 255


def cm_expect(pred, label, K, ignore_index, reduce_zero_label):
    """-> (matrix (K, K) int64, tally (4,) int64) by the header's restatement, rule by rule"""
    p = pred.reshape(-1).astype(np.int64)
    l = label.reshape(-1).astype(np.int64)
    if reduce_zero_label:
        l = np.where((l == 0) | (l == 255), 255, l - 1)
    tally = np.zeros(TALLY, dtype=np.int64)
    tally[0] = p.size
    ignored = l == ignore_index
    tally[1] = ignored.sum()
    label_out = ~ignored & (l >= K)
    tally[2] = label_out.sum()
    pred_out = ~ignored & ~label_out & (p >= K)
    tally[3] = pred_out.sum()
    keep = ~ignored & ~label_out & ~pred_out
    matrix = np.bincount(K * l[keep] + p[keep], minlength=K * K).reshape(K, K)
    return matrix.astype(np.int64), tally


def cm_case_expect(case):
    """the sum over the items of a case: what ONE call returns"""
    m, t = np.zeros((case['K'], case['K']), dtype=np.int64), np.zeros(TALLY, dtype=np.int64)
    for p, l in zip(case['preds'], case['labels']):
        mi, ti = cm_expect(p, l, case['K'], case['ignore_index'], case['reduce_zero_label'])
        m += mi
        t += ti
    return m, t


@functools.lru_cache(maxsize=None)
def in_range_cases():
    """name -> dict(preds, labels, K, ignore_index, reduce_zero_label): per (K, kind) the five shapes as the five images of a
    dataset.  Labels: the classes and the ignore value; predictions: the classes."""
    cs = {}
    for i, K in enumerate(IN_RANGE_K):
        for j, kind in enumerate(IN_RANGE_KINDS):
            rng = np.random.default_rng(500 + 10 * i + j)
            lv = list(range(K)) + [IN_RANGE_IGNORE] * (1 + K // 8)     # about a ninth of the labels (blocks) ignored, whatever K is
            pairs = [V._pair(rng, h, w, kind, lv, range(K)) for h, w in IN_RANGE_SHAPES]
            cs[f'k{K}_{kind}'] = dict(preds=[p for p, _ in pairs], labels=[l for _, l in pairs], K=K, ignore_index=IN_RANGE_IGNORE,
                                      reduce_zero_label=False)
    return cs


@functools.lru_cache(maxsize=None)
def full_size_mix():
    """one 1024 x 2048 pair, upper half 8 x 8 blocks and lower half random, 150 classes with reduce_zero_label: given to one call
    SCALED_ITEMS times over, it makes the call large enough for the 2 x, 4 x and 8 x tile.  -> (pred, label, matrix, tally)"""
    rng = np.random.default_rng(77)
    p, l = V._pair(rng, 1024, 2048, 'mix', V._label_values(150, 255), range(150))
    return (p, l) + cm_expect(p, l, 150, 255, True)


def all_keys():
    """K = 256, nothing ignored, label[y][x] = y and pred[y][x] = x on 256 x 256: each of the 65 536 bins exactly once; a block
    of the kernel sees CM_TILE distinct keys, more than any table of a block holds"""
    y, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return dict(preds=[np.ascontiguousarray(x)], labels=[np.ascontiguousarray(y)], K=256, ignore_index=-1, reduce_zero_label=False)
