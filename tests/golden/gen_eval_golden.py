"""Fixtures of the device-side pre_eval statistics: the cases of tests/device_eval_cases.py run through the REFERENCE's own
functions (``intersect_and_union`` of segmentation/mmseg/core/evaluation/metrics.py, ``metrics`` of
depth/depth/core/evaluation/metrics.py), imported through tests/golden/ref_shim.py.

    python tests/golden/gen_eval_golden.py          (by hand, where the reference tree is present)

writes tests/golden/device_eval/eval_seg_cases.npz and tests/golden/device_eval/eval_depth_cases.npz: per case and item the inputs and what the
reference returned, plus a JSON config.  Arrays and JSON only.  bev: mmdet3d's dataset module cannot be imported here
(it pulls in compiled packages), so tests/test_device_eval_host.py restates the eight lines of ``evaluate_map`` instead.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'device_eval')      # a folder of its own: golden_util.case_names() reads every tests/golden/*.npz as a sampler case
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import device_eval_cases as V  # noqa: E402
import ref_shim  # noqa: E402


def gen_seg():
    os.makedirs(OUT, exist_ok=True)
    ref_shim.import_seg()
    from mmseg.core.evaluation.metrics import intersect_and_union
    arrays, cfg = {}, {}
    for name, c in V.seg_cases().items():
        cfg[name] = dict(K=c['K'], ignore_index=c['ignore_index'], reduce_zero_label=c['reduce_zero_label'], n=len(c['preds']))
        for i, (p, l) in enumerate(zip(c['preds'], c['labels'])):
            # the harness's call: an int64 prediction, the uint8 label map of the loader (intersect_and_union writes into its label)
            res = intersect_and_union(p.astype('int64'), l.copy(), c['K'], c['ignore_index'], dict(), c['reduce_zero_label'])
            arrays[f'{name}/{i}/pred'] = p
            arrays[f'{name}/{i}/label'] = l
            arrays[f'{name}/{i}/ref'] = np.stack([r.numpy() for r in res]).astype(np.float32)        # intersect, union, pred, label
    arrays['config'] = np.array(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, 'eval_seg_cases.npz'), **arrays)


def gen_depth():
    ref_shim.import_depth()
    from depth.core.evaluation.metrics import metrics
    arrays, cfg = {}, {}
    cases = V.depth_cases()
    for name in V.FIXTURE_DEPTH:
        c = cases[name]
        cfg[name] = dict(n=len(c['preds']), crops=[None if r is None else list(r) for r in c['crops']], min_depth=V.MIN_DEPTH,
                         max_depth=V.MAX_DEPTH)
        for i, (p, g, crop) in enumerate(zip(c['preds'], c['gts'], c['crops'])):
            y0, y1, x0, x1 = crop or (0, g.shape[0], 0, g.shape[1])
            mask = np.zeros(g.shape, dtype=bool)           # kitti.py:243-252: the rectangle as a mask, then metrics() on the masked pixels
            mask[y0:y1, x0:x1] = True
            with np.errstate(all='ignore'):
                res = metrics(g[mask], p[mask], min_depth=V.MIN_DEPTH, max_depth=V.MAX_DEPTH)
            arrays[f'{name}/{i}/pred'] = p
            arrays[f'{name}/{i}/gt'] = g
            arrays[f'{name}/{i}/ref'] = np.array([float(v) for v in res], dtype=np.float64)
            arrays[f'{name}/{i}/ref_is_f32'] = np.array([isinstance(v, np.float32) for v in res])
    arrays['config'] = np.array(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, 'eval_depth_cases.npz'), **arrays)


if __name__ == '__main__':
    gen_seg()
    gen_depth()
    for f in ('eval_seg_cases.npz', 'eval_depth_cases.npz'):
        print(f, os.path.getsize(os.path.join(OUT, f)), 'bytes')
