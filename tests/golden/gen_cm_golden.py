"""Fixture of the device-side confusion matrix: the in-range cases of tests/confusion_cases.py run through the REFERENCE's own
``calculate_confusion_matrix`` (segmentation/tools/confusion_matrix.py:46-68), loaded by path through tests/golden/ref_shim.py.

    python tests/golden/gen_cm_golden.py          (by hand, where the reference tree is present)

writes tests/golden/device_eval/cm_cases.npz: per case the maps, the (K, K) float64 matrix the reference returned for the case's
images as one dataset, and a JSON config.  Arrays and JSON only.
"""
import importlib.util
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'device_eval')
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import confusion_cases as CC  # noqa: E402
import ref_shim  # noqa: E402


def load_tool():
    ref_shim.import_seg()
    for n in ('matplotlib', 'matplotlib.pyplot', 'matplotlib.ticker'):      # the tool draws with them; the matrix does not need them
        try:
            importlib.import_module(n)
        except ImportError:
            sys.modules[n] = MagicMock()
    path = os.path.join(ref_shim.REF, 'segmentation', 'tools', 'confusion_matrix.py')
    spec = importlib.util.spec_from_file_location('_ddp_ref_confusion_matrix', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class StubDataset:
    """what ``calculate_confusion_matrix`` asks of a dataset"""

    def __init__(self, case):
        self.CLASSES = tuple(f'c{i}' for i in range(case['K']))
        self.ignore_index = case['ignore_index']
        self.labels = case['labels']

    def __len__(self):
        return len(self.labels)

    def get_gt_seg_map_by_idx(self, idx):
        return self.labels[idx]


def gen():
    os.makedirs(OUT, exist_ok=True)
    tool = load_tool()
    arrays, cfg = {}, {}
    for name, c in CC.in_range_cases().items():
        assert not c['reduce_zero_label']
        cfg[name] = dict(K=c['K'], ignore_index=c['ignore_index'], n=len(c['preds']))
        # the tool's call: the unpickled results are the int64 maps the harness returns
        ref = tool.calculate_confusion_matrix(StubDataset(c), [p.astype('int64') for p in c['preds']])
        for i, (p, l) in enumerate(zip(c['preds'], c['labels'])):
            arrays[f'{name}/{i}/pred'] = p
            arrays[f'{name}/{i}/label'] = l
        arrays[f'{name}/ref'] = np.asarray(ref)
        arrays[f'{name}/ref_dtype'] = np.array(str(np.asarray(ref).dtype))
    arrays['config'] = np.array(json.dumps(cfg))
    np.savez_compressed(os.path.join(OUT, 'cm_cases.npz'), **arrays)


if __name__ == '__main__':
    gen()
    print('cm_cases.npz', os.path.getsize(os.path.join(OUT, 'cm_cases.npz')), 'bytes')
