#!/usr/bin/env python
"""Record what the PARENT commit's library gives where GroupNorm convolutions must change nothing (tests/golden/fcn_gn/):

    DDP_LIB_PATH=<parent build>/libddp_mi355x.so python tests/golden/gen_fcn_gn_parent.py workspace   # no device needed
    DDP_LIB_PATH=<parent build>/libddp_mi355x.so python tests/golden/gen_fcn_gn_parent.py bits DIR    # on the GPU; writes DIR/parent_bits.json

``workspace``: ddp_fcn_head_workspace / ddp_sample_fcn_workspace on every case of tests/fcn_gn_cases.py -> parent_workspace_bytes.json.
``bits``: sha256 of the BatchNorm / norm-free heads' outputs on the existing fcn_* / loopfcn_* fixtures -> parent_bits.json.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import fcn_gn_cases as G  # noqa: E402
from ddp_amd import _lib  # noqa: E402

if __name__ == '__main__':
    assert os.environ.get('DDP_LIB_PATH'), 'point DDP_LIB_PATH at the parent build'
    if sys.argv[1] == 'workspace':
        path = os.path.join(HERE, 'fcn_gn', 'parent_workspace_bytes.json')
        json.dump(G.workspace_bytes(_lib.load()), open(path, 'w'), indent=1, sort_keys=True)
    else:
        import torch
        path = os.path.join(sys.argv[2], 'parent_bits.json')
        os.makedirs(sys.argv[2], exist_ok=True)
        json.dump(G.unchanged_path_hashes(torch.device('cuda:0')), open(path, 'w'), indent=1, sort_keys=True)
    print('wrote', path)
