#!/usr/bin/env python
"""Record what the PARENT commit's library gives where DDP_FLAG_SCORE_PRIOR must change nothing (tests/golden/score_prior/):

    DDP_LIB_PATH=<parent build>/libddp_mi355x.so python tests/golden/gen_score_prior_parent.py DIR    # on the GPU; writes DIR/parent_bits.json

sha256 of the flag-clear sampler outputs of tests/score_prior_cases.PARENT_BITS (four cases: the bf16x3 product route, the fp32
engine, the unfused layer route, the ddpm chain) -> parent_bits.json.  tests/test_score_prior_gpu.py::test_flag_clear_bits_are_the_parents
compares the in-tree build with it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import score_prior_cases as P  # noqa: E402

if __name__ == '__main__':
    assert os.environ.get('DDP_LIB_PATH'), 'point DDP_LIB_PATH at the parent build'
    import torch
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'score_prior')
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'parent_bits.json')
    json.dump(P.flag_clear_hashes(torch.device('cuda:0')), open(path, 'w'), indent=1, sort_keys=True)
    print('wrote', path)
