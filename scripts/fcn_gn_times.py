#!/usr/bin/env python
"""FCNHeadWithTime with GroupNorm(32) convolutions next to the BatchNorm head at the C2-sized shape (8 maps of 128 x 256, 2 convs,
150 classes), and k_gn_film_relu_blk next to k_gn_apply_add_blk - the streaming apply pass over the same layout - on the same
number of rows (the FPN neck's level 0 at batch 8, 128 x 256).

  python scripts/fcn_gn_times.py                       # per-call HIP-event times (one JSON line); run it under
                                                       #   rocprofv3 --kernel-trace --stats for the per-kernel times
  python scripts/fcn_gn_times.py --trace <kernel_trace.csv>   # per-kernel medians and bytes/s from that trace (no device needed)

Bytes of an apply pass = rows x 256 channels x 4 B, read once and written once (the per-map vectors are noise beside it); the
lateral stage of the FPN also reads the coarser lateral (a quarter of the rows: 1.125 x the bytes)."""
import csv
import json
import os
import sys

ROWS = 8 * 128 * 256


def summarise(path):
    rows = [r for r in csv.DictReader(open(path)) if r['Kind'] == 'KERNEL_DISPATCH']
    rows.sort(key=lambda r: int(r['Start_Timestamp']))

    def med(v):
        v = sorted(v)
        return v[len(v) // 2] if v else None
    film, add, fin, gemm_gn, gemm_bn = [], [], [], [], []
    for i, r in enumerate(rows):
        name, us = r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        threads = int(r.get('Grid_Size') or r.get('Grid_Size_X') or 0)             # work-items of the launch (x: the only dimension)
        if 'k_gn_film_relu_blk' in name and threads == ROWS // 128 * 256:
            film.append(us)
        elif 'k_gn_apply_add_blk' in name and threads == ROWS * 64:
            add.append(us)
        elif 'k_gn_final32' in name and 'multi' not in name:
            fin.append(us)
        elif 'k_layer<0, 5' in name and i + 1 < len(rows):
            # a GroupNorm conv's GEMM is followed by k_gn_final32; the BatchNorm head runs first: its two 3x3 GEMMs per call are
            # the launches above 1 ms in front of the first apply pass (conv_seg is an eighth of the stages)
            if 'k_gn_final32' in rows[i + 1]['Kernel_Name'] and 'multi' not in rows[i + 1]['Kernel_Name']:
                gemm_gn.append(us)
            elif not film and us > 1000.0:
                gemm_bn.append(us)
    nbytes = 2.0 * ROWS * 1024
    out = dict(rows=ROWS, apply_bytes=nbytes)
    if film:
        out['k_gn_film_relu_blk'] = dict(n=len(film), median_us=round(med(film), 1), tb_per_s=round(nbytes / med(film) / 1e6, 3))
    if add:      # the neck called on its own writes its outputs as NCHW through another kernel: these are the lateral stage's launches
        out['k_gn_apply_add_blk_lateral_stage'] = dict(n=len(add), median_us=round(med(add), 1), bytes=nbytes * 1.125,
                                                       tb_per_s=round(nbytes * 1.125 / med(add) / 1e6, 3),
                                                       tb_per_s_without_the_coarse_reads=round(nbytes / med(add) / 1e6, 3))
    if fin:
        out['k_gn_final32'] = dict(n=len(fin), median_us=round(med(fin), 1))
    if gemm_gn:
        out['conv3x3_gemm_gn_with_fused_statistics'] = dict(n=len(gemm_gn), median_us=round(med(gemm_gn), 1))
    if gemm_bn:
        out['conv3x3_gemm_bn_with_relu'] = dict(n=len(gemm_bn), median_us=round(med(gemm_bn), 1))
    print(json.dumps(out))


def main():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ddp_amd
    from ddp_amd.utils import synthetic
    dev = torch.device('cuda:0')
    feat, temb = synthetic.make_fcn_inputs(8, 128, 256, 3)
    feat, temb = feat.to(dev), temb.to(dev)
    res = {}
    for norm, cfg in (('bn', dict(type='BN')), ('gn', dict(type='GN', num_groups=32))):
        head = ddp_amd.FCNHeadWithTime(num_convs=2, concat_input=False, in_channels=256, channels=256, num_classes=150, in_index=0, norm_cfg=cfg)
        head.load_state_dict(synthetic.make_fcn_state_dict(2, 150, True, False, 140, norm=norm), strict=True)
        head = head.to(dev).eval()
        for _ in range(3):
            head([feat], temb)
        ms = []
        for _ in range(15):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            head([feat], temb)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        res[f'{norm}_head_call_ms'] = dict(median=round(ms[len(ms) // 2], 3), min=round(ms[0], 3), max=round(ms[-1], 3), calls=len(ms))
    # the yardstick kernel on the same rows: the FPN neck with level 0 = 8 x 128 x 256
    inc = [96, 192, 384, 768]
    neck = ddp_amd.FPN(in_channels=inc, out_channels=256, act_cfg=None, norm_cfg=dict(type='GN', num_groups=32), num_outs=4)
    neck.load_state_dict(synthetic.make_fpn_state_dict(inc, 5), strict=True)
    neck = neck.to(dev).eval()
    levels = [t.to(dev) for t in synthetic.make_backbone_levels(8, inc, 128, 256, 5)]
    for _ in range(4):
        neck(levels)
    torch.cuda.synchronize()
    res['shape'] = dict(maps=8, h=128, w=256, num_convs=2, classes=150)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    if '--trace' in sys.argv:
        summarise(sys.argv[sys.argv.index('--trace') + 1])
    else:
        main()
