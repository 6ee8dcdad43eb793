#!/usr/bin/env python
"""Per-CALL times of the BEV sampler's head variants at the C5 size (8 x 200 x 200, K = 3) in ONE process, taken the way
scripts/call_times.py takes them (HIP events around every sample() call, package power and shader clock beside them):

  python scripts/bev_head_times.py --calls 20 --blocks 2 > profiles/<tag>_bev_head_times.jsonl

Variants: head1x1 (the product path; prescale 1), head3x3 (seg_conv_kernel = 3), prescale2 (prescale_factor = 2, 1x1 head).
--once NAME: prepare one variant and run `--calls` calls only (for a rocprofv3 --kernel-trace --stats pass of its kernels)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ddp_amd.engine import DDPEngine  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402
import bench  # noqa: E402

VARIANTS = {'head1x1': dict(), 'head3x3': dict(bev_seg_kernel=3), 'prescale2': dict(bev_prescale=2.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='bev_fusion_k3_8x200x200')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=2)
    ap.add_argument('--once', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    wl = bench.WORKLOADS[args.workload]
    cx = wl.get('feat_channels', 256)
    x, noise = synthetic.make_inputs(wl['batch'], wl['h'], wl['w'], wl['randsteps'], cx, 256, seed=0)
    dx, dn = x.to(dev), noise.to(dev)
    kw = dict(h=wl['h'], w=wl['w'], batch=wl['batch'], randsteps=wl['randsteps'], timesteps=wl['timesteps'], num_classes=wl['num_classes'],
              bit_scale=wl['bit_scale'], feat_channels=cx, device=dev, bev_input_scope=wl['bev_input_scope'],
              bev_output_scope=wl['bev_output_scope'])
    engines = {}
    for name, over in VARIANTS.items():
        if args.once and name != args.once:
            continue
        sd = synthetic.make_state_dict('bev', wl['num_classes'], wl['num_layers'], cx, seed=2, seg_conv_kernel=over.get('bev_seg_kernel', 1))
        engines[name] = DDPEngine(sd, 'bev', **kw, **over)
        engines[name].prepare()
        engines[name].sample(dx, dn)
    torch.cuda.synchronize()
    out = torch.empty(engines[next(iter(engines))].out_shape(), dtype=torch.float32, device=dev)
    if args.once:
        for _ in range(args.calls):
            engines[args.once].sample(dx, dn, out=out)
        torch.cuda.synchronize()
        return
    ps = bench.PowerSampler(0, period=0.01)
    ps.start()
    for blk in range(args.blocks):
        for name, eng in engines.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for i in range(args.calls):
                eng.sample(dx, dn, out=out)
                ev[i + 1].record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.calls)]
            pw = ps.summary(t0, t1) or {}
            s = sorted(ms)
            print(json.dumps(dict(variant=name, block=blk, median_ms=round(s[len(s) // 2], 3), min_ms=round(s[0], 3), max_ms=round(s[-1], 3),
                                  mean_ms=round(sum(ms) / len(ms), 3), power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'),
                                  sclk_mhz_min=pw.get('sclk_mhz_min'), workspace_bytes=eng.workspace.numel() * 4)), flush=True)
    ps.stop()


if __name__ == '__main__':
    main()
