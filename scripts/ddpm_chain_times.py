#!/usr/bin/env python
"""DDP_FLAG_DDPM_CHAIN against the flag-clear ddpm sampler: per-call HIP-event times in ONE process, alternating blocks, unseeded and
seeded, optionally with another build of the library (the parent commit's) in the same run.

  python scripts/ddpm_chain_times.py --shape headline --calls 10 --blocks 3 [--parent-lib /path/to/libddp_mi355x.so]

One JSON line per (shape, variant, block): median / min / max ms per call; one line per shape with what the outputs say
(flag-clear outputs ``bit_identical_to_first`` across builds and seeded / unseeded feeds of the same noise; chain vs flag clear
max-rel, free running) and the pre-pass kernel's time from the library's launch records against its bytes and flops."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ddp_amd import _lib  # noqa: E402
from ddp_amd.engine import DDPEngine, PackedWeights  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402

SHAPES = {
    # the headline shape (bench.py ade_swin_t_k3_8x512x1024) and the Cityscapes shape, sampled with ddpm
    'headline': dict(batch=8, h=128, w=256, timesteps=3, num_classes=150, time_difference=1),
    'city': dict(batch=4, h=256, w=512, timesteps=10, num_classes=19, time_difference=1),
}
SEED = 2024


def tag0(eng, *args, **kw):
    """(total ms, launches) under profiler tag 0 of one sample() call"""
    lib = eng.lib
    torch.cuda.synchronize()
    ms, n = C.c_float(0), C.c_int(0)
    _lib.check(lib.ddp_profile_begin(255), lib)
    try:
        eng.sample(*args, **kw)
        torch.cuda.synchronize()
    finally:
        rc = lib.ddp_profile_end(C.byref(ms), C.byref(n))
    _lib.check(rc, lib)
    _lib.check(lib.ddp_profile_read(0, C.byref(ms), C.byref(n)), lib)
    return ms.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='headline', choices=sorted(SHAPES))
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--layers', type=int, default=6)
    ap.add_argument('--parent-lib', default=None, help='another build of libddp_mi355x.so (same ABI): timed flag clear in the same run')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    sh = SHAPES[args.shape]
    B, h, w, K = sh['batch'], sh['h'], sh['w'], sh['timesteps']
    sd = synthetic.make_state_dict('seg', sh['num_classes'], args.layers, 256, seed=2)
    weights = PackedWeights(sd, 'seg', args.layers, dev)
    x, noise = synthetic.make_inputs(B, h, w, 1, 256, 256, seed=0)
    dx = x.to(dev)
    kw = dict(h=h, w=w, batch=B, randsteps=1, timesteps=K, num_classes=sh['num_classes'], bit_scale=0.01, accumulation=True,
              time_difference=sh['time_difference'], sampler='ddpm', device=dev, weights=weights)
    builds = [('new', None)] + ([('parent', args.parent_lib)] if args.parent_lib else [])
    engines = {}
    for bname, path in builds:
        for seeded in (False, True):
            for chain in ((False, True) if bname == 'new' else (False,)):
                name = f'{bname}_{"chain" if chain else "clear"}{"_seeded" if seeded else ""}'
                extra = dict(ddpm_chain=chain) if bname == 'new' else {}
                engines[name] = DDPEngine(sd, 'seg', lib_path=path, seeded_noise=seeded, **extra, **kw)
                engines[name].prepare()
    # the noise the seeded engines generate, handed to the unseeded ones: every variant samples the SAME problem
    gen = DDPEngine(sd, 'seg', seeded_noise=True, **dict(kw, sampler='ddim'))
    adds = [int(s.ddpm_add_noise) for s in engines['new_clear'].steps]
    gen.sample(dx, seed=SEED)
    dn = gen.last_noise().clone()
    dsn = torch.zeros((K,) + tuple(dn.shape), device=dev)
    for s, a in enumerate(adds):
        if a:
            gen.sample(dx, seed=SEED, stream_base=1 + s)
            dsn[s] = gen.last_noise()
    del gen

    def run(name, out=None):
        eng = engines[name]
        return eng.sample(dx, seed=SEED, out=out) if eng.seeded else eng.sample(dx, dn, dsn, out=out)

    outs = {n: run(n).clone() for n in engines}
    torch.cuda.synchronize()
    first = outs['new_clear']
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())          # noqa: E731
    info = dict(shape=args.shape, **sh, layers=args.layers, noise_adding_steps=adds,
                bit_identical_to_first={n: bool(torch.equal(o, first)) for n, o in outs.items() if 'clear' in n},
                chain_vs_clear_max_rel_free_running=rel(outs['new_chain'], first),
                chain_seeded_equals_chain=bool(torch.equal(outs['new_chain_seeded'], outs['new_chain'])),
                chain_argmax_agreement=float((outs['new_chain'].argmax(1) == first.argmax(1)).float().mean()))
    ms, n = tag0(engines['new_chain'], dx, dn, dsn)
    M = B * h * w
    if n:
        per = ms / n
        info['prepass'] = dict(launches=n, ms_per_launch=round(per, 4), bytes=3 * M * 1024, flops=2 * M * 256 * 256,
                               gb_per_s=round(3 * M * 1024 / per / 1e6, 1), tflops=round(2 * M * 65536 / per / 1e9, 2))
    print(json.dumps(info), flush=True)
    out = torch.empty_like(first)
    for blk in range(args.blocks):
        for name in engines:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(args.calls):
                run(name, out)
                ev[i + 1].record()
            torch.cuda.synchronize()
            t = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.calls))
            print(json.dumps(dict(shape=args.shape, variant=name, block=blk, median_ms=round(t[len(t) // 2], 3), min_ms=round(t[0], 3),
                                  max_ms=round(t[-1], 3))), flush=True)


if __name__ == '__main__':
    main()
