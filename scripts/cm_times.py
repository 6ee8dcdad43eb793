"""Per-image times of the device-side confusion matrix (ddp_amd/confusion.py, libddp_cm.so) and, in the same process on the same
box, of ``ddp_eval_seg`` on the same maps and of the host path of the reference's tools/confusion_matrix.py: the
``.cpu().numpy()`` copy of the class map + the tool's ``bincount`` lines.  The protocol is that of scripts/eval_times.py.

    python scripts/cm_times.py [--out profiles/cm1_times.jsonl] [--iters 300] [--host-iters 10]

Sizes: the ``ori`` sizes of C2 (512 x 1024, 150 classes) and C3 (1024 x 2048, 19 classes), on piecewise-constant maps (64 x 64
and 8 x 8 blocks) and on random maps; 16 C3 images in one call; the ``all_keys`` pattern (label = y mod 256, prediction = x mod
256: every block meets 8192 distinct keys) tiled to C3 size at 256 classes.

Per record:
  graph_us_per_image        HIP events around replays of a captured graph of 10 accumulating calls (one image each)
  eval_seg_graph_us         the same for ``ddp_eval_seg`` (memset + kernel) on the same maps
  device_path_wall_us       host clock around ``iters`` ``ConfusionMatrix.update`` calls of one image each AND the one
                            ``result()`` at the end, divided by ``iters``: the final copy amortised over fewer images than any of
                            the reference's validation sets holds
  host_path_wall_us         host clock around the tool's path from the same device map, split into the copy and the reduction
The script FAILS when, on a piecewise-constant kind, host_path_wall_us / device_path_wall_us is below 10 (the bound the library was
built to: the sibling kernel reached 34 - 265 x on the same bytes with 3 K bins, and this one reads the same bytes, so less would mean
that the table design failed).  Random maps and ``all_keys`` are recorded only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from ddp_amd import build, confusion as cf, evaluation as ev  # noqa: E402
from eval_times import HBM_PEAK, events_us, graph_us, seg_maps, wall_us  # noqa: E402
import bench  # noqa: E402

GATE = 10.0


def tool_lines(res_segm, gt_segm, n, ignore_index):
    """segmentation/tools/confusion_matrix.py:60-65"""
    gt_segm = gt_segm.astype(int)
    gt_segm, res_segm = gt_segm.flatten(), res_segm.flatten()
    to_ignore = gt_segm == ignore_index
    gt_segm, res_segm = gt_segm[~to_ignore], res_segm[~to_ignore]
    inds = n * gt_segm + res_segm
    return np.bincount(inds, minlength=n**2).reshape(n, n)


def all_keys_maps(h, w, dev):
    y = (torch.arange(h) % 256).to(torch.uint8)[:, None].expand(h, w)
    x = (torch.arange(w) % 256).to(torch.uint8)[None, :].expand(h, w)
    return x.contiguous().to(dev), y.contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cm1_times.jsonl'))
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--host-iters', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'cm_times.py measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    ps = bench.PowerSampler()
    ps.start()
    lines = [dict(record='header', cm_hash=build.SIDE['cm'].hash(), eval_hash=build.SIDE['eval'].hash(), source_hash=build.source_hash(),
                  torch=torch.__version__, device=torch.cuda.get_device_name(0), iters=args.iters, host_iters=args.host_iters,
                  host_threads=torch.get_num_threads(), gate=GATE, power_source=ps.source)]
    failed = []

    def measure(rec, pred, label, K, ign, gated):
        t_from = time.perf_counter()
        h, w = pred.shape
        label_host = label.cpu().numpy()
        want = tool_lines(pred.cpu().numpy(), label_host, K, ign)
        got = cf.seg_confusion([pred], [label], K, ign).cpu().numpy()
        assert np.array_equal(got, want), 'device and host paths disagree'
        matrix = torch.zeros((K, K), dtype=torch.int64, device=dev)
        tally = torch.zeros(4, dtype=torch.int64, device=dev)
        counts = torch.empty((1, 3, 256), dtype=torch.int32, device=dev)
        raw = lambda: cf.seg_confusion([pred], [label], K, ign, False, accumulate=True, out=matrix, tally=tally)
        raw_eval = lambda: ev.seg_counts([pred], [label], K, ign, False, out=counts)
        for _ in range(20):
            raw()
            raw_eval()
        rec['graph_us_per_image'] = round(graph_us(raw, args.iters), 3)
        rec['eager_us_per_call'] = round(events_us(raw, args.iters), 3)
        rec['eval_seg_graph_us'] = round(graph_us(raw_eval, args.iters), 3)
        rec['bytes_read'] = 2 * h * w
        rec['bytes_per_s'] = round(rec['bytes_read'] / (rec['graph_us_per_image'] * 1e-6))
        rec['frac_hbm_peak'] = round(rec['bytes_per_s'] / HBM_PEAK, 4)
        cm = cf.ConfusionMatrix(K, ign)
        cm.update([pred], [label]).result()
        cm.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            cm.update([pred], [label])
        res = cm.result()                                # the one copy (it synchronises)
        rec['device_path_wall_us'] = round((time.perf_counter() - t0) * 1e6 / args.iters, 2)
        assert np.array_equal(res, want.astype(np.float64) * args.iters)
        host_copy = lambda: pred.cpu().numpy()
        host = host_copy()
        t_copy = wall_us(host_copy, args.host_iters)
        t0 = time.perf_counter()
        for _ in range(args.host_iters):
            tool_lines(host, label_host, K, ign)
        t_red = (time.perf_counter() - t0) * 1e6 / args.host_iters
        rec.update(host_copy_wall_us=round(t_copy, 1), host_reduce_wall_us=round(t_red, 1), host_path_wall_us=round(t_copy + t_red, 1))
        rec['host_over_device'] = round(rec['host_path_wall_us'] / rec['device_path_wall_us'], 1)
        rec['gated'] = gated
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if gated and rec['host_over_device'] < GATE:
            failed.append(rec)

    for cfg_name, h, w, K in (('C2', 512, 1024, 150), ('C3', 1024, 2048, 19)):
        for kind in ('const64', 'const8', 'random'):
            pred, label = seg_maps(kind, h, w, K, dev, seed=1)
            measure(dict(record='cm', config=cfg_name, h=h, w=w, num_classes=K, maps=kind), pred, label, K, 255, gated=kind != 'random')
    pred, label = all_keys_maps(1024, 2048, dev)
    measure(dict(record='cm', config='all_keys', h=1024, w=2048, num_classes=256, maps='all_keys'), pred, label, 256, -1, gated=False)

    # 16 different C3 images in ONE call (8192 blocks, 67 MB read - more than the L2 holds)
    h, w, K, nb = 1024, 2048, 19, 16
    for kind in ('const64', 'const8', 'random'):
        t_from = time.perf_counter()
        maps = [seg_maps(kind, h, w, K, dev, seed=10 + i) for i in range(nb)]
        P, L = [m[0] for m in maps], [m[1] for m in maps]
        matrix = torch.zeros((K, K), dtype=torch.int64, device=dev)
        counts = torch.empty((nb, 3, 256), dtype=torch.int32, device=dev)
        call = lambda: cf.seg_confusion(P, L, K, 255, False, accumulate=True, out=matrix)
        call_eval = lambda: ev.seg_counts(P, L, K, 255, False, out=counts)
        for _ in range(5):
            call()
            call_eval()
        us = graph_us(call, max(args.iters // 3, 50), per_graph=5)
        us_eval = graph_us(call_eval, max(args.iters // 3, 50), per_graph=5)
        rec = dict(record='cm_batch', config='C3', h=h, w=w, num_classes=K, maps=kind, images_per_call=nb, graph_us_per_call=round(us, 3),
                   graph_us_per_image=round(us / nb, 3), eval_seg_graph_us_per_image=round(us_eval / nb, 3), bytes_read=2 * h * w * nb)
        rec['bytes_per_s'] = round(rec['bytes_read'] / (us * 1e-6))
        rec['frac_hbm_peak'] = round(rec['bytes_per_s'] / HBM_PEAK, 4)
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del maps, P, L
    ps.stop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')
    print('wrote', args.out)
    if failed:
        raise SystemExit(f'host path / device path below {GATE} x on: ' + ', '.join(f"{r['config']} {r['maps']} ({r['host_over_device']} x)" for r in failed))


if __name__ == '__main__':
    main()
