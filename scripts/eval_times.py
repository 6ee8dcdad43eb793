"""Per-image times of the device-side pre_eval statistics (ddp_amd/evaluation.py, libddp_eval.so) and, in the same process on the
same box, of the host path the harness runs without ``device_eval``: ``.cpu().numpy().astype('int64')`` + the ``torch.histc``
formulation of ``intersect_and_union`` (seg), ``.cpu().numpy()`` + the nine numpy reductions of ``metrics`` (depth), ``.cpu()`` +
the (classes, pixels, thresholds) boolean tensor of ``evaluate_map`` (bev).

    python scripts/eval_times.py [--out profiles/eval1_times.jsonl] [--iters 300] [--host-iters 10]

Sizes: the ``ori`` sizes of C2 (512 x 1024, 150 classes) and C3 (1024 x 2048, 19 classes), on piecewise-constant maps (64 x 64
and 8 x 8 blocks) and on random maps; depth 352 x 1216 with the Garg rectangle; bev 6 x 200 x 200, 7 thresholds.

Per record:
  graph_us_per_image   HIP events around replays of a captured graph of 10 calls (one image each): memset + kernel(s) + the
                       boundary between them, no host enqueue in the way.  ``bytes_per_s`` = map bytes read / this time.
  eager_us_per_call    HIP events around back-to-back eager calls: what a Python caller gets (the larger of enqueue and device time)
  device_path_wall_us  host clock around ``*_pre_eval`` of one image: uploads excluded (the maps are on the device), the one small
                       device-to-host copy and its synchronisation included
  host_path_wall_us    host clock around today's path, from the same device map, split into the copy (+ cast) and the reduction
with the package power and shader clock over the record's window beside them (bench.PowerSampler).
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
from ddp_amd import build, evaluation as ev  # noqa: E402
import bench  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, the spec figure DESIGN.md quotes fractions of


def block_map(g, h, w, hi, bs, dev):
    small = torch.randint(0, hi, ((h + bs - 1) // bs, (w + bs - 1) // bs), generator=g, dtype=torch.int64)
    return small.repeat_interleave(bs, 0).repeat_interleave(bs, 1)[:h, :w].to(torch.uint8).contiguous().to(dev)


def seg_maps(kind, h, w, K, dev, seed):
    """label: classes + 5 % ignored (255); prediction: the label on about two thirds of the blocks / pixels"""
    g = torch.Generator().manual_seed(seed)
    bs = {'const64': 64, 'const8': 8, 'random': 1}[kind]
    label, other = block_map(g, h, w, K, bs, dev), block_map(g, h, w, K, bs, dev)
    keep = block_map(g, h, w, 3, bs, dev) > 0
    ign = block_map(g, h, w, 20, bs, dev) == 0
    pred = torch.where(keep, label, other)
    return pred.contiguous(), torch.where(ign, torch.full_like(label, 255), label).contiguous()


def intersect_and_union(pred_label, label, num_classes, ignore_index, reduce_zero_label=False):
    """segmentation/mmseg/core/evaluation/metrics.py:58-87 (label_map empty)"""
    pred_label = torch.from_numpy(pred_label)
    label = torch.from_numpy(label)
    if reduce_zero_label:
        label[label == 0] = 255
        label = label - 1
        label[label == 254] = 255
    mask = (label != ignore_index)
    pred_label = pred_label[mask]
    label = label[mask]
    intersect = pred_label[pred_label == label]
    area_intersect = torch.histc(intersect.float(), bins=(num_classes), min=0, max=num_classes - 1)
    area_pred_label = torch.histc(pred_label.float(), bins=(num_classes), min=0, max=num_classes - 1)
    area_label = torch.histc(label.float(), bins=(num_classes), min=0, max=num_classes - 1)
    return area_intersect, area_pred_label + area_label - area_intersect, area_pred_label, area_label


def depth_metrics(gt, pred, min_depth, max_depth):
    """depth/depth/core/evaluation/metrics.py:7-44"""
    mask = np.logical_and(gt > min_depth, gt < max_depth)
    gt, pred = gt[mask], pred[mask]
    if gt.shape[0] == 0:
        return (np.nan,) * 9
    thresh = np.maximum((gt / pred), (pred / gt))
    a1, a2, a3 = (thresh < 1.25).mean(), (thresh < 1.25 ** 2).mean(), (thresh < 1.25 ** 3).mean()
    abs_rel = np.mean(np.abs(gt - pred) / gt)
    sq_rel = np.mean(((gt - pred) ** 2) / gt)
    rmse = np.sqrt(((gt - pred) ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    err = np.log(pred) - np.log(gt)
    silog = np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100
    log_10 = (np.abs(np.log10(gt) - np.log10(pred))).mean()
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, 0 if np.isnan(silog) else silog, sq_rel


def bev_counts_host(pred, label, thresholds):
    """bev/mmdet3d/datasets/nuscenes_dataset.py:506-514"""
    K = pred.shape[0]
    pred = pred.detach().reshape(K, -1)
    label = label.detach().bool().reshape(K, -1)
    pred = pred[:, :, None] >= thresholds
    label = label[:, :, None]
    return (pred & label).sum(dim=1), (pred & ~label).sum(dim=1), (~pred & label).sum(dim=1)


def events_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def graph_us(fn, iters, per_graph=10):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(per_graph):
            fn()
    for _ in range(3):
        graph.replay()
    return events_us(graph.replay, max(iters // per_graph, 5)) / per_graph


def wall_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval1_times.jsonl'))
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--host-iters', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'eval_times.py measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    ps = bench.PowerSampler()
    ps.start()
    lines = [dict(record='header', eval_hash=build.SIDE['eval'].hash(), source_hash=build.source_hash(), torch=torch.__version__,
                  device=torch.cuda.get_device_name(0), iters=args.iters, host_iters=args.host_iters, host_threads=torch.get_num_threads(),
                  power_source=ps.source)]

    def measure(rec, raw, device_path, host_copy, host_reduce, nbytes):
        t_from = time.perf_counter()
        for _ in range(20):
            raw()
        rec['graph_us_per_image'] = round(graph_us(raw, args.iters), 3)
        rec['eager_us_per_call'] = round(events_us(raw, args.iters), 3)
        rec['bytes_read'] = nbytes
        rec['bytes_per_s'] = round(nbytes / (rec['graph_us_per_image'] * 1e-6))
        rec['frac_hbm_peak'] = round(rec['bytes_per_s'] / HBM_PEAK, 4)
        device_path()
        rec['device_path_wall_us'] = round(wall_us(device_path, max(args.iters // 3, 10)), 1)
        host = host_copy()
        host_reduce(host)
        t_copy = wall_us(host_copy, args.host_iters)
        t0 = time.perf_counter()
        for _ in range(args.host_iters):
            host_reduce(host)
        t_red = (time.perf_counter() - t0) * 1e6 / args.host_iters
        rec.update(host_copy_wall_us=round(t_copy, 1), host_reduce_wall_us=round(t_red, 1), host_path_wall_us=round(t_copy + t_red, 1))
        rec['host_over_device'] = round(rec['host_path_wall_us'] / rec['device_path_wall_us'], 1)
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for cfg_name, h, w, K in (('C2', 512, 1024, 150), ('C3', 1024, 2048, 19)):
        for kind in ('const64', 'const8', 'random'):
            pred, label = seg_maps(kind, h, w, K, dev, seed=1)
            label_host = label.cpu().numpy()
            out = torch.empty((1, 3, 256), dtype=torch.int32, device=dev)
            want = intersect_and_union(pred.cpu().numpy().astype('int64'), label_host.copy(), K, 255)
            got = ev.seg_pre_eval([pred], [label], K, 255)[0]
            assert all(torch.equal(a, b) for a, b in zip(want, got)), 'device and host paths disagree'
            measure(dict(record='seg', config=cfg_name, h=h, w=w, num_classes=K, maps=kind),
                    raw=lambda: ev.seg_counts([pred], [label], K, 255, False, out=out),
                    device_path=lambda: ev.seg_pre_eval([pred], [label], K, 255),
                    host_copy=lambda: pred.cpu().numpy().astype('int64'),
                    host_reduce=lambda p: intersect_and_union(p, label_host.copy(), K, 255),
                    nbytes=2 * h * w)

    # the same kernel with a grid that fills the chip: 16 different C3 images in ONE call (8192 blocks, 67 MB read - more than the L2
    # holds): what the kernel streams when the launch and the memset are spread over 16 images
    h, w, K, nb = 1024, 2048, 19, 16
    for kind in ('const64', 'const8', 'random'):
        t_from = time.perf_counter()
        maps = [seg_maps(kind, h, w, K, dev, seed=10 + i) for i in range(nb)]
        P, L = [m[0] for m in maps], [m[1] for m in maps]
        out = torch.empty((nb, 3, 256), dtype=torch.int32, device=dev)
        call = lambda: ev.seg_counts(P, L, K, 255, False, out=out)
        for _ in range(5):
            call()
        us = graph_us(call, max(args.iters // 3, 50), per_graph=5)
        rec = dict(record='seg_batch', config='C3', h=h, w=w, num_classes=K, maps=kind, images_per_call=nb, graph_us_per_call=round(us, 3),
                   graph_us_per_image=round(us / nb, 3), bytes_read=2 * h * w * nb)
        rec['bytes_per_s'] = round(rec['bytes_read'] / (us * 1e-6))
        rec['frac_hbm_peak'] = round(rec['bytes_per_s'] / HBM_PEAK, 4)
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del maps, P, L

    h, w = 352, 1216
    g = torch.Generator().manual_seed(2)
    gt = (torch.rand(h, w, generator=g) * 89.5 + 0.5) * (torch.rand(h, w, generator=g) > 0.2)
    pred = (gt * (torch.rand(h, w, generator=g) + 0.5)).clamp(1e-3, 80) + (gt == 0) * 10.0
    gt_d, pred_d = gt.to(dev).contiguous(), pred.to(dev).contiguous()[None]
    crop = ev.garg_crop(h, w)
    gt_host = gt.numpy()
    mask = np.zeros((h, w), dtype=bool)
    mask[crop[0]:crop[1], crop[2]:crop[3]] = True
    sums = torch.empty((1, 16), dtype=torch.float64, device=dev)
    ws = torch.empty(ev.depth_workspace_bytes([(h, w)]) // 8, dtype=torch.float64, device=dev)
    measure(dict(record='depth', h=h, w=w, crop='garg'),
            raw=lambda: ev.depth_sums([pred_d[0]], [gt_d], 1e-3, 80, [crop], out=sums, workspace=ws),
            device_path=lambda: ev.depth_pre_eval([pred_d], [gt_d], 1e-3, 80, crops=[crop]),
            host_copy=lambda: pred_d.cpu().numpy(),
            host_reduce=lambda p: depth_metrics(gt_host[mask], p[0][mask], 1e-3, 80),
            nbytes=8 * h * w)

    K, n = 6, 200
    g = torch.Generator().manual_seed(3)
    prob = torch.rand(K, n, n, generator=g).to(dev)
    mask_h = torch.rand(K, n, n, generator=g) < 0.4
    mask_d = mask_h.to(torch.uint8).to(dev)
    thr = torch.tensor(list(ev.BEV_THRESHOLDS))
    bout = torch.empty((1, K, len(thr), 3), dtype=torch.int32, device=dev)
    measure(dict(record='bev', num_classes=K, h=n, w=n, thresholds=len(thr)),
            raw=lambda: ev.bev_counts([prob], [mask_d], ev.BEV_THRESHOLDS, out=bout),
            device_path=lambda: ev.bev_pre_eval([prob], [mask_d]),
            host_copy=lambda: prob.cpu(),
            host_reduce=lambda p: bev_counts_host(p, mask_h, thr),
            nbytes=5 * K * n * n)
    ps.stop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
