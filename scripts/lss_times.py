"""Times of the device-side LSS lift and pool (ddp_amd/lss.py, libddp_lss.so) at the size of the camera-only BEV configuration
(N 6, D 118, 32 x 88 feature pixels, C 80, 256 x 256 x 1 cells; B 1 and 4) and, in the same process on the same box, of a torch-ROCm
restatement of the reference's route: the (B, N, D, fH, fW, C) volume, ``argsort`` of the ranks, ``index_add_`` - with its peak
memory.  The protocol is that of scripts/cm_times.py (HIP events around replays of a captured graph, after warm-up).

    python scripts/lss_times.py [--out profiles/lss1_times.jsonl] [--iters 200]

Per record (one line per batch size, APPENDED to the file):
  plan_us               ``ddp_lss_plan``: memset, ranks + histogram, scan, fill, sort
  pool_us               ``ddp_lss_pool``: pre-pass + pooling kernel, on the plan above
  pool_empty_plan_us    the same call on a plan without a kept point: the pre-pass, and a pooling kernel that only stores zeros - so
                        pool_us - pool_empty_plan_us is what walking the lists and reading the rows costs
  kernel_us             per kernel name, the mean device time torch.profiler saw over ``--prof-iters`` eager calls (None when the
                        profiler gives no device records): the split of plan_us and pool_us
  bytes                 what each kernel moves, counted from the shapes and the plan (rows read = kept points x C x 4)
  torch_route_us        the restated reference route, eager (its temporaries do not fit a graph's private pool gracefully)
  torch_route_peak_bytes   ``torch.cuda.max_memory_allocated`` over one such call, minus what was allocated before it
No ratio is required of this script; it records.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from ddp_amd import build, lss as L  # noqa: E402
from eval_times import HBM_PEAK, events_us, graph_us  # noqa: E402
import bench  # noqa: E402

GEOM = dict(image_size=(256, 704), feature_size=(32, 88), xbound=(-51.2, 51.2, 0.4), ybound=(-51.2, 51.2, 0.4), zbound=(-10.0, 10.0, 20.0),
            dbound=(1.0, 60.0, 0.5), channels=80)
YAWS = (0.0, 55.0, -55.0, 180.0, 110.0, -110.0)


def rig(B, dev):
    """a nuScenes-like rig: six yaws, focal 1266, post_rot 0.48 I, post_trans (-32, -176, 0); sample b turned by b degrees"""
    c2l_r, c2l_t = torch.zeros(B, 6, 3, 3), torch.zeros(B, 6, 3)
    for b in range(B):
        for n, yaw in enumerate(YAWS):
            a = math.radians(yaw + b)
            fwd, right, down = [math.cos(a), math.sin(a), 0.0], [math.sin(a), -math.cos(a), 0.0], [0.0, 0.0, -1.0]
            c2l_r[b, n] = torch.tensor([right, down, fwd]).t()
            c2l_t[b, n] = torch.tensor([1.5 * math.cos(a), 1.5 * math.sin(a), 1.5])
    intr = torch.tensor([[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]]).expand(B, 6, 3, 3)
    post_r = (0.48 * torch.eye(3)).expand(B, 6, 3, 3)
    post_t = torch.tensor([-32.0, -176.0, 0.0]).expand(B, 6, 3)
    extra_r, extra_t = torch.eye(3).expand(B, 3, 3), torch.zeros(B, 3)
    return [t.contiguous().to(dev) for t in (c2l_r, c2l_t, intr, post_r, post_t, extra_r, extra_t)]


def torch_route(pool, mats, x, B):
    """the reference's get_geometry + get_cam_feats + bev_pool as torch device ops: volume, argsort, index_add_"""
    c2l_r, c2l_t, intr, post_r, post_t, extra_r, extra_t = mats
    N, D, C = 6, pool.D, pool.C
    fH, fW = pool.feature_size
    iH, iW = pool.image_size
    dev = x.device
    ds = torch.arange(*GEOM['dbound'], dtype=torch.float, device=dev).view(-1, 1, 1).expand(-1, fH, fW)
    xs = torch.linspace(0, iW - 1, fW, dtype=torch.float, device=dev).view(1, 1, fW).expand(D, fH, fW)
    ys = torch.linspace(0, iH - 1, fH, dtype=torch.float, device=dev).view(1, fH, 1).expand(D, fH, fW)
    pts = torch.stack((xs, ys, ds), -1) - post_t.view(B, N, 1, 1, 1, 3)
    pts = torch.inverse(post_r).view(B, N, 1, 1, 1, 3, 3).matmul(pts.unsqueeze(-1))
    pts = torch.cat((pts[..., :2, :] * pts[..., 2:3, :], pts[..., 2:3, :]), -2)
    pts = c2l_r.matmul(torch.inverse(intr)).view(B, N, 1, 1, 1, 3, 3).matmul(pts).squeeze(-1) + c2l_t.view(B, N, 1, 1, 1, 3)
    pts = extra_r.view(B, 1, 1, 1, 1, 3, 3).matmul(pts.unsqueeze(-1)).squeeze(-1) + extra_t.view(B, 1, 1, 1, 1, 3)
    dx, bx, nx = L.grid_of(GEOM['xbound'], GEOM['ybound'], GEOM['zbound'])
    dx, bx, nx = dx.to(dev), bx.to(dev), nx.to(dev)
    depth = x[:, :D].softmax(dim=1)
    vol = (depth.unsqueeze(1) * x[:, D:D + C].unsqueeze(2)).view(B, N, C, D, fH, fW).permute(0, 1, 3, 4, 5, 2).reshape(-1, C)
    cell = ((pts - (bx - dx / 2.0)) / dx).long().view(-1, 3)
    kept = ((cell >= 0) & (cell < nx)).all(1)
    batch = torch.arange(B, device=dev).repeat_interleave(cell.shape[0] // B)
    rank = ((batch * nx[2] + cell[:, 2]) * nx[0] + cell[:, 0]) * nx[1] + cell[:, 1]
    vol, rank = vol[kept], rank[kept]
    order = rank.argsort()
    out = torch.zeros(B * int(nx[2]) * int(nx[0]) * int(nx[1]), C, device=dev)
    out.index_add_(0, rank[order], vol[order])
    out = out.view(B, int(nx[2]), int(nx[0]), int(nx[1]), C).permute(0, 4, 1, 2, 3)
    return torch.cat(out.unbind(dim=2), 1), int(kept.sum())


def kernel_times(fn, iters):
    """mean device microseconds per kernel name over ``iters`` eager calls, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            if 'k_lss_' in ev.key:
                name = ev.key[ev.key.index('k_lss_'):].split('(')[0].split('E')[0]
                t = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0)
                out[name] = round(out.get(name, 0.0) + t / iters, 3)
        return out or None
    except Exception as e:              # a box without the tracer: the event-timed totals still stand
        print('no per-kernel times:', e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lss1_times.jsonl'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--prof-iters', type=int, default=20)
    ap.add_argument('--torch-iters', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lss_times.py measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    ps = bench.PowerSampler()
    ps.start()
    lines = []
    for B in (1, 4):
        t_from = time.perf_counter()
        pool = L.LssPool(**GEOM)
        mats = rig(B, dev)
        cam, extra = L.pack_cameras(*mats)
        g = torch.Generator().manual_seed(B)
        x = (torch.randn((B * 6, pool.D + pool.C, 32, 88), generator=g) * 2.0).to(dev)
        out = torch.empty((B, pool.C, 256, 256), device=dev)
        pool.plan(cam, extra)
        got = pool.pool(x, out=out).clone()
        ranks = pool.ranks().clone()
        kept = int((ranks >= 0).sum())
        lists = torch.bincount(ranks[ranks >= 0].long(), minlength=B * 65536)
        # agreement with the torch route (same device, fp32 both): the sums differ in order only
        ref, kept_ref = torch_route(pool, mats, x, B)
        torch.cuda.synchronize()
        err = float((got - ref).abs().max() / ref.abs().max())
        P, K, X, C, D = ranks.numel(), B * 65536, B * 6 * 32 * 88, pool.C, pool.D
        rec = dict(record='lss', lss_hash=build.SIDE['lss'].hash(), torch=torch.__version__, device=torch.cuda.get_device_name(0), batch=B, cams=6,
                   depth_bins=D, feature=[32, 88], channels=C, cells=[256, 256, 1], points=P, kept=kept, kept_torch_route=kept_ref,
                   nonempty_cells=int((lists > 0).sum()), mean_list=round(kept / max(int((lists > 0).sum()), 1), 2), longest_list=int(lists.max()),
                   max_rel_vs_torch_route=err, iters=args.iters)
        for _ in range(10):
            pool.plan(cam, extra)
            pool.pool(x, out=out)
        rec['plan_us'] = round(graph_us(lambda: pool.plan(cam, extra), args.iters), 3)
        rec['pool_us'] = round(graph_us(lambda: pool.pool(x, out=out), args.iters), 3)
        rec['kernel_us'] = kernel_times(lambda: (pool.plan(cam, extra), pool.pool(x, out=out)), args.prof_iters)
        pool.plan_from_ranks(torch.full_like(ranks, -1))
        rec['pool_empty_plan_us'] = round(graph_us(lambda: pool.pool(x, out=out), args.iters), 3)
        pool.plan(cam, extra)
        rec['bytes'] = dict(rank=4 * P + 4 * kept, scan=12 * K, fill=4 * P + 12 * kept, sort=8 * K + 8 * kept,
                            pre_read=4 * X * (3 * D + C), pre_write=4 * P + 4 * X * C,
                            pool_lists=8 * K + 8 * kept, pool_rows=4 * kept * C, pool_store=4 * K * C,
                            inputs=4 * X * (D + C), output=4 * K * C, volume_never_formed=4 * P * C)
        rec['pool_store_bytes_per_s'] = round(4 * K * C / (rec['pool_empty_plan_us'] * 1e-6))
        rec['pool_rows_bytes_per_s'] = round(4 * kept * C / (max(rec['pool_us'] - rec['pool_empty_plan_us'], 1e-3) * 1e-6))
        rec['frac_hbm_peak_store'] = round(rec['pool_store_bytes_per_s'] / HBM_PEAK, 4)
        # the torch route: eager, events; peak memory over one call
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch_route(pool, mats, x, B)
        torch.cuda.synchronize()
        rec['torch_route_peak_bytes'] = int(torch.cuda.max_memory_allocated() - base)
        rec['torch_route_us'] = round(events_us(lambda: torch_route(pool, mats, x, B), args.torch_iters), 1)
        rec['workspace_bytes'] = pool.workspace_bytes(B, 6)
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    ps.stop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')
    print('appended to', args.out)


if __name__ == '__main__':
    main()
