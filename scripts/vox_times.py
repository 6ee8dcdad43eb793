"""Times of the device-side hard voxelisation (ddp_amd/vox.py, libddp_vox.so) at the size of the camera + lidar BEV configuration's lidar
branch (about 250 000 points of 5 floats per sample, range +-51.2 m x +-51.2 m x [-5, 3] m, voxels of 0.1 x 0.1 x 0.2 m - a grid of
1024 x 1024 x 40 -, 10 points per voxel, at most 120 000 voxels; B 1 and 4) and, in the same process on the same card, of a torch-ROCm
restatement: a stable sort of the cell ids, ``unique_consecutive``, a scatter.  The protocol is that of scripts/dlss_times.py (HIP
events around replays of a captured graph, after warm-up; the clocks beside them).

    python scripts/vox_times.py [--out profiles/vox1_times.jsonl] [--iters 200]

Per record (one line per batch size, APPENDED to the file):
  cells_us / assign_us / gather_us / pack_us   the library calls, graph replays;  call_us: cells + assign + pack in one graph
  kernel_us                                    per kernel name, the mean device time torch.profiler saw over ``--prof-iters`` eager calls
  torch_us                                     the restatement, eager (its shapes depend on the data: it synchronises and cannot be captured)
  torch_equal                                  the restatement's voxels, coordinates and sizes equal the library's, bit for bit
  *_peak_bytes                                 ``torch.cuda.max_memory_allocated`` over one call (the library allocates nothing: its figure is the
                                               workspace)
No ratio is required of this script; it records.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from ddp_amd import build, vox as L  # noqa: E402
from dlss_times import peak_bytes  # noqa: E402
from eval_times import events_us, graph_us  # noqa: E402
import bench  # noqa: E402

VOXEL, RANGE, T, CAP = [0.1, 0.1, 0.2], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], 10, 120000
POINTS = 250000


def cloud(B, dev):
    """B point lists of about POINTS rows of 5 floats: ranges 2 .. 55 m around the rig (the far ones fall outside), heights -2 .. 3 m,
    a tenth of them parked in one spot (a voxel of thousands of points)"""
    out = []
    for b in range(B):
        g = torch.Generator().manual_seed(40 + b)
        n = POINTS - 1000 * b
        rad, ang = 2.0 + 53.0 * torch.rand(n, generator=g), 2 * math.pi * torch.rand(n, generator=g)
        p = torch.stack([rad * torch.cos(ang), rad * torch.sin(ang), -2.0 + 5.0 * torch.rand(n, generator=g), torch.rand(n, generator=g),
                         torch.zeros(n)], 1)
        p[::10, :3] = torch.tensor([3.0, 4.0, 0.5]) + 0.01 * torch.rand(len(p[::10]), 3, generator=g)
        out.append(p.contiguous().to(dev))
    return out


def torch_voxelize(p, grid, lo, vs):
    """one sample with torch ops -> voxels (M, T, F), coors (M, 3), num (M): the same result as the library"""
    q = torch.floor((p[:, :3] - lo) / vs)
    ok = ((q >= 0) & (q < grid)).all(1)
    idx = torch.nonzero(ok).squeeze(1)
    qi = q[idx].long()
    ids = (qi[:, 0] * int(grid[1]) + qi[:, 1]) * int(grid[2]) + qi[:, 2]
    sid, order = torch.sort(ids, stable=True)
    uniq, counts = torch.unique_consecutive(sid, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    first = idx[order[starts]]                                            # a stable sort keeps a cell's points in index order
    vorder = torch.argsort(first)[:CAP]                                    # voxels in the order of their first point
    voxel_of_seg = torch.full((len(uniq),), -1, dtype=torch.long, device=p.device)
    voxel_of_seg[vorder] = torch.arange(len(vorder), device=p.device)
    seg = torch.repeat_interleave(torch.arange(len(uniq), device=p.device), counts)
    rank = torch.arange(len(sid), device=p.device) - starts[seg]
    keep = (rank < T) & (voxel_of_seg[seg] >= 0)
    voxels = torch.zeros(len(vorder), T, p.shape[1], device=p.device)
    voxels[voxel_of_seg[seg[keep]], rank[keep]] = p[idx[order[keep]]]
    cid = uniq[vorder]
    coors = torch.stack([cid // (int(grid[1]) * int(grid[2])), cid // int(grid[2]) % int(grid[1]), cid % int(grid[2])], 1).int()
    return voxels, coors, counts[vorder].clamp(max=T).int()


def torch_batch(points, grid, lo, vs):
    """``BEVFusion.voxelize`` on top: the batch column, the concatenation, the mean"""
    per = [torch_voxelize(p, grid, lo, vs) for p in points]
    feats = torch.cat([v for v, _, _ in per])
    coords = torch.cat([torch.nn.functional.pad(c, (1, 0), value=k) for k, (_, c, _) in enumerate(per)])
    sizes = torch.cat([n for _, _, n in per])
    return feats.sum(1) / sizes.type_as(feats).view(-1, 1), coords, sizes, feats


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
            if 'k_vox_' in ev.key:
                name = ev.key[ev.key.index('k_vox_'):].split('(')[0].split('E')[0]
                t = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0)
                out[name] = round(out.get(name, 0.0) + t / iters, 3)
        return out or None
    except Exception as e:              # a box without the tracer: the event-timed totals still stand
        print('no per-kernel times:', e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vox1_times.jsonl'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--prof-iters', type=int, default=10)
    ap.add_argument('--torch-iters', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'vox_times.py measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    ps = bench.PowerSampler()
    ps.start()
    lines = []
    for B in (1, 4):
        t_from = time.perf_counter()
        points = cloud(B, dev)
        before = [p.clone() for p in points]
        hv = L.HardVoxelizer(VOXEL, RANGE, T, CAP)
        grid = torch.tensor(hv.grid, device=dev, dtype=torch.float32)
        lo, vs = torch.tensor(RANGE[:3], device=dev), torch.tensor(VOXEL, device=dev)
        feats, coords, sizes = (t.clone() for t in hv.voxelize_batch(points))
        raw = hv.voxelize_batch(points, reduce=False)[0].clone()
        counts = hv.counts()
        pvox = hv.tables()[1]
        want = torch_batch(points, grid, lo, vs)
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(points, before))
        equal = bool(torch.equal(coords, want[1]) and torch.equal(sizes, want[2]) and torch.equal(raw, want[3]))
        rec = dict(record='vox', vox_hash=build.LATER['vox'].hash(), torch=torch.__version__, device=torch.cuda.get_device_name(0), batch=B,
                   grid=hv.grid, max_points=T, max_voxels=CAP, points=[int(p.shape[0]) for p in points], voxels=counts,
                   points_in_a_voxel=int((pvox >= 0).sum()), largest_population=int(torch.bincount(pvox[0][pvox[0] >= 0]).max()),
                   torch_equal=equal, mean_max_abs_vs_torch=float((feats - want[0]).abs().max()), iters=args.iters)
        for _ in range(10):
            hv.cells(points).assign().pack()
        rec['cells_us'] = round(graph_us(lambda: hv.cells(points), args.iters), 3)
        rec['assign_us'] = round(graph_us(lambda: hv.assign(), args.iters), 3)
        rec['gather_us'] = round(graph_us(lambda: hv.gather(), args.iters), 3)
        rec['pack_us'] = round(graph_us(lambda: hv.pack(), args.iters), 3)
        rec['call_us'] = round(graph_us(lambda: hv.cells(points).assign().pack(), args.iters), 3)
        rec['kernel_us'] = kernel_times(lambda: (hv.cells(points).assign().gather(), hv.pack()), args.prof_iters)
        rec['launches'] = dict(cells=B, assign=5 + T, gather=2 * B, pack=1 + 2 * B)
        rec['workspace_bytes'] = hv.workspace_bytes(B, max(int(p.shape[0]) for p in points), 5)
        rec['torch_us'] = round(events_us(lambda: torch_batch(points, grid, lo, vs), args.torch_iters), 1)
        rec['torch_peak_bytes'] = peak_bytes(lambda: torch_batch(points, grid, lo, vs))
        rec['library_faster_than_torch'] = bool(rec['call_us'] < rec['torch_us'])
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del want
    ps.stop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')
    print('appended to', args.out)


if __name__ == '__main__':
    main()
