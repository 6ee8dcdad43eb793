"""Times of the device-side front of ``DepthLSSTransform`` (ddp_amd/dlss.py, libddp_dlss.so) at the size of the camera + lidar BEV
configuration (6 cameras of 256 x 704, about 250 000 lidar points per sample on the six-yaw rig; B 1 and 4) and, in the same process on
the same card, of the torch-ROCm restatement of each step: the reference's Python loop over samples and cameras with its indexed
assignment (bev/mmdet3d/models/vtransforms/base.py:243-279), and eager ``dtransform[0:6]``.  The protocol is that of
scripts/lss_times.py (HIP events around replays of a captured graph, after warm-up).

    python scripts/dlss_times.py [--out profiles/dlss1_times.jsonl] [--iters 200]

Per record (one line per batch size, APPENDED to the file):
  project_us / scatter_us / stem_us      the library calls, graph replays
  kernel_us                              per kernel name, the mean device time torch.profiler saw over ``--prof-iters`` eager calls
  torch_project_us / torch_scatter_us    the reference's chain up to ``on_img`` / its masked indexed assignment, eager (boolean-mask indexing
                                         synchronises: it cannot be captured)
  torch_stem_us, torch_stem_graph_us     eager ``dtransform[0:6]`` with HIP events, and the same six modules replayed from a graph
  *_peak_bytes                           ``torch.cuda.max_memory_allocated`` over one call, minus what was allocated before it (the library
                                         routes allocate nothing: their figure is the workspace)
  stem_faster_than_eager                 the keep-or-drop figure of the stem at B = 1: stem_us < min(torch_stem_us, torch_stem_graph_us)
No ratio is required of this script; it records.
"""
import argparse
import json
import math
import os
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from ddp_amd import build, dlss as L  # noqa: E402
from eval_times import events_us, graph_us  # noqa: E402
import bench  # noqa: E402

IMAGE = (256, 704)
YAWS = (0.0, 55.0, -55.0, 180.0, 110.0, -110.0)
POINTS = 250000


def rig(B, dev):
    """a nuScenes-like rig: six yaws, focal 1266, img_aug 0.48 I + (-32, -176, 0); sample b turned by b degrees; lidar_aug a small turn,
    scale and shift -> lidar2image, img_aug (B, 6, 4, 4), lidar_aug (B, 4, 4)"""
    l2i, aug, laug = torch.zeros(B, 6, 4, 4, dtype=torch.float64), torch.zeros(B, 6, 4, 4, dtype=torch.float64), torch.zeros(B, 4, 4, dtype=torch.float64)
    k = torch.eye(4, dtype=torch.float64)
    k[0, 0] = k[1, 1] = 1266.4
    k[0, 2], k[1, 2] = 816.3, 491.5
    for b in range(B):
        for n, yaw in enumerate(YAWS):
            a = math.radians(yaw + b)
            fwd, right, down = [math.cos(a), math.sin(a), 0.0], [math.sin(a), -math.cos(a), 0.0], [0.0, 0.0, -1.0]
            c2l = torch.eye(4, dtype=torch.float64)
            c2l[:3, :3] = torch.tensor([right, down, fwd], dtype=torch.float64).t()
            c2l[:3, 3] = torch.tensor([1.5 * math.cos(a), 1.5 * math.sin(a), 1.5], dtype=torch.float64)
            l2i[b, n] = k @ torch.inverse(c2l)
            aug[b, n] = torch.eye(4, dtype=torch.float64)
            aug[b, n, 0, 0] = aug[b, n, 1, 1] = 0.48
            aug[b, n, :3, 3] = torch.tensor([-32.0, -176.0, 0.0], dtype=torch.float64)
        t = math.radians(3.0 + b)
        laug[b] = torch.eye(4, dtype=torch.float64)
        laug[b, :3, :3] = 1.02 * torch.tensor([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
        laug[b, :3, 3] = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    return [t.float().contiguous().to(dev) for t in (l2i, aug, laug)]


def cloud(B, dev):
    """B point lists of about POINTS rows of 5 floats: ranges 2 .. 55 m around the rig, heights -2 .. 3 m"""
    out = []
    for b in range(B):
        g = torch.Generator().manual_seed(40 + b)
        n = POINTS - 1000 * b
        rad, ang = 2.0 + 53.0 * torch.rand(n, generator=g), 2 * math.pi * torch.rand(n, generator=g)
        out.append(torch.stack([rad * torch.cos(ang), rad * torch.sin(ang), -2.0 + 5.0 * torch.rand(n, generator=g), torch.rand(n, generator=g),
                                torch.zeros(n)], 1).contiguous().to(dev))
    return out


def torch_project(points, l2i, aug, laug):
    """base.py:243-275 per sample, on copies of the points -> [(coords (N, P, 2), on_img (N, P), dist (N, P))]"""
    out = []
    for b in range(len(points)):
        cur = points[b][:, :3].clone()
        cur -= laug[b][:3, 3]
        cur = torch.inverse(laug[b][:3, :3]).matmul(cur.transpose(1, 0))
        cur = l2i[b][:, :3, :3].matmul(cur)
        cur += l2i[b][:, :3, 3].reshape(-1, 3, 1)
        dist = cur[:, 2, :]
        cur[:, 2, :] = torch.clamp(cur[:, 2, :], 1e-5, 1e5)
        cur[:, :2, :] /= cur[:, 2:3, :]
        cur = aug[b][:, :3, :3].matmul(cur)
        cur += aug[b][:, :3, 3].reshape(-1, 3, 1)
        cur = cur[:, :2, :].transpose(1, 2)[..., [1, 0]]
        on = (cur[..., 0] < IMAGE[0]) & (cur[..., 0] >= 0) & (cur[..., 1] < IMAGE[1]) & (cur[..., 1] >= 0)
        out.append((cur, on, dist))
    return out


def torch_scatter(proj, N, dev):
    """base.py:239-241, 276-279: zeros, then per sample and camera the masked indexed assignment (duplicates: undefined winner)"""
    depth = torch.zeros(len(proj), N, 1, *IMAGE, device=dev)
    for b, (cur, on, dist) in enumerate(proj):
        for c in range(N):
            mc = cur[c, on[c]].long()
            depth[b, c, 0, mc[:, 0], mc[:, 1]] = dist[c, on[c]]
    return depth


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated() - base)
    del keep
    return peak


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
            if 'k_dlss_' in ev.key:
                name = ev.key[ev.key.index('k_dlss_'):].split('(')[0].split('E')[0]
                t = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0)
                out[name] = round(out.get(name, 0.0) + t / iters, 3)
        return out or None
    except Exception as e:              # a box without the tracer: the event-timed totals still stand
        print('no per-kernel times:', e, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dlss1_times.jsonl'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--prof-iters', type=int, default=20)
    ap.add_argument('--torch-iters', type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'dlss_times.py measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    dtransform = nn.Sequential(nn.Conv2d(1, 8, 1), nn.BatchNorm2d(8), nn.ReLU(True), nn.Conv2d(8, 32, 5, stride=4, padding=2), nn.BatchNorm2d(32),
                               nn.ReLU(True)).to(dev).eval()
    with torch.no_grad():
        for mod in dtransform:
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.25, 0.25)
                mod.running_var.uniform_(0.5, 1.5)
    ps = bench.PowerSampler()
    ps.start()
    lines = []
    for B in (1, 4):
        t_from = time.perf_counter()
        l2i, aug, laug = rig(B, dev)
        points = cloud(B, dev)
        before = [p.clone() for p in points]
        ld = L.LidarDepth(IMAGE)
        lidar, cam = L.pack_lidar(l2i, aug, laug)
        pmax = max(int(p.shape[0]) for p in points)
        image = torch.empty((B, 6, 1) + IMAGE, device=dev)
        stem_out = torch.empty((B * 6, 32) + L.stem_size(IMAGE), device=dev)
        ld.project_packed(points, lidar, cam)
        ld.scatter(out=image)
        ld.stem(image, dtransform, out=stem_out)
        pix, dep = ld.tables()
        on = int((pix >= 0).sum())
        lit = int((image != 0).sum())
        # agreement with the torch route on this card: same pixels lit; depths equal except on contested pixels (its winner is undefined)
        with torch.no_grad():
            proj = torch_project(points, l2i, aug, laug)
            ref_image = torch_scatter(proj, 6, dev)
            ref_stem = dtransform(ref_image.flatten(0, 1).clone())
            my_on_ref = dtransform(image.flatten(0, 1).clone())
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(points, before))
        rec = dict(record='dlss', dlss_hash=build.SIDE['dlss'].hash(), torch=torch.__version__, device=torch.cuda.get_device_name(0), batch=B, cams=6,
                   image=list(IMAGE), points=[int(p.shape[0]) for p in points], pmax=pmax, on_image_pairs=on, lit_pixels=lit,
                   lit_share=round(lit / image.numel(), 5), pixels_lit_differently_from_torch=int(((image != 0) != (ref_image != 0)).sum()),
                   pixels_with_another_depth_than_torch=int((image != ref_image).sum()), contested_pairs=on - lit,
                   stem_max_abs_vs_eager_on_the_same_image=float((stem_out - my_on_ref).abs().max()), stem_abs_max=float(my_on_ref.abs().max()),
                   iters=args.iters)
        del ref_stem
        for _ in range(10):
            ld.project_packed(points, lidar, cam)
            ld.scatter(out=image)
            ld.stem(image, dtransform, out=stem_out)
        rec['project_us'] = round(graph_us(lambda: ld.project_packed(points, lidar, cam), args.iters), 3)
        rec['scatter_us'] = round(graph_us(lambda: ld.scatter(out=image), args.iters), 3)
        rec['stem_us'] = round(graph_us(lambda: ld.stem(image, dtransform, out=stem_out), args.iters), 3)
        rec['kernel_us'] = kernel_times(lambda: (ld.project_packed(points, lidar, cam), ld.scatter(out=image), ld.stem(image, dtransform, out=stem_out)),
                                        args.prof_iters)
        rec['workspace_bytes'] = ld.workspace_bytes(B, 6, pmax)
        rec['bytes'] = dict(project_read=sum(12 * int(p.shape[0]) for p in points), project_write=8 * B * 6 * pmax, vote_read=4 * B * 6 * pmax,
                            winner=2 * 4 * image.numel(), image_write=4 * image.numel(), stem_read=4 * image.numel(), stem_write=4 * stem_out.numel(),
                            stage1_never_stored=4 * 8 * image.numel())
        with torch.no_grad():
            rec['torch_project_us'] = round(events_us(lambda: torch_project(points, l2i, aug, laug), args.torch_iters), 1)
            rec['torch_scatter_us'] = round(events_us(lambda: torch_scatter(proj, 6, dev), args.torch_iters), 1)
            rec['torch_project_peak_bytes'] = peak_bytes(lambda: torch_project(points, l2i, aug, laug))
            rec['torch_scatter_peak_bytes'] = peak_bytes(lambda: torch_scatter(proj, 6, dev))
            flat = image.flatten(0, 1)
            for _ in range(5):
                dtransform(flat.clone())
            rec['torch_stem_us'] = round(events_us(lambda: dtransform(flat), max(args.iters // 4, 10)), 3)   # ReLU in place on temporaries only
            rec['torch_stem_graph_us'] = round(graph_us(lambda: dtransform(flat), args.iters), 3)
            rec['torch_stem_peak_bytes'] = peak_bytes(lambda: dtransform(flat))
        rec['stem_faster_than_eager'] = bool(rec['stem_us'] < min(rec['torch_stem_us'], rec['torch_stem_graph_us']))
        pw = ps.summary(t_from, time.perf_counter()) or {}
        rec.update(power_w=pw.get('power_w'), sclk_mhz=pw.get('sclk_mhz'), sclk_mhz_min=pw.get('sclk_mhz_min'))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del proj, ref_image, my_on_ref
    ps.stop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')
    print('appended to', args.out)


if __name__ == '__main__':
    main()
