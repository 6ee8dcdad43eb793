"""``pre_eval`` on the device (second half): what evaluation needs from a map of millions of pixels is 3 x K
counters (seg), ten sums (depth) or K x T x 3 counters (bev).  libddp_eval.so (include/ddp_eval_mi355x.h) reduces them next to
the epilogue that wrote the map; one small device-to-host copy per call replaces the full-size ``.cpu().numpy().astype('int64')``
and the host-side histograms.

  seg    ``seg_pre_eval``    -> per image the 4-tuple of ``intersect_and_union`` (segmentation/mmseg/core/evaluation/metrics.py:26-87)
  depth  ``depth_pre_eval``  -> per image the 9-tuple of ``metrics`` (depth/depth/core/evaluation/metrics.py:7-44)
  bev    ``bev_pre_eval``    -> per sample the (K, T, 3) tp / fp / fn counts of ``evaluate_map`` (bev/mmdet3d/datasets/nuscenes_dataset.py:502-514),
         ``bev_metrics``     -> its dict (:516-523)

The ``*_counts`` / ``*_sums`` functions below them are the raw calls (device tensors in, device tensor out, nothing synchronises):
they are what a hipGraph captures.  There is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _eval_lib as E

BEV_THRESHOLDS = (0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _device_of(tensors, default=None):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if default is not None:
        return torch.device(default)
    return torch.device('cuda', torch.cuda.current_device())


def _as_u8(x, what):
    """-> uint8 tensor, where ``x`` lives; other integer / float dtypes are accepted when every value is an integer in 0..255."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f'{what}: expected a tensor or an ndarray, got {type(x).__name__}')
    if x.dtype == torch.bool:
        x = x.to(torch.uint8)
    if x.dtype != torch.uint8:
        if x.numel() and (float(x.min()) < 0 or float(x.max()) > 255 or (x.is_floating_point() and bool((x != x.round()).any()))):
            raise ValueError(f'{what}: dtype {x.dtype} with values outside the integers 0..255')
        x = x.to(torch.uint8)
    return x


def _squeeze_map(x, what):
    if x.dim() == 3 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 2:
        raise ValueError(f'{what}: expected an (H, W) map, got shape {tuple(x.shape)}')
    return x


def _chunks(n):
    return [(i, min(i + E.MAX_ITEMS, n)) for i in range(0, n, E.MAX_ITEMS)]


# ---- seg -------------------------------------------------------------------------------------------------------------------
def seg_counts(preds, labels, num_classes, ignore_index=255, reduce_zero_label=False, out=None):
    """One ``ddp_eval_seg`` call: ``preds`` / ``labels`` are <= 64 contiguous device uint8 (H, W) maps.  -> ``out``, an
    (n, 3, 256) int32 device tensor of [intersect, pred, label] counts (allocated when None).  Enqueued on the current stream."""
    n = len(preds)
    dev = preds[0].device if n else _device_of(())
    if out is None:
        out = torch.empty((n, 3, E.SEG_BINS), dtype=torch.int32, device=dev)
    items = (E.SegItem * max(n, 1))()
    for i, (p, l) in enumerate(zip(preds, labels)):
        items[i] = E.SegItem(p.data_ptr(), l.data_ptr(), p.shape[0], p.shape[1])
    lib = E.load()
    E.check(lib.ddp_eval_seg(items, n, int(num_classes), int(ignore_index), int(bool(reduce_zero_label)), out.data_ptr(), _stream(dev)), lib)
    return out


def seg_pre_eval(preds, labels, num_classes, ignore_index=255, reduce_zero_label=False, device=None):
    """``preds``: list of device uint8 (H, W) class maps (what ``simple_test(on_device=True)`` returns); ``labels``: the ground
    truth maps, device / CPU tensors or ndarrays (uploaded).  -> per image ``(area_intersect, area_union, area_pred_label,
    area_label)``, CPU float32 tensors of ``num_classes`` entries: drop-in for ``dataset.pre_eval``'s entries.  One device-to-host
    copy of the counter block per call (calls of more than 64 images run in chunks into one block)."""
    if len(preds) != len(labels):
        raise ValueError(f'{len(preds)} predictions for {len(labels)} label maps')
    n = len(preds)
    if n == 0:
        return []
    P = [_squeeze_map(_as_u8(p, f'pred {i}'), f'pred {i}') for i, p in enumerate(preds)]
    L = [_squeeze_map(_as_u8(l, f'label {i}'), f'label {i}') for i, l in enumerate(labels)]
    for i, (p, l) in enumerate(zip(P, L)):
        if p.shape != l.shape:
            raise ValueError(f'image {i}: prediction {tuple(p.shape)} and label {tuple(l.shape)} differ in shape')
    dev = _device_of(P + L, device)
    P = [p.to(dev, non_blocking=True).contiguous() for p in P]
    L = [l.to(dev, non_blocking=True).contiguous() for l in L]
    K = int(num_classes)
    counts = torch.empty((n, 3, E.SEG_BINS), dtype=torch.int32, device=dev)
    for a, b in _chunks(n):
        seg_counts(P[a:b], L[a:b], K, ignore_index, reduce_zero_label, out=counts[a:b])
    c = counts.cpu()[:, :, :K].to(torch.float32)         # the one copy (counts < 2^31 pixels per map; histc returns float32)
    return [(c[i, 0], c[i, 1] + c[i, 2] - c[i, 0], c[i, 1], c[i, 2]) for i in range(n)]


# ---- depth -----------------------------------------------------------------------------------------------------------------
def garg_crop(h, w):
    """(y0, y1, x0, x1) of depth/depth/datasets/kitti.py:246-247."""
    return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)


def eigen_crop(h, w):
    """(y0, y1, x0, x1) of depth/depth/datasets/kitti.py:250-251."""
    return int(0.3324324 * h), int(0.91351351 * h), int(0.0359477 * w), int(0.96405229 * w)


def _depth_items(preds, gts, crops):
    items = (E.DepthItem * max(len(preds), 1))()
    for i, (p, g) in enumerate(zip(preds, gts)):
        h, w = p.shape
        y0, y1, x0, x1 = (0, h, 0, w) if crops is None or crops[i] is None else crops[i]
        items[i] = E.DepthItem(p.data_ptr(), g.data_ptr(), h, w, int(y0), int(y1), int(x0), int(x1))
    return items


def depth_workspace_bytes(shapes):
    """workspace of one ``ddp_eval_depth`` call on maps of these (h, w)"""
    items = (E.DepthItem * max(len(shapes), 1))()
    for i, (h, w) in enumerate(shapes):
        items[i] = E.DepthItem(None, None, h, w, 0, h, 0, w)
    nbytes = C.c_size_t(0)
    lib = E.load()
    E.check(lib.ddp_eval_depth_workspace(items, len(shapes), C.byref(nbytes)), lib)
    return int(nbytes.value)


def depth_sums(preds, gts, min_depth, max_depth, crops=None, out=None, workspace=None):
    """One ``ddp_eval_depth`` call on <= 64 contiguous device float32 (H, W) maps.  -> ``out``, (n, 16) float64 on the device:
    n, the three ratio counts, the six fp64 sums (include/ddp_eval_mi355x.h).  ``workspace``: a device uint8 / float64 tensor of
    ``depth_workspace_bytes`` (allocated when None).  Enqueued on the current stream."""
    n = len(preds)
    dev = preds[0].device if n else _device_of(())
    if out is None:
        out = torch.empty((n, E.DEPTH_COLS), dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(depth_workspace_bytes([tuple(p.shape) for p in preds]) // 8, 1), dtype=torch.float64, device=dev)
    items = _depth_items(preds, gts, crops)
    lib = E.load()
    E.check(lib.ddp_eval_depth(items, n, float(min_depth), float(max_depth), out.data_ptr(), workspace.data_ptr(), _stream(dev)), lib)
    return out


def depth_finalize(row):
    """the 16 columns of one image -> ``(a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel)`` with the rules of
    ``calculate``: no valid pixel -> nine NaN; a NaN silog -> 0.  Host fp64."""
    r = [float(v) for v in row]
    n = r[0]
    if n == 0:
        return (float('nan'),) * 9
    a1, a2, a3 = r[1] / n, r[2] / n, r[3] / n
    abs_rel, sq_rel = r[4] / n, r[9] / n
    rmse = math.sqrt(r[5] / n) if r[5] >= 0 else float('nan')
    log_10 = r[6] / n
    rmse_log = math.sqrt(r[7] / n) if r[7] >= 0 else float('nan')
    var = r[7] / n - (r[8] / n) ** 2
    silog = math.sqrt(var) * 100 if var >= 0 else float('nan')
    if math.isnan(silog):
        silog = 0
    return a1, a2, a3, abs_rel, rmse, log_10, rmse_log, silog, sq_rel


def _as_f32_map(x, what):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise ValueError(f'{what}: expected a float32 tensor or ndarray')
    return _squeeze_map(x, what)


def depth_pre_eval(preds, gts, min_depth, max_depth, crops=None, device=None):
    """``preds``: list of device float32 (1, H, W) / (H, W) maps (``simple_test(on_device=True)``); ``gts``: ground truth maps of the
    same sizes (uploaded when on the host); ``crops``: per image None or the (y0, y1, x0, x1) of ``garg_crop`` / ``eigen_crop``.
    -> per image the nine-tuple of ``metrics(gt[valid], pred[valid], min_depth, max_depth)``, finalised in host fp64."""
    if len(preds) != len(gts) or (crops is not None and len(crops) != len(preds)):
        raise ValueError(f'{len(preds)} predictions, {len(gts)} ground truth maps, {None if crops is None else len(crops)} crops')
    n = len(preds)
    if n == 0:
        return []
    P = [_as_f32_map(p, f'pred {i}') for i, p in enumerate(preds)]
    G = [_as_f32_map(g, f'gt {i}') for i, g in enumerate(gts)]
    for i, (p, g) in enumerate(zip(P, G)):
        if p.shape != g.shape:
            raise ValueError(f'image {i}: prediction {tuple(p.shape)} and ground truth {tuple(g.shape)} differ in shape')
    dev = _device_of(P + G, device)
    P = [p.to(dev, non_blocking=True).contiguous() for p in P]
    G = [g.to(dev, non_blocking=True).contiguous() for g in G]
    sums = torch.empty((n, E.DEPTH_COLS), dtype=torch.float64, device=dev)
    for a, b in _chunks(n):
        depth_sums(P[a:b], G[a:b], min_depth, max_depth, None if crops is None else crops[a:b], out=sums[a:b])
    return [depth_finalize(row) for row in sums.cpu().numpy()]


# ---- bev -------------------------------------------------------------------------------------------------------------------
def bev_counts(probs, gts, thresholds, out=None):
    """One ``ddp_eval_bev`` call: <= 64 contiguous device (K, ...) float32 probability maps and uint8 masks of one size.
    -> ``out``, (n, K, T, 3) int32 [tp, fp, fn] on the device.  Enqueued on the current stream."""
    n = len(probs)
    dev = probs[0].device if n else _device_of(())
    K = int(probs[0].shape[0]) if n else 1
    n_pix = int(probs[0].numel() // K) if n else 1
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if out is None:
        out = torch.empty((n, K, len(thr), 3), dtype=torch.int32, device=dev)
    items = (E.BevItem * max(n, 1))()
    for i, (p, g) in enumerate(zip(probs, gts)):
        items[i] = E.BevItem(p.data_ptr(), g.data_ptr())
    lib = E.load()
    E.check(lib.ddp_eval_bev(items, n, K, n_pix, thr.ctypes.data_as(C.POINTER(C.c_float)), len(thr), out.data_ptr(), _stream(dev)), lib)
    return out


def bev_pre_eval(probs, gt_masks, thresholds=BEV_THRESHOLDS, device=None):
    """``probs``: list of device float32 (K, H, W) maps (``masks_bev``); ``gt_masks``: (K, H, W) bool / uint8 (``gt_masks_bev``).
    -> per sample an int64 (K, T, 3) CPU tensor of tp / fp / fn.  The thresholds are rounded to float32 first, as
    ``torch.tensor([0.35, ...])`` does in the reference."""
    if len(probs) != len(gt_masks):
        raise ValueError(f'{len(probs)} probability maps for {len(gt_masks)} masks')
    n = len(probs)
    if n == 0:
        return []
    dev = _device_of(list(probs) + list(gt_masks), device)
    P, G = [], []
    for i, (p, g) in enumerate(zip(probs, gt_masks)):
        if isinstance(p, np.ndarray):
            p = torch.from_numpy(p)
        if p.dtype != torch.float32:
            raise ValueError(f'prob {i}: expected float32')
        g = _as_u8(g, f'gt mask {i}')
        if p.dim() < 2 or tuple(g.shape) != tuple(p.shape) or tuple(p.shape) != tuple(probs[0].shape):
            raise ValueError(f'sample {i}: probabilities {tuple(p.shape)} / mask {tuple(g.shape)}: one (K, ...) shape per call')
        P.append(p.to(dev, non_blocking=True).contiguous())
        G.append(g.to(dev, non_blocking=True).contiguous())
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    out = torch.empty((n, P[0].shape[0], len(thr), 3), dtype=torch.int32, device=dev)
    for a, b in _chunks(n):
        bev_counts(P[a:b], G[a:b], thr, out=out[a:b])
    c = out.cpu().to(torch.int64)
    return [c[i] for i in range(n)]


def bev_metrics(counts, class_names, thresholds=BEV_THRESHOLDS):
    """``counts``: the per-sample (K, T, 3) tensors of ``bev_pre_eval``.  -> the dict of ``evaluate_map`` (:516-523): float32 running
    sums of tp / fp / fn, iou = tp / (tp + fp + fn + 1e-7)."""
    thr = torch.tensor(list(thresholds))
    K, T = len(class_names), len(thr)
    tp, fp, fn = torch.zeros(K, T), torch.zeros(K, T), torch.zeros(K, T)
    for c in counts:
        c = torch.as_tensor(c)
        tp += c[..., 0]
        fp += c[..., 1]
        fn += c[..., 2]
    ious = tp / (tp + fp + fn + 1e-7)
    metrics = {}
    for index, name in enumerate(class_names):
        metrics[f'map/{name}/iou@max'] = ious[index].max().item()
        for threshold, iou in zip(thr, ious[index]):
            metrics[f'map/{name}/iou@{threshold.item():.2f}'] = iou.item()
    metrics['map/mean/iou@max'] = ious.max(dim=1).values.mean().item()
    return metrics
