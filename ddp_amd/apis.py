"""Test harness around the sampling loop: ``single_gpu_test`` / ``multi_gpu_test`` with the call
protocol of segmentation/mmseg/apis/test.py:34-229 - ``model(return_loss=False, [rescale=True,] **data)`` per batch of a
DataLoader, per-image results appended in dataset order, optional ``dataset.pre_eval`` / ``dataset.format_results`` -
and the result collection of mmcv's ``collect_results_gpu`` / ``collect_results_cpu`` (rank-interleaved order of a
``DistributedSampler(shuffle=False)``, padding samples cut off at ``len(dataset)``, list on rank 0 and ``None`` elsewhere).

Two things differ from the reference on purpose:
  * ``samples_per_gpu > 1`` is valid (the reference is hard-wired to one image per GPU and iteration: "only
    samples_per_gpu=1 valid now", test.py:124-125,210-211): the MI355X sampler takes b >= 1 images with independent
    noise, ``DDP.simple_test`` returns one map per image and ``pre_eval`` is called per image with its own index;
  * nothing is exchanged between ranks while the loader runs - the only collective is ONE ``all_gather_object`` (RCCL
    when the process group is 'nccl', gloo in the CPU tests) or one shared-directory exchange at the very end.
"""
import os
import pickle
import shutil
import tempfile

import torch
import torch.distributed as dist


def _dist_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _model_device(model):
    for p in model.parameters():
        return p.device
    return torch.device('cpu')


def _to_device(data, device):
    """the loader hands over host tensors (the reference relies on MMDataParallel.scatter for this step)."""
    if torch.is_tensor(data):
        return data.to(device, non_blocking=True)
    if isinstance(data, (list, tuple)):
        return type(data)(_to_device(d, device) for d in data)
    return data


def _run_batch(model, data, device, batch_indices=None, **kwargs):
    from .engine import CALLER_INPUTS
    data = dict(data)
    data['img'] = _to_device(data['img'], device)
    # the conditioning entries of the batch (DDP.forward(hints=, prior=, class_prior=, score_prior=)): on the device of img, passed
    # through with **data
    for row in CALLER_INPUTS:
        if data.get(row.name) is not None:
            data[row.name] = _to_device(data[row.name], device)
    # seeded noise (model.noise_seed set): image i of the batch draws the noise of dataset index batch_indices[0] + i, whatever
    # samples_per_gpu is and whichever rank the batch landed on (a batch_sampler of a sequential or strided sampler hands out
    # increasing indices; the first one names the batch)
    inner = getattr(model, 'module', model)
    if getattr(inner, 'noise_seed', None) is not None and batch_indices:
        kwargs = dict(kwargs, image_base=int(batch_indices[0]))
    with torch.no_grad():
        return model(return_loss=False, **kwargs, **data)


def _post(dataset, result, batch_indices, pre_eval, format_only, format_args):
    if format_only:
        return dataset.format_results(result, indices=batch_indices, **(format_args or {}))
    if pre_eval:
        out = []
        for r, i in zip(result, batch_indices):          # per image: valid for samples_per_gpu > 1
            out.extend(dataset.pre_eval([r], indices=[i]))
        return out
    return result


def seg_gt_loader(dataset, index):
    """the default ``gt_loader`` of ``device_eval``: what ``CustomDataset.pre_eval`` (mmseg/datasets/custom.py:298-312) hands to
    ``intersect_and_union`` for image ``index``."""
    return dict(label=dataset.get_gt_seg_map_by_idx(index), num_classes=len(dataset.CLASSES), ignore_index=dataset.ignore_index,
                reduce_zero_label=dataset.reduce_zero_label)


def _post_device(dataset, result, batch_indices, gt_loader, confusion=None):
    """``device_eval``: ``result`` holds the device maps of ``model(on_device=True)``; the per-image entries of ``dataset.pre_eval``
    come from ``ddp_amd.evaluation`` - one small device-to-host copy per batch.  uint8 maps are class maps (seg), float32 maps
    are depth maps; depth needs a caller-given ``gt_loader`` -> dict(gt=, crop=, min_depth=, max_depth=).
    ``confusion``: a ``ddp_amd.confusion.ConfusionMatrix`` that also takes the batch's class maps and the labels loaded here
    (uploaded once, for both reductions); it copies nothing back."""
    from . import evaluation as ev
    if not result:
        return []
    if any(not torch.is_tensor(r) for r in result):
        raise TypeError('device_eval=True: the model did not return device tensors (does its test entry take on_device=True?)')
    if result[0].dtype == torch.uint8:
        gts = [(gt_loader or seg_gt_loader)(dataset, i) for i in batch_indices]
        out = [None] * len(result)
        groups = {}
        for j, g in enumerate(gts):          # one call per distinct (num_classes, ignore_index, reduce_zero_label): one, in practice
            groups.setdefault((int(g['num_classes']), int(g['ignore_index']), bool(g['reduce_zero_label'])), []).append(j)
        for (k, ign, rzl), js in groups.items():
            labels = [gts[j]['label'] for j in js]
            if confusion is not None:
                if (k, ign, rzl) != (confusion.num_classes, confusion.ignore_index, confusion.reduce_zero_label):
                    raise ValueError(f'confusion: the matrix was made for (num_classes, ignore_index, reduce_zero_label) = '
                                     f'{(confusion.num_classes, confusion.ignore_index, confusion.reduce_zero_label)}, the ground truth of '
                                     f'image {batch_indices[js[0]]} has {(k, ign, rzl)}')
                labels = [ev._as_u8(l, f'label {batch_indices[j]}').to(result[j].device, non_blocking=True) for j, l in zip(js, labels)]
                confusion.update([result[j] for j in js], labels)
            for j, t in zip(js, ev.seg_pre_eval([result[j] for j in js], labels, k, ign, rzl)):
                out[j] = t
        return out
    if confusion is not None:
        raise ValueError('confusion= takes class maps (uint8): the reference has no confusion matrix for depth maps')
    if gt_loader is None:
        raise ValueError('device_eval=True on depth maps needs gt_loader(dataset, index) -> dict(gt=, crop=, min_depth=, max_depth=): '
                         'the reference has no ground-truth accessor for depth datasets')
    gts = [gt_loader(dataset, i) for i in batch_indices]
    out = [None] * len(result)
    groups = {}
    for j, g in enumerate(gts):
        groups.setdefault((float(g['min_depth']), float(g['max_depth'])), []).append(j)
    for (lo, hi), js in groups.items():
        for j, t in zip(js, ev.depth_pre_eval([result[j] for j in js], [gts[j]['gt'] for j in js], lo, hi,
                                              crops=[gts[j].get('crop') for j in js])):
            out[j] = t
    return out


def _check_device_eval(device_eval, pre_eval, confusion=None):
    if device_eval and not pre_eval:
        raise ValueError('device_eval=True requires pre_eval=True (it replaces dataset.pre_eval; the other paths need the maps on the host)')
    if confusion is not None and not device_eval:
        raise ValueError('confusion= requires device_eval=True (the matrix is accumulated from the device maps of on_device=True)')


def single_gpu_test(model, data_loader, pre_eval=False, format_only=False, format_args=None, device_eval=False, gt_loader=None,
                    confusion=None):
    """test.py:34-137 without the drawing / deprecated ``efficient_test`` branches.  Returns the list of per-image
    results (or pre-eval tuples / formatted file names) in dataset order.
    ``device_eval=True`` (with ``pre_eval=True``): the model is called with ``on_device=True`` and the per-image pre-eval entries
    are reduced on the device (``ddp_amd.evaluation``); ``gt_loader(dataset, index)`` supplies the ground truth (default for
    seg datasets: ``seg_gt_loader``).  The entries equal ``dataset.pre_eval``'s, so ``dataset.evaluate`` is untouched.
    ``confusion`` (with ``device_eval=True``): a ``ddp_amd.confusion.ConfusionMatrix``; every batch's device maps and the labels
    ``gt_loader`` returned also go through ``confusion.update`` - no second load, nothing copied back; read ``confusion.result()``
    afterwards (``tools/confusion_matrix.py``'s matrix without the pickled predictions).  The return value is unchanged."""
    assert not (pre_eval and format_only), '``pre_eval`` and ``format_only`` are mutually exclusive'
    _check_device_eval(device_eval, pre_eval, confusion)
    model.eval()
    device = _model_device(model)
    dataset = data_loader.dataset
    results = []
    for batch_indices, data in zip(data_loader.batch_sampler, data_loader):
        if device_eval:
            results.extend(_post_device(dataset, _run_batch(model, data, device, batch_indices, on_device=True), batch_indices, gt_loader,
                                        confusion))
            continue
        result = _run_batch(model, data, device, batch_indices)
        results.extend(_post(dataset, result, batch_indices, pre_eval, format_only, format_args))
    return results


def multi_gpu_test(model, data_loader, tmpdir=None, gpu_collect=False, pre_eval=False, format_only=False,
                   format_args=None, device_eval=False, gt_loader=None):
    """test.py:140-229: every rank walks its DistributedSampler shard, then the per-rank lists are merged.
    ``device_eval`` / ``gt_loader``: see ``single_gpu_test``.  There is no ``confusion=`` here: a ``DistributedSampler`` repeats
    samples to pad its shards, ``collect_results`` cuts their entries off again, and an accumulator cannot un-count them."""
    assert not (pre_eval and format_only), '``pre_eval`` and ``format_only`` are mutually exclusive'
    _check_device_eval(device_eval, pre_eval)
    model.eval()
    device = _model_device(model)
    dataset = data_loader.dataset
    results = []
    for batch_indices, data in zip(data_loader.batch_sampler, data_loader):
        if device_eval:
            results.extend(_post_device(dataset, _run_batch(model, data, device, batch_indices, rescale=True, on_device=True),
                                        batch_indices, gt_loader))
            continue
        result = _run_batch(model, data, device, batch_indices, rescale=True)
        results.extend(_post(dataset, result, batch_indices, pre_eval, format_only, format_args))
    return collect_results(results, len(dataset), tmpdir=tmpdir, gpu_collect=gpu_collect)


def _interleave(parts, size):
    """rank r of a DistributedSampler(shuffle=False) owns samples r, r + world, ...: zip the per-rank lists back
    together and drop the samples the sampler repeated to even out the shards."""
    ordered = []
    for group in zip(*parts):
        ordered.extend(group)
    # ragged tails (a rank that ran fewer batches): append what zip() dropped, still rank-interleaved
    n = min(len(p) for p in parts) if parts else 0
    longest = max((len(p) for p in parts), default=0)
    for i in range(n, longest):
        for p in parts:
            if i < len(p):
                ordered.append(p[i])
    return ordered[:size]


def collect_results(results, size, tmpdir=None, gpu_collect=False):
    """``gpu_collect=True``: one ``all_gather_object`` over the process group (mmcv ``collect_results_gpu``);
    otherwise every rank pickles its list into ``tmpdir`` and rank 0 reads them back (``collect_results_cpu``)."""
    rank, world = _dist_info()
    if world == 1:
        return results[:size]
    if gpu_collect:
        parts = [None] * world
        dist.all_gather_object(parts, results)
        return _interleave(parts, size) if rank == 0 else None
    # shared-directory exchange: rank 0 chooses the directory and tells the others
    holder = [tmpdir]
    if tmpdir is None:
        if rank == 0:
            holder[0] = tempfile.mkdtemp(prefix='ddp_amd_collect_')
        dist.broadcast_object_list(holder, src=0)
    tmpdir = holder[0]
    os.makedirs(tmpdir, exist_ok=True)
    with open(os.path.join(tmpdir, f'part_{rank}.pkl'), 'wb') as f:
        pickle.dump(results, f)
    dist.barrier()
    if rank != 0:
        return None
    parts = []
    for r in range(world):
        with open(os.path.join(tmpdir, f'part_{r}.pkl'), 'rb') as f:
            parts.append(pickle.load(f))
    shutil.rmtree(tmpdir, ignore_errors=True)
    return _interleave(parts, size)
