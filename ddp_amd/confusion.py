"""The K x K confusion matrix of the reference's ``segmentation/tools/confusion_matrix.py:46-68`` (``calculate_confusion_matrix``),
accumulated on the device by libddp_cm.so (include/ddp_cm_mi355x.h).  The tool takes every full-size class map to the host and
reduces it with ``np.bincount(n * gt + res, minlength=n ** 2)``; here the maps stay where the epilogue wrote them, one (K, K)
accumulator of 64-bit counters lives on the device for the whole dataset, and the only device-to-host copy is the one
``ConfusionMatrix.result()`` makes at the end.

  ``seg_confusion``      the raw call: <= 64 device uint8 maps in, an int64 (K, K) device tensor out, nothing synchronises (what a
                         hipGraph captures)
  ``ConfusionMatrix``    the dataset-level accumulator: ``update`` per batch, ``result`` / ``normalized`` / ``pre_eval_totals`` at
                         the end; ``apis.single_gpu_test(..., device_eval=True, confusion=cm)`` feeds it

There is no CPU fallback.
"""
import numpy as np
import torch

from . import _cm_lib as M
from .evaluation import _as_u8, _device_of, _squeeze_map, _stream


def seg_confusion(preds, labels, num_classes, ignore_index=255, reduce_zero_label=False, accumulate=False, out=None, tally=None):
    """One ``ddp_cm_seg`` call: ``preds`` / ``labels`` are <= 64 contiguous device uint8 (H, W) maps.  -> ``out``, an int64
    (K, K) device tensor, rows the (mapped) ground truth and columns the prediction, the sum over all the maps (allocated when
    None; zeroed by the call unless ``accumulate``, which adds to what ``out`` holds).  ``tally``: None or an int64 (4,) device
    tensor of [pixels seen, ignored, label >= K, prediction >= K], treated like ``out``.  Enqueued on the current stream."""
    n = len(preds)
    K = int(num_classes)
    dev = preds[0].device if n else _device_of(())
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)((K, K), dtype=torch.int64, device=dev)
    items = (M.Item * max(n, 1))()
    for i, (p, l) in enumerate(zip(preds, labels)):
        items[i] = M.Item(p.data_ptr(), l.data_ptr(), p.shape[0], p.shape[1])
    lib = M.load()
    M.check(lib.ddp_cm_seg(items, n, K, int(ignore_index), int(bool(reduce_zero_label)), int(bool(accumulate)), out.data_ptr(),
                           None if tally is None else tally.data_ptr(), None, _stream(dev)), lib)
    return out


def normalize(matrix):
    """the tool's normalisation (confusion_matrix.py:89-91): per ground-truth row, in percent; a row without pixels is NaN"""
    matrix = np.asarray(matrix)
    per_label_sums = matrix.sum(axis=1)[:, np.newaxis]
    with np.errstate(invalid='ignore', divide='ignore'):
        return matrix.astype(np.float32) / per_label_sums * 100


def totals_from_matrix(matrix):
    """-> (total_area_intersect, total_area_union, total_area_pred_label, total_area_label), float64 (K,) arrays: the diagonal,
    the column sums and the row sums of the matrix"""
    matrix = np.asarray(matrix, dtype=np.float64)
    intersect, pred, label = np.diag(matrix).copy(), matrix.sum(axis=0), matrix.sum(axis=1)
    return intersect, pred + label - intersect, pred, label


class ConfusionMatrix:
    """Dataset-level accumulator.  ``update`` enqueues and returns; nothing is copied back until ``result`` / ``tally``."""

    def __init__(self, num_classes, ignore_index=255, reduce_zero_label=False, device=None):
        self.num_classes = int(num_classes)
        if not 2 <= self.num_classes <= 256:
            raise ValueError(f'num_classes {num_classes} out of range [2,256]')
        self.ignore_index = int(ignore_index)
        self.reduce_zero_label = bool(reduce_zero_label)
        self.device = None if device is None else torch.device(device)
        self._matrix = None      # int64 (K, K) and (4,) on the device, allocated by the first update
        self._tally = None

    def _buffers(self, dev):
        if self._matrix is None:
            self.device = dev
            self._matrix = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=dev)
            self._tally = torch.zeros(M.TALLY, dtype=torch.int64, device=dev)
        elif dev != self._matrix.device:
            raise ValueError(f'the accumulator lives on {self._matrix.device}, the maps on {dev}')
        return self._matrix, self._tally

    def update(self, preds, labels):
        """``preds``: device uint8 (H, W) class maps (``simple_test(on_device=True)``); ``labels``: the ground truth maps, device /
        CPU tensors or ndarrays (uploaded) - what ``evaluation.seg_pre_eval`` accepts.  Calls of more than 64 images run in
        chunks.  Nothing is copied back and nothing synchronises."""
        if len(preds) != len(labels):
            raise ValueError(f'{len(preds)} predictions for {len(labels)} label maps')
        if not len(preds):
            return self
        P = [_squeeze_map(_as_u8(p, f'pred {i}'), f'pred {i}') for i, p in enumerate(preds)]
        L = [_squeeze_map(_as_u8(l, f'label {i}'), f'label {i}') for i, l in enumerate(labels)]
        for i, (p, l) in enumerate(zip(P, L)):
            if p.shape != l.shape:
                raise ValueError(f'image {i}: prediction {tuple(p.shape)} and label {tuple(l.shape)} differ in shape')
        dev = _device_of(P + L, self.device)
        P = [p.to(dev, non_blocking=True).contiguous() for p in P]
        L = [l.to(dev, non_blocking=True).contiguous() for l in L]
        matrix, tally = self._buffers(dev)
        for a in range(0, len(P), M.MAX_ITEMS):
            seg_confusion(P[a:a + M.MAX_ITEMS], L[a:a + M.MAX_ITEMS], self.num_classes, self.ignore_index, self.reduce_zero_label,
                          accumulate=True, out=matrix, tally=tally)
        return self

    def reset(self):
        if self._matrix is not None:
            self._matrix.zero_()
            self._tally.zero_()

    def result(self):
        """the one device-to-host copy -> np.float64 (K, K), the dtype of the tool's ``np.zeros(shape=[n, n])`` accumulator"""
        if self._matrix is None:
            return np.zeros((self.num_classes, self.num_classes), dtype=np.float64)
        return self._matrix.cpu().numpy().astype(np.float64)

    def tally(self):
        """-> np.int64 (4,): pixels seen, ignored, dropped for a label >= K, dropped for a prediction >= K;
        tally[0] == tally[1] + tally[2] + tally[3] + result().sum()"""
        if self._tally is None:
            return np.zeros(M.TALLY, dtype=np.int64)
        return self._tally.cpu().numpy()

    def normalized(self, matrix=None):
        """the tool's ``astype(float32) / row sums * 100`` (what ``plot_confusion_matrix`` draws), NaN rows included"""
        return normalize(self.result() if matrix is None else matrix)

    def pre_eval_totals(self, matrix=None):
        """-> (intersect, union, pred, label) per class, from the diagonal, the column sums and the row sums.  They equal the
        sums of the per-image ``pre_eval`` entries only when ``tally()[2] == tally()[3] == 0``: ``intersect_and_union`` still
        counts the prediction of a pixel whose label is >= K, and the label of a pixel whose prediction is >= K; the matrix
        has no bin for either."""
        return totals_from_matrix(self.result() if matrix is None else matrix)
