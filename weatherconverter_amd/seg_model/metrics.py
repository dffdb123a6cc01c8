"""Streaming segmentation metrics (reference ``seg_model/metrics/stream_metrics.py``) with the confusion
matrix kept on the GPU.

The reference scores a batch with ``argmax -> .cpu().numpy() -> np.bincount``: a host sync, a D2H copy of the
prediction and a second pass over it per batch.  Here ``update`` is one ``wc_seg_confusion`` launch (the
argmax fused, logits read once) that adds into an int64 device matrix; nothing synchronises until
``confusion_matrix`` is read.  ``get_results`` runs the reference's formulas on the host from those counts
and equals the reference bit for bit for equal counts.
"""
from typing import Optional

import numpy as np
import torch

from .. import kernels as K


class StreamSegMetrics:
    """Stream Metrics for Semantic Segmentation Task: the reference's interface (``update``, ``get_results``,
    ``to_str``, ``reset``, ``confusion_matrix``)."""

    def __init__(self, n_classes: int, device=None):
        K._req(2 <= n_classes <= K.SEG_MAX_CLASSES, f'StreamSegMetrics: n_classes in 2..{K.SEG_MAX_CLASSES}')
        self.n_classes = int(n_classes)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.hist = torch.zeros((self.n_classes, self.n_classes), dtype=torch.int64, device=self.device)

    def _labels(self, t) -> torch.Tensor:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t))
        t = t.to(self.device, torch.int64, non_blocking=True)
        return (t.unsqueeze(0) if t.dim() == 2 else t).contiguous()

    def update(self, label_trues, label_preds, pred_out: Optional[torch.Tensor] = None):
        """Add one batch.  label_trues: (B, H, W) labels (any integer dtype, numpy or tensor).  label_preds:
        device fp32 logits (B, C, H, W) -- the fused argmax + histogram, ``pred_out`` (uint8 (B, H, W))
        receives the argmax when given -- or an integer prediction map (B, H, W), numpy or tensor (numpy
        inputs are uploaded; a host prediction outside [0, C) raises, a device one is ignored like a bad
        label).  No call synchronises the host with the device."""
        lt = self._labels(label_trues)
        if isinstance(label_preds, torch.Tensor) and label_preds.is_floating_point():
            K._req(label_preds.dim() == 4, 'StreamSegMetrics.update: logits are (B, C, H, W)')
            lp = label_preds.detach().to(self.device, torch.float32).contiguous()
            K.seg_confusion(lp, lt, self.hist, pred_out)
            return
        K._req(pred_out is None, 'StreamSegMetrics.update: pred_out goes with logits only')
        lp = label_preds
        if isinstance(lp, np.ndarray):
            lp = torch.from_numpy(np.ascontiguousarray(lp))
        if not lp.is_cuda and lp.numel():
            lo, hi = int(lp.min()), int(lp.max())
            if lo < 0 or hi >= self.n_classes:
                raise ValueError(f'StreamSegMetrics.update: predictions in [{lo}, {hi}] outside [0, {self.n_classes})')
        lp = lp.to(self.device, non_blocking=True)
        if lp.dtype != torch.uint8:
            # a device value outside [0, 255] must stay outside [0, C) after the narrowing
            lp = torch.where((lp >= 0) & (lp < 255), lp, torch.full_like(lp, 255)).to(torch.uint8)
        lp = (lp.unsqueeze(0) if lp.dim() == 2 else lp).contiguous()
        K.seg_confusion(lp, lt, self.hist)

    @property
    def confusion_matrix(self) -> np.ndarray:
        """float64 (C, C) numpy array, the reference's type: rows are true classes.  Reading it is the one
        host synchronisation."""
        return self.hist.cpu().numpy().astype(np.float64)

    @staticmethod
    def to_str(results) -> str:
        """One ``name: value`` line per scalar metric (the per-class IoU is left out), after a leading newline."""
        return '\n' + ''.join('%s: %f\n' % (k, v) for k, v in results.items() if k != 'Class IoU')

    @staticmethod
    def results_from(hist: np.ndarray) -> dict:
        """The five metrics of a (C, C) count matrix, rows = true classes, in float64 with the reference's
        order of operations: overall accuracy tp.sum() / total, mean accuracy nanmean(tp / row sums), IoU
        tp / (row + column - tp) with nanmean over it (a class absent from labels and predictions is NaN and
        leaves the means), and the frequency-weighted IoU over the classes that occur."""
        hist = np.asarray(hist, dtype=np.float64)
        tp, rows, columns, total = np.diag(hist), hist.sum(axis=1), hist.sum(axis=0), hist.sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            overall = tp.sum() / total
            mean_acc = np.nanmean(tp / rows)
            iou = tp / (rows + columns - tp)
            mean_iou = np.nanmean(iou)
            freq = rows / total
            present = freq > 0
            freq_weighted = (freq[present] * iou[present]).sum()
        return {'Overall Acc': overall, 'Mean Acc': mean_acc, 'FreqW Acc': freq_weighted, 'Mean IoU': mean_iou,
                'Class IoU': {c: iou[c] for c in range(hist.shape[0])}}

    def get_results(self) -> dict:
        """Overall Acc, Mean Acc, FreqW Acc, Mean IoU (float64) and Class IoU, from the counts so far."""
        return self.results_from(self.confusion_matrix)

    def reset(self):
        self.hist.zero_()


class AverageMeter:
    """Running means by key (the reference's ``AverageMeter`` interface): ``update(id, val)`` adds a value,
    ``get_results(id)`` is the mean of what was added since the key's last ``reset``."""

    def __init__(self):
        self.book = {}  # id -> [sum, count]

    def reset_all(self):
        self.book.clear()

    def reset(self, id):
        if id in self.book:
            self.book[id] = [0, 0]

    def update(self, id, val):
        if id in self.book:
            total, count = self.book[id]
            self.book[id] = [total + val, count + 1]
        else:
            self.book[id] = [val, 1]

    def get_results(self, id):
        total, count = self.book[id]
        return total / count
