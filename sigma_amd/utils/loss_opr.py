"""``ProbOhemCrossEntropy2d`` under the reference's import name (utils/loss_opr.py:137-187): cross entropy on the hard
pixels only.  The reference's class inverts boolean masks with ``1 - mask``, which current torch refuses; this one is
written for the project: on the channels-last logits of the classifier GEMM the pixels are selected by the radix-select
kernels of csrc/ohem.hip and the loss runs on the cross-entropy kernels (``pointwise.ohem_cross_entropy``); anything
else takes the torch formulation below.

Rules (N pixels in the batch; valid = label != ignore_label, and inside [0, classes); p = softmax(pred)[label] at valid
pixels, 1 elsewhere):
  1. min_kept > num_valid, num_valid == 0 or min_kept <= 0: every valid pixel is kept (thresh is not applied).
  2. otherwise q = the min(N, min_kept)-th smallest p, threshold = max(thresh, q), and a valid pixel is kept iff
     p <= threshold: ties at the threshold are all kept.
  3. the result is nn.CrossEntropyLoss(weight, reduction, ignore_index) on the labels with every other pixel set to
     ignore_label; the selection carries no gradient.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


class ProbOhemCrossEntropy2d(nn.Module):
    def __init__(self, ignore_label, reduction='mean', thresh=0.6, min_kept=256, down_ratio=1, use_weight=False, weight=None):
        super().__init__()
        if use_weight:
            raise NotImplementedError("use_weight=True selects the reference's 19-class Cityscapes table, which fits none of "
                                      "Sigma's datasets: pass the class weights of yours as weight=<1-D tensor>")
        self.ignore_label = int(ignore_label)
        self.reduction = reduction
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.down_ratio = down_ratio            # accepted and unused, as in the reference
        self.criterion = nn.CrossEntropyLoss(weight=weight, reduction=reduction, ignore_index=self.ignore_label)

    def mined_labels(self, pred, target):
        """`target` with every pixel the rules drop set to ignore_label (torch formulation; reads the data-dependent
        branch on the host)"""
        with torch.no_grad():
            nc = pred.shape[1]
            valid = (target != self.ignore_label) & (target >= 0) & (target < nc)
            num_valid = int(valid.sum())
            keep = valid
            if 0 < self.min_kept <= num_valid:
                safe = torch.where(valid, target, torch.zeros_like(target))
                p = F.softmax(pred, dim=1).gather(1, safe.unsqueeze(1)).squeeze(1)
                p = torch.where(valid, p, torch.ones_like(p))
                ordered = torch.sort(p.reshape(-1)).values          # not kthvalue: refused on the GPU in deterministic mode
                q = ordered[min(ordered.numel(), self.min_kept) - 1]
                threshold = torch.clamp(q, min=self.thresh)
                keep = valid & (p <= threshold)
            return torch.where(keep, target, torch.full_like(target, self.ignore_label))

    def forward(self, pred, target):
        from ..pointwise import cross_entropy_deterministic, ohem_cross_entropy
        target = target.long()
        w = self.criterion.weight
        loss = ohem_cross_entropy(pred, target, self.ignore_label, self.thresh, self.min_kept, weight=w,
                                  reduction=self.reduction) if pred.is_cuda else None
        if loss is not None:
            return loss
        mined = self.mined_labels(pred, target)
        if torch.are_deterministic_algorithms_enabled():
            loss = cross_entropy_deterministic(self.criterion, pred, mined)
            if loss is not None:
                return loss
        return self.criterion(pred, mined)
