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

``FocalLoss2d`` under the same import name (utils/loss_opr.py:12-23): nn.NLLLoss(weight, reduction, ignore_index) of
(1 - softmax)^e * log_softmax, per pixel w_y (1 - p_y)^e (lse - x_y).  The reference's class stores ``gamma`` and never
reads it: its exponent is the literal 2.  Here ``exponent=None`` keeps that, a float ``exponent`` selects another one; on
the classifier's channels-last logits the loss runs on sigma_softmax_focal_fwd / _bwd (``pointwise.focal_cross_entropy``)
for e = 0 or e >= 1, anything else -- 0 < e < 1 included -- takes the torch formulation.

``RegionLoss2d`` is NOT one of the reference's criteria: a soft region-overlap loss (Dice, Jaccard, Tversky), optionally summed
with the mean cross entropy, for the same background-dominated datasets; on the classifier's channels-last logits it runs on
the kernels of csrc/region.hip (``pointwise.region_loss``, up to 64 classes), anything else takes its torch formulation.

``DistillLoss2d`` is not one of the reference's criteria either: the loss of a student against a frozen teacher's logits (KL
at a temperature, optionally summed with the mean cross entropy), ``forward(input, target, teacher_logits)``; on the
classifier's channels-last logits it runs on the kernels of csrc/distill.hip (``pointwise.distill_loss``, up to 64 classes),
anything else takes its torch formulation.  ``EncoderDecoder.attach_teacher`` is what calls it with three arguments.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class FocalLoss2d(nn.Module):
    """``FocalLoss2d(gamma=0, weight=None, reduction='mean', ignore_index=255)`` of the reference, plus ``exponent``.

    ``gamma`` is accepted and unused, as in the reference (whatever is passed, the reference raises 1 - softmax to the
    power 2).  ``exponent=None`` reproduces that; ``exponent=<float>`` is the focal exponent actually applied.  ``weight``
    (a list, an array or a tensor of per-class weights) is held as the reference holds it, as the fp32 weight of
    ``self.loss = nn.NLLLoss(...)``: the state-dict key is ``loss.weight`` and ``.to(device)`` moves it."""

    def __init__(self, gamma=0, weight=None, reduction='mean', ignore_index=255, exponent=None):
        super().__init__()
        self.gamma = gamma                      # accepted and unused, as in the reference
        self.exponent = 2.0 if exponent is None else float(exponent)
        if not self.exponent >= 0.0:
            raise ValueError(f"FocalLoss2d: exponent {exponent!r} is negative or NaN")
        if weight is not None and not torch.is_tensor(weight) and len(weight) == 0:
            weight = None                       # the reference's `if weight:` on an empty list
        if weight is not None:
            weight = weight.detach().cpu() if torch.is_tensor(weight) else torch.from_numpy(np.array(weight))
            weight = weight.float()
        self.loss = nn.NLLLoss(weight=weight, reduction=reduction, ignore_index=ignore_index)

    def forward(self, input, target):
        from ..pointwise import focal_cross_entropy, focal_deterministic
        target = target.long()
        crit = self.loss
        if input.is_cuda:
            loss = focal_cross_entropy(input, target, crit.ignore_index, self.exponent, weight=crit.weight, reduction=crit.reduction)
            if loss is not None:
                return loss
            if torch.are_deterministic_algorithms_enabled():
                return focal_deterministic(input, target, crit.ignore_index, self.exponent, weight=crit.weight, reduction=crit.reduction)
        return crit((1 - F.softmax(input, 1)) ** self.exponent * F.log_softmax(input, 1), target)


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


class RegionLoss2d(nn.Module):
    """A soft region-overlap loss, a criterion of the project's own (the reference has none): the overlap score the
    evaluator reports, made differentiable.  With p = softmax(input) and sums over the valid pixels of the batch (valid:
    target != ignore_index and inside [0, classes)):

        I_c = sum p_c [y = c]    P_c = sum p_c    Y_c = sum [y = c]
        T_c = (I_c + s) / ((1 - a - b) I_c + a P_c + b Y_c + s)              the Tversky index of class c
        region = mean over the classes with Y_c > 0 of 1 - T_c               (0 when nothing is labelled)
        loss = region_weight * region + ce_weight * mean cross entropy       (CE term 0 when nothing is labelled)

    ``kind``: "dice" (a = b = 0.5), "jaccard" (a = b = 1) or "tversky" (``alpha`` = a >= 0 weighs false positives, ``beta`` =
    b > 0 false negatives; both required, and rejected for the other two).  ``smooth`` = s >= 0.  On the channels-last
    logits of the classifier the loss runs on the kernels of csrc/region.hip (``pointwise.region_loss``, up to 64 classes)
    and ``last_terms`` then holds the device tensor (region, cross entropy) of that forward; anything else -- CPU tensors,
    other layouts, more classes -- takes ``torch_formulation``, element-wise ops and fixed-order sums only (one-hot by
    comparison), which is therefore also what runs under the deterministic flag.  Under DistributedDataParallel the sums
    are per rank: each rank's loss is the overlap on its own pixels."""

    def __init__(self, kind="dice", ignore_index=255, smooth=0.0, alpha=None, beta=None, ce_weight=0.0, region_weight=1.0):
        super().__init__()
        from ..pointwise import REGION_KINDS
        if kind == "tversky":
            if alpha is None or beta is None:
                raise ValueError("RegionLoss2d: kind 'tversky' needs alpha and beta")
            self.alpha, self.beta = float(alpha), float(beta)
            if not self.alpha >= 0.0:
                raise ValueError(f"RegionLoss2d: alpha {alpha!r} is negative or NaN")
            if not self.beta > 0.0:
                raise ValueError(f"RegionLoss2d: beta {beta!r} is not positive")
        elif kind in REGION_KINDS:
            if alpha is not None or beta is not None:
                raise ValueError(f"RegionLoss2d: kind {kind!r} fixes alpha and beta; pass them with kind='tversky'")
            self.alpha, self.beta = REGION_KINDS[kind]
        else:
            raise ValueError(f"RegionLoss2d: kind {kind!r} is not one of 'dice', 'jaccard', 'tversky'")
        self.kind = kind
        self.ignore_index = int(ignore_index)
        self.smooth, self.ce_weight, self.region_weight = float(smooth), float(ce_weight), float(region_weight)
        for name in ("smooth", "ce_weight", "region_weight"):
            if not getattr(self, name) >= 0.0:
                raise ValueError(f"RegionLoss2d: {name} {getattr(self, name)!r} is negative or NaN")
        self.last_terms = None

    def torch_formulation(self, input, target):
        nc = input.shape[1]
        lab = target.long()
        valid = ((lab != self.ignore_index) & (lab >= 0) & (lab < nc)).unsqueeze(1)
        hit = (lab.unsqueeze(1) == torch.arange(nc, device=input.device).view(1, nc, 1, 1)) & valid
        onehot, validf = hit.to(input.dtype), valid.to(input.dtype)
        lsm = F.log_softmax(input, dim=1)
        p = lsm.exp()
        I, P, Y = (p * onehot).sum(dim=(0, 2, 3)), (p * validf).sum(dim=(0, 2, 3)), onehot.sum(dim=(0, 2, 3))
        a, b, s = self.alpha, self.beta, self.smooth
        present = Y > 0
        D = torch.where(present, (1.0 - a - b) * I + a * P + b * Y + s, torch.ones_like(I))
        miss = torch.where(present, 1.0 - (I + s) / D, torch.zeros_like(I))
        region = miss.sum() / present.sum().clamp_min(1)
        nll = -torch.where(hit, lsm, torch.zeros_like(lsm)).sum()
        return self.region_weight * region + self.ce_weight * (nll / validf.sum().clamp_min(1.0))

    def forward(self, input, target):
        from ..pointwise import region_loss
        if input.is_cuda:
            out = region_loss(input, target, self.ignore_index, self.alpha, self.beta, self.smooth, self.region_weight,
                              self.ce_weight, with_terms=True)
            if out is not None:
                self.last_terms = out[1]
                return out[0]
        return self.torch_formulation(input, target)


class DistillLoss2d(nn.Module):
    """The distillation loss, a criterion of the project's own (the reference has none): the student's logits `input` held to
    a frozen teacher's `teacher_logits` of the same shape.  With T = temperature, p = softmax(input / T), q = softmax(teacher
    / T), valid pixels as everywhere (target != ignore_index and inside [0, classes)) and S = the valid pixels, or every
    pixel with ``kd_all``:

        kd   = T^2 * mean over S of sum_c [q_c > 0] q_c (log q_c - log p_c)     (0 when S is empty)
        ce   = mean over the valid pixels of the cross entropy of input          (0 when nothing is labelled)
        loss = kd_weight * kd + ce_weight * ce

    The teacher gets no gradient.  On the channels-last logits of the classifier (either pitch for either tensor) the loss
    runs on the kernels of csrc/distill.hip (``pointwise.distill_loss``, up to 64 classes) and ``last_terms`` then holds the
    device tensor (kd, ce) of that forward; anything else -- CPU tensors, other layouts, more classes -- takes
    ``torch_formulation``, element-wise ops and fixed-order sums only (one-hot by comparison), which is therefore also what
    runs under the deterministic flag."""

    def __init__(self, temperature=1.0, kd_weight=1.0, ce_weight=0.0, ignore_index=255, kd_all=False):
        super().__init__()
        self.temperature, self.kd_weight, self.ce_weight = float(temperature), float(kd_weight), float(ce_weight)
        if not (self.temperature > 0.0 and self.temperature != float("inf")):
            raise ValueError(f"DistillLoss2d: temperature {temperature!r} is not a positive number")
        for name in ("kd_weight", "ce_weight"):
            if not getattr(self, name) >= 0.0:
                raise ValueError(f"DistillLoss2d: {name} {getattr(self, name)!r} is negative or NaN")
        self.ignore_index = int(ignore_index)
        self.kd_all = bool(kd_all)
        self.last_terms = None

    def torch_formulation(self, input, target, teacher_logits):
        nc = input.shape[1]
        lab = target.long()
        valid = ((lab != self.ignore_index) & (lab >= 0) & (lab < nc)).unsqueeze(1)
        hit = (lab.unsqueeze(1) == torch.arange(nc, device=input.device).view(1, nc, 1, 1)) & valid
        T = self.temperature
        teacher = teacher_logits.detach().to(input.dtype)
        lp, lq = F.log_softmax(input / T, dim=1), F.log_softmax(teacher / T, dim=1)
        q = lq.exp()
        kl = torch.where(q > 0, q * (lq - lp), torch.zeros_like(q))
        if self.kd_all:
            kd = kl.sum() / max(kl.numel() // nc, 1)
        else:
            kd = torch.where(valid, kl, torch.zeros_like(kl)).sum() / valid.to(input.dtype).sum().clamp_min(1.0)
        lsm = F.log_softmax(input, dim=1)
        nll = -torch.where(hit, lsm, torch.zeros_like(lsm)).sum()
        ce = nll / valid.to(input.dtype).sum().clamp_min(1.0)
        return self.kd_weight * (T * T) * kd + self.ce_weight * ce

    def forward(self, input, target, teacher_logits):
        from ..pointwise import distill_loss
        if input.is_cuda:
            out = distill_loss(input, teacher_logits, target, self.ignore_index, self.temperature, self.kd_weight, self.ce_weight,
                               self.kd_all, with_terms=True)
            if out is not None:
                self.last_terms = out[1]
                return out[0]
        return self.torch_formulation(input, target, teacher_logits)
