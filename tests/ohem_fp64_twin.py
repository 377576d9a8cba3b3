"""fp64 restatement of ProbOhemCrossEntropy2d (reference utils/loss_opr.py:137-187) in plain torch, in the p domain as the
reference does it -- the anchor of tests/test_ohem_cpu.py (against the reference's own output, tests/golden/loss_ohem.npz)
and the reference of tests/test_ohem_gpu.py.

N pixels, valid = label != ignore (and inside [0, classes)), p = softmax(x)[label] at valid pixels and 1 elsewhere:
  1. min_kept > num_valid, num_valid == 0 or min_kept <= 0: every valid pixel is kept;
  2. else q = the min(N, min_kept)-th smallest p, threshold = max(thresh, q), kept = valid and p <= threshold;
  3. nn.CrossEntropyLoss(weight, reduction, ignore_index) on the kept pixels; the selection carries no gradient.

``twin`` also returns what the kernels' domain needs: nll = lse - x_y, tau = -log(threshold) (-inf without mining) and
|nll - tau| per row.  ``variant`` builds the WRONG restatements of the negative controls:
  "exact_k"    the min_kept pixels of smallest p are kept (the first in pixel order among equals), thresh is ignored
  "strict"     p < threshold in place of p <= threshold
  "den_valid"  'mean' divides by the number of valid pixels in place of the summed weights of the kept ones
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

VARIANTS = ("exact_k", "strict", "den_valid")


def twin(x, lab, ignore, thresh, min_kept, weight=None, reduction="mean", upstream=1.0, variant=None):
    """x (rows, classes), lab (rows,) int64; upstream: the gradient of the result (a float, or (rows,) for 'none').
    Returns a dict: loss ((rows,) for 'none'), dl (rows, classes), keep, valid, mined, mining (bool), threshold (p domain,
    None without mining), tau, nll, lse, xy, p, dist = |nll - tau| (inf without mining), wy, den, tau_row (the index of
    a row whose p equals the threshold when the k-th value governs, else -1)."""
    assert variant in (None,) + VARIANTS
    x = x.double()
    rows, nc = x.shape
    valid = (lab != ignore) & (lab >= 0) & (lab < nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, safe[:, None])[:, 0]
    sm = torch.softmax(x, 1)
    p = torch.where(valid, sm.gather(1, safe[:, None])[:, 0], torch.ones_like(lse))
    nll = torch.where(valid, lse - xy, torch.zeros_like(lse))
    num_valid = int(valid.sum())
    mining = 0 < min_kept <= num_valid
    keep, threshold, tau_row = valid, None, -1
    if mining:
        k = min(rows, int(min_kept))
        order = torch.sort(p, stable=True)
        q = float(order.values[k - 1])
        if variant == "exact_k":
            keep = torch.zeros_like(valid)
            keep[order.indices[:k]] = True
            keep &= valid
            threshold = q
        else:
            threshold = max(float(thresh), q)
            keep = valid & ((p < threshold) if variant == "strict" else (p <= threshold))
        if q >= float(thresh):
            tau_row = int(order.indices[k - 1])
    w64 = weight.double().to(x.device) if weight is not None else torch.ones(nc, dtype=torch.float64, device=x.device)
    wy = torch.where(keep, w64[safe], torch.zeros_like(lse))
    row = wy * nll
    den = float(valid.sum()) if variant == "den_valid" else float(wy.sum())
    up = upstream.double().to(x.device) if torch.is_tensor(upstream) else torch.full((rows,), float(upstream), dtype=torch.float64, device=x.device)
    if reduction == "none":
        loss, gr = row, up
    elif reduction == "sum":
        loss, gr = row.sum(), up
    else:
        loss = row.sum() / den if den != 0 else row.sum() * float("nan")
        gr = up / den if den != 0 else torch.zeros_like(up)
    oh = F.one_hot(safe, nc).double()
    dl = (gr * wy)[:, None] * (sm - oh)
    if mining:
        import math
        tau = -math.log(threshold)
        dist = (nll - tau).abs()
    else:
        tau, dist = float("-inf"), torch.full_like(nll, float("inf"))
    mined = torch.where(keep, lab, torch.full_like(lab, ignore))
    return dict(loss=loss, dl=dl, keep=keep, valid=valid, mined=mined, mining=mining, threshold=threshold, tau=tau, nll=nll, lse=lse,
                xy=xy, p=p, dist=dist, wy=wy, den=den, tau_row=tau_row, sm=sm, oh=oh, gr=gr)
