"""fp64 restatement of FocalLoss2d (reference utils/loss_opr.py:12-23) with a free exponent, in plain torch: the anchor of
tests/test_focal_cpu.py (against the reference's own output, tests/golden/loss_focal.npz) and the reference of
tests/test_focal_gpu.py.  The formulas of include/sigma_ops.h (sigma_softmax_focal_fwd / _bwd):

  valid     label != ignore and 0 <= label < classes
  p = softmax(x), y the label, q = 1 - p_y, nll = lse - x_y, w the class weights (ones without)
  row_loss  = w_y q^gamma nll                                   (0 at rows that are not valid)
  den       = sum of w_y over the valid rows
  'none' = row_loss, 'sum' = sum of row_loss, 'mean' = sum of row_loss / den (NaN for den = 0: 0 / 0)
  dlogit_c  = g_r w_y m (p_c - [c == y]),   m = q^gamma + gamma q^(gamma - 1) p_y nll      (gamma = 0: m = 1)
  g_r       = upstream ('sum'; per row for 'none'), upstream / den ('mean'; zero for den = 0)

q is formed as -expm1(-nll), so that a row whose label has nearly all the probability keeps its relative precision.
``variant`` builds the WRONG restatements of the negative controls:
  "detached"   the gradient with the modulating factor held constant: m = q^gamma
  "square"     the reference's fixed exponent 2 whatever gamma is
  "den_count"  'mean' divides by the number of valid pixels in place of the summed weights
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

VARIANTS = ("detached", "square", "den_count")


def twin(x, lab, ignore, gamma, weight=None, reduction="mean", upstream=1.0, variant=None):
    """x (rows, classes), lab (rows,) int64; upstream: the gradient of the result (a float, or (rows,) for 'none').
    Returns a dict: loss ((rows,) for 'none'), dl (rows, classes), row, valid, lse, xy, nll, py, q, qg = q^gamma, m, wy,
    den, gr (the per-row g_r), sm (softmax) and oh (one-hot of the label)."""
    assert variant in (None,) + VARIANTS
    x = x.double()
    rows, nc = x.shape
    gamma = 2.0 if variant == "square" else float(gamma)
    valid = (lab != ignore) & (lab >= 0) & (lab < nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(x, 1)
    xy = x.gather(1, safe[:, None])[:, 0]
    sm = torch.softmax(x, 1)
    nll = torch.where(valid, lse - xy, torch.zeros_like(lse)).clamp_min(0.0)
    py = torch.exp(-nll)
    q = -torch.expm1(-nll)
    if gamma == 0.0:
        qg, m = torch.ones_like(q), torch.ones_like(q)
    else:
        t = q ** (gamma - 1.0)                                  # gamma >= 1 in every use: bounded
        qg = t * q
        m = qg if variant == "detached" else qg + gamma * t * py * nll
    w64 = weight.double().to(x.device) if weight is not None else torch.ones(nc, dtype=torch.float64, device=x.device)
    wy = torch.where(valid, w64[safe], torch.zeros_like(lse))
    row = wy * qg * nll
    den = float(valid.sum()) if variant == "den_count" else float(wy.sum())
    up = upstream.double().to(x.device) if torch.is_tensor(upstream) else torch.full((rows,), float(upstream), dtype=torch.float64, device=x.device)
    if reduction == "none":
        loss, gr = row, up
    elif reduction == "sum":
        loss, gr = row.sum(), up
    else:
        loss = row.sum() / den if den != 0 else row.sum() * float("nan")
        gr = up / den if den != 0 else torch.zeros_like(up)
    oh = F.one_hot(safe, nc).double()
    dl = (gr * wy * m)[:, None] * (sm - oh)
    return dict(loss=loss, dl=dl, row=row, valid=valid, lse=lse, xy=xy, nll=nll, py=py, q=q, qg=qg, m=m, wy=wy, den=den, gr=gr,
                sm=sm, oh=oh)
