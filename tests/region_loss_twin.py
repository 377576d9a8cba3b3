"""The region-overlap loss (Dice, Jaccard, Tversky) in fp64, plain torch: the definition the kernels of csrc/region.hip,
``pointwise.RegionLossFn`` and ``RegionLoss2d`` are held to.  Forward by the formulas of include/sigma_region.h, gradient by
autograd.  No GPU is needed.

Rows x64 (rows, classes) fp64 and labels (rows,) int64.  A row is valid when label != ignore and 0 <= label < classes.  With
p = softmax(x) and sums over the valid rows:

    I_c = sum p_c [y = c]    P_c = sum p_c    Y_c = sum [y = c]    n = number of valid rows
    N_c = I_c + s            D_c = (1 - a - b) I_c + a P_c + b Y_c + s            T_c = N_c / D_c
    K = { c : Y_c > 0 }      region = (1 / |K|) sum_{c in K} (1 - T_c)            (0 when K is empty)
    loss = rw region + cw (1 / n) sum_valid (lse - x_y)                          (CE term 0 when n = 0)

``VARIANTS`` names four plausible wrong implementations; ``twin(..., variant=name)`` computes them, so that a test can show
its bounds tell them from the right one:
    "p_over_ignored"   P_c summed over the ignored rows too
    "mean_over_all"    the mean of 1 - T_c taken over all C classes instead of K
    "no_dot"           the term -p_c dot dropped from the gradient (the softmax Jacobian taken as diagonal)
    "smooth_num_only"  s added to the numerator only
"""
from __future__ import annotations

import torch

KINDS = {"dice": (0.5, 0.5), "jaccard": (1.0, 1.0)}
VARIANTS = ("p_over_ignored", "mean_over_all", "no_dot", "smooth_num_only")


def is_valid(lab, nc, ignore):
    return (lab != ignore) & (lab >= 0) & (lab < nc)


def twin(x64, lab, ignore, a, b, s=0.0, rw=1.0, cw=0.0, upstream=1.0, variant=None):
    """dict of fp64 tensors: loss, region, ce, sums (3, C) = I, P, Y, lse, sm = softmax, oh = one-hot (zero rows where not
    valid), valid, n, kcount, T, N, D, A = dloss/dI, B = dloss/dP (zero outside K), cwn = cw / n, g = B + A [c = y], dot, and
    dl = upstream * dloss/dx by autograd (by the formula without the dot term for the variant "no_dot")."""
    assert x64.dtype == torch.float64 and variant in (None,) + VARIANTS
    rows, nc = x64.shape
    x = x64.detach().clone().requires_grad_(True)
    valid = is_valid(lab, nc, ignore)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    oh = ((safe[:, None] == torch.arange(nc)[None, :]) & valid[:, None]).double()
    vf = valid.double()[:, None]
    lse = torch.logsumexp(x, dim=1)
    sm = torch.softmax(x, dim=1)
    I = (sm * oh).sum(0)
    P = sm.sum(0) if variant == "p_over_ignored" else (sm * vf).sum(0)
    Y = oh.sum(0)
    n = vf.sum()
    present = Y > 0
    kcount = present.sum()
    N = I + s
    D = (1.0 - a - b) * I + a * P + b * Y + (0.0 if variant == "smooth_num_only" else s)
    Ds = torch.where(present, D, torch.ones_like(D))
    T = torch.where(present, N / Ds, torch.zeros_like(D))
    miss = torch.where(present, 1.0 - T, torch.zeros_like(T))
    denom = float(nc) if variant == "mean_over_all" else kcount.clamp_min(1).double()
    region = miss.sum() / denom
    xy = x.gather(1, safe[:, None])[:, 0]
    ce = (torch.where(valid, lse - xy, torch.zeros_like(lse))).sum() / n.clamp_min(1.0)
    loss = rw * region + cw * ce
    (grad,) = torch.autograd.grad(loss, x)
    with torch.no_grad():
        f = rw / denom
        A = torch.where(present, -f * (D - (1.0 - a - b) * N) / (Ds * Ds), torch.zeros_like(D))
        B = torch.where(present, f * a * N / (Ds * Ds), torch.zeros_like(D))
        cwn = cw / n if n > 0 else torch.zeros(())
        g = (B[None, :] + oh * A[None, :]) * vf
        dot = (sm * g).sum(1)
        if variant == "no_dot":
            grad = (sm * g + cwn * (sm - oh)) * vf
        dl = upstream * grad
    d = dict(loss=loss, region=region, ce=ce, sums=torch.stack([I, P, Y]), lse=lse, sm=sm, oh=oh, valid=valid, n=n,
             kcount=kcount, T=T, N=N, D=D, A=A, B=B, cwn=cwn, g=g, dot=dot, dl=dl)
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()}


def formula_gradient(t, upstream=1.0):
    """upstream * [ p_c (g_c - dot) + cwn (p_c - [c = y]) ] on valid rows, zero elsewhere: the gradient of the issue, from a
    twin's quantities (tests hold it against the twin's autograd gradient)"""
    vf = t["valid"].double()[:, None]
    return upstream * (t["sm"] * (t["g"] - t["dot"][:, None]) + t["cwn"] * (t["sm"] - t["oh"])) * vf
