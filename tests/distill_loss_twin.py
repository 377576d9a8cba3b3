"""The distillation loss (temperature KL against a teacher + cross entropy) in fp64, plain torch: the definition the kernels
of csrc/distill.hip, ``pointwise.DistillLossFn`` and ``DistillLoss2d`` are held to.  Forward by the formulas of
include/sigma_distill.h, gradient by autograd.  No GPU is needed.

Rows x64 and t64 (rows, classes) fp64 -- the student's and the teacher's logits -- and labels (rows,) int64.  A row is valid
when label != ignore and 0 <= label < classes; the KD set S is the valid rows, or every row with `kd_all`.  With
p = softmax(x / T), q = softmax(t / T), P1 = softmax(x):

    kl_r = sum_c [q_c > 0] q_c ((t_c / T - lse(t / T)) - (x_c / T - lse(x / T)))
    kd   = T^2 (1 / |S|) sum_{r in S} kl_r                     (0 when S is empty)
    ce   = (1 / n) sum_valid (lse(x) - x_y)                    (0 when n = 0)
    loss = kw kd + cw ce
    dloss / dx_rc = kw (T / |S|) (p_c - q_c) [r in S] + (cw / n) (P1_c - [c = y]) [r valid]

``VARIANTS`` names five plausible wrong implementations; ``twin(..., variant=name)`` computes them, so that a test can show
its bounds tell them from the right one:
    "no_t2"          the factor T^2 dropped from kd (and with it from the gradient)
    "reverse_kl"     KL(p || q) instead of KL(q || p)
    "teacher_t1"     the teacher's softmax taken at T = 1
    "ce_over_all"    the cross-entropy mean taken over all rows instead of the valid ones
    "grad_inv_t"     the right loss, the KD gradient scaled by 1 / T instead of T
"""
from __future__ import annotations

import torch

VARIANTS = ("no_t2", "reverse_kl", "teacher_t1", "ce_over_all", "grad_inv_t")


def is_valid(lab, nc, ignore):
    return (lab != ignore) & (lab >= 0) & (lab < nc)


def _select(cond, a):
    return torch.where(cond, a, torch.zeros_like(a))


def twin(x64, t64, lab, ignore, T=1.0, kw=1.0, cw=0.0, kd_all=False, upstream=1.0, variant=None):
    """dict of fp64 tensors: loss, kd, ce, lse (rows, 3) = lse(x), lse(x / T), lse(t / T); p, q, P1; lp = log p, lq = log q;
    oh = one-hot (zero rows where not valid), valid, in_s, n, ns = |S|, klr (rows; zero outside S), nll (rows; zero where not
    valid), c0 = kw T / |S|, c1 = cw / n, and dl = upstream * dloss/dx by autograd (by the formula for "grad_inv_t")."""
    assert x64.dtype == torch.float64 and t64.dtype == torch.float64 and variant in (None,) + VARIANTS
    rows, nc = x64.shape
    dev = x64.device
    x = x64.detach().clone().requires_grad_(True)
    valid = is_valid(lab, nc, ignore)
    in_s = torch.ones_like(valid) if kd_all else valid
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    oh = ((safe[:, None] == torch.arange(nc, device=dev)[None, :]) & valid[:, None]).double()
    lse1 = torch.logsumexp(x, dim=1)
    lp = torch.log_softmax(x / T, dim=1)
    lq = torch.log_softmax(t64 / (1.0 if variant == "teacher_t1" else T), dim=1)
    p, q = lp.exp(), lq.exp()
    if variant == "reverse_kl":
        klr = _select(p > 0, p * (lp - lq)).sum(1)
    else:
        klr = _select(q > 0, q * (lq - lp)).sum(1)           # a select: q = 0 contributes exactly 0
    klr = _select(in_s, klr)
    ns, n = in_s.double().sum(), valid.double().sum()
    kd = (1.0 if variant == "no_t2" else T * T) * klr.sum() / ns.clamp_min(1.0)
    xy = x.gather(1, safe[:, None])[:, 0]
    nll = _select(valid, lse1 - xy)
    ce = nll.sum() / (float(max(rows, 1)) if variant == "ce_over_all" else n.clamp_min(1.0))
    loss = kw * kd + cw * ce
    finite = bool(torch.isfinite(loss))
    with torch.no_grad():
        P1 = torch.softmax(x, dim=1)
        c0 = kw * T / ns if ns > 0 else torch.zeros((), dtype=torch.float64, device=dev)
        c1 = cw / n if n > 0 else torch.zeros((), dtype=torch.float64, device=dev)
        formula = lambda a: a * (p - q) * in_s.double()[:, None] + c1 * (P1 - oh) * valid.double()[:, None]
    if variant == "grad_inv_t":
        grad = formula(kw / (T * ns) if ns > 0 else c0)
    elif finite:
        (grad,) = torch.autograd.grad(loss, x)
    else:
        grad = formula(c0)                                   # a +inf loss (a -inf student logit where q > 0): the formula's gradient
    d = dict(loss=loss, kd=kd, ce=ce, lse=torch.stack([lse1, torch.logsumexp(x / T, dim=1), torch.logsumexp(t64 / T, dim=1)], 1),
             p=p, q=q, P1=P1, lp=lp, lq=lq, oh=oh, valid=valid, in_s=in_s, n=n, ns=ns, klr=klr, nll=nll, c0=c0, c1=c1,
             dl=upstream * grad)
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()}


def formula_gradient(t, upstream=1.0):
    """upstream * [ c0 (p - q) [r in S] + c1 (P1 - [c = y]) [r valid] ]: the gradient of the issue, from a twin's quantities
    (tests hold it against the twin's autograd gradient)"""
    return upstream * (t["c0"] * (t["p"] - t["q"]) * t["in_s"].double()[:, None]
                       + t["c1"] * (t["P1"] - t["oh"]) * t["valid"].double()[:, None])
