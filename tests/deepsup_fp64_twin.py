"""fp64 statement of the deep-supervision loss term CE(upsample_s(z), label) in plain torch, for tests/test_deepsup_cpu.py
and tests/test_deepsup_gpu.py.  The interpolation is written out from its index formula, not taken from F.interpolate
(tests/test_deepsup_cpu.py compares the two); the gradient comes from autograd.

Per axis with coarse size n and integer scale s (bilinear, align_corners=False):
    src = max((dst + 0.5) / s - 0.5, 0),  i0 = floor(src),  i1 = min(i0 + 1, n - 1),  lambda = src - i0
    out[dst] = (1 - lambda) v[i0] + lambda v[i1]

``variant`` names a WRONG formulation, for the sensitivity controls (each must leave the bounds of tests/deepsup_bounds.py
somewhere, else the GPU test could pass vacuously):
    "align_corners"  src = dst (n - 1) / (n s - 1)
    "no_clamp"       i1 = i0 + 1 even past the last sample, where a zero is read
    "swap_lambda"    lambda v[i0] + (1 - lambda) v[i1]
    "scale_x2"       the formula with 2 s in the place of s
    "count_all"      the count taken over all pixels instead of the valid ones
"""
from __future__ import annotations

import torch

VARIANTS = ("align_corners", "no_clamp", "swap_lambda", "scale_x2", "count_all")


def taps(n: int, s: int, variant=None):
    """(i0, i1, lambda) of the n s destination indices of one axis: int64, int64, fp64"""
    dst = torch.arange(n * s, dtype=torch.float64)
    if variant == "align_corners":
        src = dst * ((n - 1) / (n * s - 1)) if n * s > 1 else torch.zeros_like(dst)
    else:
        sc = 2 * s if variant == "scale_x2" else s
        src = ((dst + 0.5) / sc - 0.5).clamp_min(0.0)
    i0 = src.floor().clamp_max(n - 1)
    lam = src - i0
    i0 = i0.long()
    i1 = i0 + 1 if variant == "no_clamp" else (i0 + 1).clamp_max(n - 1)
    return i0, i1, lam


def interp_matrix(n: int, s: int, variant=None) -> torch.Tensor:
    """U (n s, n) fp64 with U @ v = the interpolated vector.  "no_clamp" has n + 1 columns; the last one meets a zero."""
    i0, i1, lam = taps(n, s, variant)
    cols = n + 1 if variant == "no_clamp" else n
    w0, w1 = (lam, 1.0 - lam) if variant == "swap_lambda" else (1.0 - lam, lam)
    U = torch.zeros(n * s, cols, dtype=torch.float64)
    rows = torch.arange(n * s)
    U[rows, i0] += w0
    U[rows, i1] += w1
    return U


def upsample(z: torch.Tensor, s: int, variant=None) -> torch.Tensor:
    """bilinear x s of channels-last z (B, h, w, C) -> (B, h s, w s, C), in z's dtype (fp64 for the twin)"""
    B, h, w, C = z.shape
    Uh, Uw = interp_matrix(h, s, variant).to(z.dtype), interp_matrix(w, s, variant).to(z.dtype)
    if variant == "no_clamp":
        z = torch.nn.functional.pad(z, (0, 0, 0, 1, 0, 1))
    return torch.einsum("Yi,Xj,bijc->bYXc", Uh, Uw, z)


def adjoint(q: torch.Tensor, h: int, w: int, s: int) -> torch.Tensor:
    """sum over the fine pixels P of wgt(P -> (i, j)) q(P): (B, h s, w s, C) -> (B, h, w, C)"""
    Uh, Uw = interp_matrix(h, s).to(q.dtype), interp_matrix(w, s).to(q.dtype)
    return torch.einsum("Yi,Xj,bYXc->bijc", Uh, Uw, q)


def twin(z64: torch.Tensor, label: torch.Tensor, s: int, ignore_index: int, g=None, variant=None) -> dict:
    """z64 (B, h, w, nc) fp64 coarse logits, label (B, h s, w s) int64.  Returns the quantities the kernels produce and
    those the bounds are made of: zhat (B, H, W, nc), lse, valid, zy and row = lse - zy (zero where not valid), total =
    sum of row, count, loss = total / count, sm = softmax(zhat), oh = one-hot of the valid labels, and dl = g d(total)/dz
    with g = 1 / count when not given (the mean's gradient for an upstream of 1)."""
    nc = z64.shape[-1]
    z = z64.detach().clone().requires_grad_(True)
    zhat = upsample(z, s, variant)
    lse = torch.logsumexp(zhat, dim=-1)
    valid = (label != ignore_index) & (label >= 0) & (label < nc)
    safe = torch.where(valid, label, torch.zeros_like(label))
    zy = zhat.gather(-1, safe[..., None])[..., 0]
    row = torch.where(valid, lse - zy, torch.zeros_like(lse))
    total = row.sum()
    count = torch.tensor(float(label.numel()) if variant == "count_all" else float(valid.sum()), dtype=torch.float64)
    gg = (1.0 / count if count > 0 else torch.tensor(0.0, dtype=torch.float64)) if g is None else torch.as_tensor(g, dtype=torch.float64)
    (dz,) = torch.autograd.grad(total, z)
    oh = torch.nn.functional.one_hot(safe, nc).to(torch.float64) * valid[..., None]
    return dict(zhat=zhat.detach(), lse=lse.detach(), valid=valid, zy=zy.detach(), row=row.detach(), total=total.detach(),
                count=count, loss=(total / count).detach(), sm=torch.softmax(zhat.detach(), -1), oh=oh, g=gg, dl=dz * gg)
