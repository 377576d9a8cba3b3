"""fp64 statement of the deep-supervision loss term criterion(upsample_s(z), label) for the criteria with options, in plain
torch, for tests/test_deepsup_loss_cpu.py and tests/test_deepsup_loss_gpu.py.  The interpolation is
that of tests/deepsup_fp64_twin.py (``upsample`` below: its matrices, written out from the index formula); on its rows
    "options"  nn.CrossEntropyLoss(weight, label_smoothing) in fp64, per pixel,
    "focal"    tests/focal_fp64_twin.twin,
    "ohem"     tests/ohem_fp64_twin.twin for the kept set, then nn.CrossEntropyLoss(weight) on the mined labels;
the reduction is written out ('mean' divides by the summed w_y of the labelled / kept pixels) and the gradient with respect
to the COARSE logits comes from autograd.  Labels outside [0, classes) count as ignored.

``variant`` names a WRONG formulation, for the sensitivity controls (each must leave the bounds of
tests/deepsup_loss_bounds.py somewhere, else the GPU test could pass vacuously):
    "wy_wrong_class"      w_y taken at class y + 1 (mod C)                                   (options, focal, ohem; needs weights)
    "smooth_no_W"         the smoothing term (eps / C) (lse - sum_c w_c z_c), W left out      (options with eps > 0)
    "focal_m_one_term"    the modulating factor held constant in the gradient: m = q^gamma   (focal, gamma > 0)
    "mean_pixels"         'mean' divided by the number of labelled pixels, not by sum of w_y  ('mean' with weights)
    "ohem_thresh_always"  thresh applied although min_kept > num_valid                        (ohem)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from tests import focal_fp64_twin, ohem_fp64_twin
from tests.deepsup_fp64_twin import interp_matrix

VARIANTS = ("wy_wrong_class", "smooth_no_W", "focal_m_one_term", "mean_pixels", "ohem_thresh_always")


def upsample(z, s):
    """tests/deepsup_fp64_twin.upsample -- the same two matrices of the same index formula -- applied one axis after the
    other.  That module contracts both in one einsum, which at 4 x 120 x 160 forms the outer product of the two matrices
    (seconds forward, a quarter of a minute in the adjoint); tests/test_deepsup_loss_cpu.py holds the two to 1e-12."""
    B, h, w, C = z.shape
    Uh, Uw = interp_matrix(h, s).to(z.dtype), interp_matrix(w, s).to(z.dtype)
    return torch.einsum("Xj,bYjc->bYXc", Uw, torch.einsum("Yi,bijc->bYjc", Uh, z))


def adjoint(q, h, w, s):
    """tests/deepsup_fp64_twin.adjoint, one axis after the other: (B, h s, w s, C) -> (B, h, w, C)"""
    Uh, Uw = interp_matrix(h, s).to(q.dtype), interp_matrix(w, s).to(q.dtype)
    return torch.einsum("Yi,bYjc->bijc", Uh, torch.einsum("Xj,bYXc->bYjc", Uw, q))


def twin(z64, label, s, ignore, kind, weight=None, eps=0.0, gamma=0.0, thresh=0.7, min_kept=0, reduction="mean", upstream=1.0,
         variant=None):
    """z64 (B, h, w, nc) fp64 coarse logits, label (B, h s, w s) int64, weight (nc,) or None; upstream: the gradient of the
    result, a float or (B, h s, w s) for 'none'.  Returns zhat (B, H, W, nc), lse, valid, row (the per-pixel loss, zero where
    not valid / not kept), wy (w_y at the pixels that count, else 0), den = sum of wy, loss ('none': (B, H, W)), gP (the
    upstream of every fine pixel: upstream / den for 'mean') and dl = d(upstream . loss) / dz (B, h, w, nc); for "ohem" also
    keep, mined, counts = (num_valid, kept) and the dict `sel` of tests/ohem_fp64_twin.twin."""
    assert kind in ("options", "focal", "ohem") and variant in (None,) + VARIANTS
    nc = z64.shape[-1]
    z = z64.detach().clone().requires_grad_(True)
    zhat = upsample(z, s)
    rows = zhat.reshape(-1, nc)
    lab = label.reshape(-1)
    valid = (lab != ignore) & (lab >= 0) & (lab < nc)
    clean = torch.where(valid, lab, torch.full_like(lab, ignore))
    w64 = weight.double() if weight is not None else None
    if variant == "wy_wrong_class" and w64 is not None:
        w_used = w64.roll(-1)                                     # w_used[y] = w[y + 1]
    else:
        w_used = w64
    out = {}
    if kind == "focal":
        t = focal_fp64_twin.twin(rows, lab, ignore, gamma, weight=w_used, reduction="none")
        row, wy = t["row"], t["wy"]
        if variant == "focal_m_one_term":
            row = wy * t["qg"].detach() * t["nll"]
    else:
        counted = valid
        if kind == "ohem":
            sel = ohem_fp64_twin.twin(rows.detach(), lab, ignore, thresh, min_kept, weight=w64)
            keep = sel["keep"]
            if variant == "ohem_thresh_always" and not sel["mining"]:
                keep = valid & (sel["p"] <= float(thresh))
            clean = torch.where(keep, lab, torch.full_like(lab, ignore))
            counted = keep
            out.update(keep=keep.view(label.shape), mined=clean.view(label.shape), sel=sel,
                       counts=(int(valid.sum()), int(keep.sum())))
        crit = nn.CrossEntropyLoss(weight=w_used, ignore_index=ignore, reduction="none", label_smoothing=float(eps) if kind == "options" else 0.0)
        row = crit(rows, clean)
        wv = w_used if w_used is not None else torch.ones(nc, dtype=torch.float64)
        wy = torch.where(counted, wv[torch.where(counted, lab, torch.zeros_like(lab))], torch.zeros(lab.shape, dtype=torch.float64))
        if variant == "smooth_no_W" and eps > 0:
            W = wv.sum()
            row = row - torch.where(counted, (eps / nc) * (W - 1.0) * torch.logsumexp(rows, 1), torch.zeros_like(row))
    den = float(valid.sum()) if variant == "mean_pixels" and kind != "ohem" else \
        float(out["counts"][1]) if variant == "mean_pixels" else float(wy.sum())
    up = upstream.double().reshape(-1) if torch.is_tensor(upstream) else torch.full(lab.shape, float(upstream), dtype=torch.float64)
    if reduction == "none":
        loss, gP = row.view(label.shape), up
    elif reduction == "sum":
        loss, gP = row.sum(), up
    else:
        loss = row.sum() / den if den != 0 else row.sum() * float("nan")
        gP = up / den if den != 0 else torch.zeros_like(up)
    (dz,) = torch.autograd.grad((row * gP).sum(), z)
    out.update(zhat=zhat.detach(), lse=torch.logsumexp(zhat.detach(), -1), valid=valid.view(label.shape), row=row.detach().view(label.shape),
               wy=wy.detach().view(label.shape), den=den, loss=loss.detach(), gP=gP.view(label.shape), dl=dz)
    return out
