"""Inputs, error bounds and an fp32 emulation of the fused upsample + loss kernels for the criteria with options
(csrc/deepsup.hip: sigma_upsample_loss_fwd / _bwd), shared by tests/test_deepsup_loss_gpu.py (the kernels against the fp64
twin of tests/deepsup_loss_twin.py) and tests/test_deepsup_loss_cpu.py (the emulation against the same bounds on the same
inputs, and the wrong variants of the twin against them, so that the GPU test cannot pass vacuously).  No GPU is needed to
import or run anything here.

Inputs: ``tests/deepsup_bounds.deepsup_inputs`` (N(0, 3^2) coarse logits, NaN behind the classes, ~10 % ignore_index, one
negative label, one label inside the pad) and the class weights of ``tests/loss_regimes.weights`` (one exact zero).

Nothing below is a free tolerance.  A bound is the project's bound of the ROW formula, evaluated on the exact interpolated
row z of a fine pixel P, plus what the interpolation adds, plus the summation terms of tests/deepsup_bounds.py.  u = 2^-24;
A_c = the interpolation of |v_c| with the weights of P, Amax = max_c A_c, l = lse(z), p = softmax(z), g_P the upstream gradient
of the pixel, N = (2 s)^2 the largest footprint.

interpolation   |z^_c - z_c| <= 4 u A_c (four roundings on the way of any v, tests/deepsup_bounds.py); lse is 1-Lipschitz in the
                max norm: 4 u Amax on l.
lse             E_lse = u [(C + 8) (|l| + 1) + 4 Amax]                                         (tests/deepsup_bounds.py)
options         row = a (l - z_y) + b (W l - sum_c w_c z_c),  a = (1 - eps) w_y,  b = eps / C,  W = sum_c w_c.
  row             (2 C + 16) u S_row of ``loss_regimes.opt_ref`` for the row formula;  moving the row from z to z^ adds
                  4 u [ a (Amax + A_y) + b (W Amax + sum_c w_c A_c) ].
  d row / d z_c   term e_c = g_P [ (a + b W) p_c - a [c == y] - b w_c ]:  (2 C + 24) u S_dl of ``opt_ref``;  p^_c = exp(z^_c - l^)
                  moves by p_c 4 u (A_c + Amax) relative to its own size:  |g_P| (a + b W) p_c 4 u (A_c + Amax).
focal           row = w_y q^gamma nll;  K = C + 12 and S_row, S_dl of ``loss_regimes.focal_ref`` (tests/focal_bounds.py) for the
                row formula.  The interpolation moves d = z_y - l by dI = 4 u (A_y + Amax).  tests/focal_bounds.py bounds the
                sensitivities over an interval of d, not at a point (where q is of the size of the error a first-order
                bound fails); here the interval is widened by dI:  D' = (C + 12) u (|l| + 1 + |z_y|) + dI, and m_hi, M1_hi are
                taken at its far end as there.
  row             + w_y m_hi dI                               (d (q^gamma nll) / dd = -m)
  d row / d z_c   + |g_P| w_y [ M1_hi (p_c + [c == y]) dI + m_hi p_c 4 u (A_c + Amax) ]      (|dm / dd| <= M1)
                The backward multiplies g_P by coef = w_y m, stored by the forward, where the row kernels form (g w_y) m:
                one rounding either way, counted in the (gamma + R + 8) of S_dl.
ohem            the selection is exact or the test's inputs are wrong (``ohem_gap``: no valid pixel within 2 E_row of tau, a
                condition on the inputs); then the options bounds with eps = 0 on the mined labels.
partial         [:, 0]: sum of the rows' E_row + (ceil(rows / 2^18) + 10) u sum |row| over the rows of a workgroup (a thread's
                adds, the wave, the four waves: tests/deepsup_bounds.py).  [:, 1]: (ceil(rows / 2^18) + 10) u sum w_y -- the
                weights are no whole numbers; without weights the pairs' second halves are whole numbers below 2^24, exact.
loss            'none' E_row;  'sum' E_num = sum E_partial[:, 0] + 13 u sum |partial[:, 0]| (torch's tree over 1024 pairs);
                'mean' = num / den with E_den alike:  E_num / den + |loss| E_den / den + u |loss|.
dlogits         an element is sum_P wgt_P e_c(P) over up to N fine pixels, wgt exact for s a power of two, one rounding per
                accumulation and butterfly step in any order:
                    E_dl = sum_P wgt_P E_e(P) + (N + 2) u sum_P wgt_P |e|_c(P) + N 2^-126,
                |e|_c the sum of the magnitudes of the terms of e_c.  Through the front end with 'mean' g = upstream / den is
                formed on the device from the fp32 den: (ceil(rows / 2^18) + 10 + 13 + 3) u |dl| more.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import focal_bounds
from tests.deepsup_bounds import CASES as BASE_CASES
from tests.deepsup_bounds import IGNORE, SIGMA_CE_BLOCKS, U, deepsup_inputs
from tests.deepsup_fp64_twin import interp_matrix, taps
from tests.deepsup_loss_twin import adjoint, twin, upsample
from tests.loss_regimes import GAMMAS, emulate_ce_fp32, focal_ref, opt_ref, weights

GRID_CASE = (1, 16, 17, 32, 5, 8)          # 278528 fine pixels > 2^18: the forward's grid-stride loop takes a second trip
G1_CASE = (4, 120, 160, 2, 40, 40)         # 768000 backward items >= 2^19: one lane per item (G = 1)
CASES = list(BASE_CASES) + [GRID_CASE]     # every kind; G1_CASE runs one kind only (the CPU twin's time)
CASE_IDS = ["%dx%dx%d_x%d_%d@%d" % c for c in CASES]

# name -> the criterion: kind, class weights?, eps, gamma, reduction
KINDS = {
    "w": dict(kind="options", weighted=True, eps=0.0, gamma=0.0, reduction="mean"),
    "w+eps": dict(kind="options", weighted=True, eps=0.1, gamma=0.0, reduction="mean"),
    "eps": dict(kind="options", weighted=False, eps=0.1, gamma=0.0, reduction="mean"),
    "sum": dict(kind="options", weighted=True, eps=0.0, gamma=0.0, reduction="sum"),
    "none": dict(kind="options", weighted=True, eps=0.1, gamma=0.0, reduction="none"),
}
for _g in GAMMAS:
    KINDS[f"focal{_g:g}"] = dict(kind="focal", weighted=False, eps=0.0, gamma=_g, reduction="mean")
    KINDS[f"focal{_g:g}w"] = dict(kind="focal", weighted=True, eps=0.0, gamma=_g, reduction="mean")
KIND_IDS = list(KINDS)
G1_KIND = "w+eps"

# OHEM: (case, seed, thresh, min_kept, what decides) -- found on the CPU with the twin (``ohem_gap`` is empty for each; in the
# mining pairs 0 < kept < num_valid).  "kth": the min_kept-th value is above thresh in the p domain; "thresh": below;
# "all": min_kept > num_valid, no mining.
OHEM_PAIRS = [((1, 3, 5, 8, 5, 8), 0, 0.7, 800, "kth"),
              ((2, 5, 4, 4, 37, 40), 0, 0.05, 16, "thresh"),
              ((2, 2, 3, 16, 40, 40), 0, 0.7, 100000, "all")]
OHEM_IDS = [p[4] for p in OHEM_PAIRS]


def class_weights(nc, weighted=True, seed=11):
    return weights(nc, seed) if weighted else None


def upstream_of(spec, lab, seed=5):
    """the gradient of the result: 1 for 'mean' / 'sum', a random fp32 per pixel (one exact zero) for 'none'"""
    if spec["reduction"] != "none":
        return 1.0
    up = torch.randn(lab.shape, generator=torch.Generator().manual_seed(seed))
    up.view(-1)[0] = 0.0
    return up


def k_sum(rows):
    return -(-rows // (256 * SIGMA_CE_BLOCKS)) + 10


def _blocks(rows):
    return (torch.arange(rows) // 256) % SIGMA_CE_BLOCKS


def _focal_hi(nll, D, gamma):
    """m_hi and M1_hi of tests/focal_bounds.py over the interval of half width D around d = -nll"""
    if gamma == 0.0:
        return torch.ones_like(nll), torch.zeros_like(nll)
    nll_hi, nll_lo = nll + D, (nll - D).clamp_min(0.0)
    q_hi, p_hi = -torch.expm1(-nll_hi), torch.exp(-nll_lo)
    t_hi = q_hi ** (gamma - 1.0)
    return t_hi * q_hi + gamma * t_hi * p_hi * nll_hi, gamma * t_hi * p_hi * (gamma + 1.0 + nll_hi)


def bounds(x64, lab, s, spec, w, upstream=1.0, variant=None, thresh=0.7, min_kept=0):
    """The fp64 twin of (x64 (B, h, w, nc), lab, the criterion `spec` with the weight `w`) -- ``variant`` reaches the twin
    alone, the bounds are those of the right formulation -- plus the bounds of the module docstring: E_lse, E_row (B, H, W),
    partial (1024, 2) exact in the kernels' layout, E_partial (1024, 2), E_loss (a float; E_row for 'none'), E_dl (B, h, w, nc)
    for the kernel handed the twin's g_P, and E_front: E_dl with the device-formed denominator of 'mean' on top."""
    B, h, wd, nc = x64.shape
    kind = spec["kind"]
    kw = dict(weight=w, eps=spec["eps"], gamma=spec["gamma"], thresh=thresh, min_kept=min_kept, reduction=spec["reduction"],
              upstream=upstream)
    t = twin(x64, lab, s, IGNORE, kind, variant=variant, **kw)
    r = twin(x64, lab, s, IGNORE, kind, **kw) if variant is not None else t
    rows = lab.numel()
    z = r["zhat"].reshape(-1, nc)
    l = r["lse"].reshape(-1)
    gP = r["gP"].reshape(-1)
    lab_eff = (r["mined"] if kind == "ohem" else lab).reshape(-1)
    A = upsample(x64.abs(), s).reshape(-1, nc)
    Amax = A.max(-1).values
    E_lse = U * ((nc + 8) * (l.abs() + 1.0) + 4.0 * Amax)
    if kind == "focal":
        gamma = spec["gamma"]
        f = focal_ref(z, lab_eff, nc, w, gamma, gP)
        K, valid, wy, sm, oh = f["K"], f["valid"], f["wy"], f["sm"], f["oh"]
        safe = torch.where(valid, lab_eff, torch.zeros_like(lab_eff))
        Ay = A.gather(1, safe[:, None])[:, 0]
        dI = 4.0 * U * (Ay + Amax)
        m_hi, M1_hi = _focal_hi(f["nll"], K * U * (l.abs() + 1.0 + f["xy"].abs()) + dI, gamma)
        E_row = K * U * f["S_row"] + wy * m_hi * dI
        gw = (gP.abs() * wy)[:, None]
        E_e = K * U * f["S_dl"] + gw * ((M1_hi * dI)[:, None] * (sm + oh) + m_hi[:, None] * sm * 4.0 * U * (A + Amax[:, None]))
        mag = gw * f["m"][:, None] * (sm + oh)
    else:
        eps = spec["eps"] if kind == "options" else 0.0
        o = opt_ref(z, lab_eff, nc, w, eps, gP)
        valid, wy = o["valid"], o["wy"]
        safe = torch.where(valid, lab_eff, torch.zeros_like(lab_eff))
        Ay = A.gather(1, safe[:, None])[:, 0]
        w64 = w.double() if w is not None else torch.ones(nc, dtype=torch.float64)
        W = w64.sum()
        a, b = (1.0 - eps) * wy, eps / nc
        sm = torch.softmax(z, 1)
        oh = F.one_hot(safe, nc).double()
        E_row = (2 * nc + 16) * U * o["S_row"] + 4.0 * U * (a * (Amax + Ay) + b * (W * Amax + (w64 * A).sum(1)))
        ga = gP.abs()[:, None]
        E_e = (2 * nc + 24) * U * o["S_dl"] + ga * (a[:, None] + b * W) * sm * 4.0 * U * (A + Amax[:, None])
        mag = ga * ((a[:, None] + b * W) * sm + a[:, None] * oh + b * w64[None, :])
    vcol = valid[:, None]
    E_row = torch.where(valid, E_row, torch.zeros_like(E_row))
    E_e, mag = torch.where(vcol, E_e, torch.zeros_like(E_e)), torch.where(vcol, mag, torch.zeros_like(mag))
    blk, zero = _blocks(rows), torch.zeros(SIGMA_CE_BLOCKS, dtype=torch.float64)
    row_t, row_r = t["row"].reshape(-1), r["row"].reshape(-1)
    partial = torch.stack([zero.index_add(0, blk, row_t), zero.index_add(0, blk, t["wy"].reshape(-1))], 1)
    part_r1 = zero.index_add(0, blk, r["wy"].reshape(-1))
    E_partial = torch.stack([zero.index_add(0, blk, E_row) + k_sum(rows) * U * zero.index_add(0, blk, row_r.abs()),
                             k_sum(rows) * U * part_r1], 1)
    E_num = float(E_partial[:, 0].sum()) + 13 * U * float(row_r.abs().sum())
    E_den = float(E_partial[:, 1].sum()) + 13 * U * float(part_r1.sum())
    if spec["reduction"] == "none":
        E_loss = E_row.view(lab.shape)
    elif spec["reduction"] == "sum":
        E_loss = E_num
    else:
        den = r["den"]
        E_loss = E_num / den + abs(float(r["loss"])) * E_den / den + U * abs(float(r["loss"])) if den > 0 else float("nan")
    N = (2 * s) ** 2
    shp = (B, h * s, wd * s, nc)
    E_dl = adjoint(E_e.view(shp), h, wd, s) + (N + 2) * U * adjoint(mag.view(shp), h, wd, s) + N * 2.0 ** -126
    E_front = E_dl + ((k_sum(rows) + 16) * U * r["dl"].abs() if spec["reduction"] == "mean" else 0.0)
    t.update(E_lse=E_lse.view(lab.shape), E_row=E_row.view(lab.shape), partial=partial, E_partial=E_partial, E_loss=E_loss, E_dl=E_dl,
             E_front=E_front)
    return t


def ohem_gap(x64, lab, s, thresh, min_kept):
    """(twin of the selection, the number of valid fine pixels with |nll - tau| <= 2 E_row): a pixel that close to tau could
    change sides by rounding alone (the pixel that supplies tau itself, when the k-th value decides, is not counted: the
    kernels take tau from its own fp32 nll and keep ties).  E_row is the bound of the unweighted nll the selection reads.  A condition on the
    inputs, not a tolerance."""
    spec = dict(kind="ohem", weighted=False, eps=0.0, gamma=0.0, reduction="mean")
    nll_spec = dict(spec, kind="options")
    b = bounds(x64, lab, s, nll_spec, None)
    t = twin(x64, lab, s, IGNORE, "ohem", thresh=thresh, min_kept=min_kept)
    sel = t["sel"]
    near = sel["valid"] & (sel["dist"] <= 2.0 * b["E_row"].reshape(-1))
    if sel["tau_row"] >= 0:
        near[sel["tau_row"]] = False        # the pixel whose nll IS tau: kept on either side of any rounding (ties are kept)
    return t, int(near.sum())


def interpolate_fp32(buf, s, nc):
    """the interpolated rows as the kernels form them, axis by axis in fp32 (tests/deepsup_bounds.emulate_fp32)"""
    f32 = torch.float32
    B, h, w, ld = buf.shape

    def lerp(n, v, dim):
        i0, i1, lam = taps(n, s)
        shape = [1] * v.dim()
        shape[dim] = -1
        lam = lam.to(f32).view(shape)
        return (1.0 - lam) * v.index_select(dim, i0) + lam * v.index_select(dim, i1)

    return lerp(w, lerp(h, buf[..., :nc], 1), 2)


def emulate_fp32(buf, lab, s, nc, spec, w, upstream=1.0, thresh=0.7, min_kept=0):
    """The kernels' formulas and the front end's reduction in fp32 torch ops on the padded buffer buf (B, h, w, ld): the
    interpolated rows, then the row kernels' emulation in its walking form (tests/loss_regimes.emulate_ce_fp32,
    tests/focal_bounds.emulate_fp32), the selection in the nll domain for "ohem", the pairs in the kernels' layout, the
    loss, g_P as the Function forms it and dlogits (pad columns zero)."""
    f32 = torch.float32
    B, h, wd, ld = buf.shape
    kind, red = spec["kind"], spec["reduction"]
    z = interpolate_fp32(buf, s, nc).reshape(-1, nc)
    flat = lab.reshape(-1)
    rows = flat.numel()
    out = {}
    if kind == "ohem":
        e = emulate_ce_fp32(z, flat, nc, None, 0.0, 0.0, "walk")
        nll, valid = e["row"], e["valid"]
        nv = int(valid.sum())
        keep = valid
        if 0 < min_kept <= nv:
            kth = torch.sort(nll[valid], descending=True).values[min_kept - 1]
            tau = torch.minimum(torch.tensor(0.0 - math.log(thresh), dtype=f32), kth)
            keep = valid & ~(nll < tau)
        flat = torch.where(keep, flat, torch.full_like(flat, IGNORE))
        out.update(keep=keep.view(lab.shape), counts=(nv, int(keep.sum())))

    def run(g):
        if kind == "focal":
            return focal_bounds.emulate_fp32(z, flat, nc, w, spec["gamma"], g, form="walk")
        return emulate_ce_fp32(z, flat, nc, w, spec["eps"] if kind == "options" else 0.0, g, "walk")

    e = run(0.0)
    # a workgroup's sums: fp32 values added in fp64 and rounded once -- index_add's own serial fp32 order (hundreds of adds per
    # workgroup at 2^18 pixels and more) is not the kernels', whose thread / wave / workgroup adds the bound counts
    blk, zero = _blocks(rows), torch.zeros(SIGMA_CE_BLOCKS, dtype=torch.float64)
    partial = torch.stack([zero.index_add(0, blk, e["row"].double()), zero.index_add(0, blk, e["wy"].double())], 1).to(f32)
    tot = partial.sum(0)
    up = upstream.to(f32).reshape(-1) if torch.is_tensor(upstream) else torch.full((rows,), float(upstream), dtype=f32)
    if red == "mean":
        loss = tot[0] / tot[1]
        gP = up / tot[1] if float(tot[1]) > 0 else torch.zeros_like(up)
    else:
        loss, gP = (tot[0] if red == "sum" else e["row"].view(lab.shape)), up
    d = run(gP)["dl"]
    d = torch.where(e["valid"][:, None], d, torch.zeros_like(d))
    Uh, Uw = interp_matrix(h, s).to(f32), interp_matrix(wd, s).to(f32)
    dl = torch.zeros(B, h, wd, ld, dtype=f32)
    dl[..., :nc] = torch.einsum("Yi,bYjc->bijc", Uh, torch.einsum("Xj,bYXc->bYjc", Uw, d.view(B, h * s, wd * s, nc)))
    assert e["lse"].dtype == f32 and partial.dtype == f32 and dl.dtype == f32
    out.update(lse=e["lse"].view(lab.shape), row=e["row"].view(lab.shape), partial=partial, loss=loss, dl=dl)
    return out
