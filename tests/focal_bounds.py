"""Inputs, error bounds and an fp32 emulation of the focal kernels, shared by tests/test_focal_gpu.py (the kernels against
the fp64 twin) and tests/test_focal_cpu.py (the emulation against the same bounds on the same inputs, so that the GPU test
cannot pass vacuously).  No GPU is needed to import or run anything here.

Inputs (``focal_inputs``): those of ``_padded_logits`` / ``_labels`` of tests/test_head_classes_gpu.py -- N(0, 3^2) logits,
NaN behind the classes, ~10 % ignore_index, every 7th row a label inside the pad, every 11th a negative one -- drawn from a
CPU generator so that both tests see the same numbers.  On top, at valid rows: every 5th row has its label's logit raised
by 5, 10 ... 40 (q down to 1e-17: below the rounding of d), every 13th lowered by 30 (q = 1, nll ~ 35), and eight further
rows raised by 150: every other exp underflows, lse = x_y and q = 0 exactly in fp32.

Bounds, |got - ref| <= K u S with u = 2^-24 (``check`` / ``rejects`` of tests/test_stream_fp64_gpu.py).  Notation: l = lse,
d = x_y - l, nll = -d, p_y = exp(d), q = 1 - p_y, t = q^(gamma - 1), G = q^gamma = t q, T = gamma t p_y nll, m = G + T,
A = |l| + 1 + |x_y|; exp / log within 2 ulp.

lse       the code of the plain kernels: K = C + 8, S = |l| + 1 (tests/test_loss_options_gpu.py).
d         computed as fl(x_y - l^): |d^ - d| <= (C + 9) u A.  The kernel's p_y^ = exp(d^) (1 + 2u) is exp of a point within
          3u of d^, and 1 - p_y^ rounds once more RELATIVE to q.  So every quantity below is the exact function evaluated at
          points d~ of the interval I = [d - D, min(d + D, 0)], D = (C + 12) u A, with relative roundings on top.  A
          first-order bound at d is NOT enough: where q <= D the relative error of q^ is of order one (the error is
          second order in u), so the sensitivities are bounded over the whole of I, at the end with the larger q and nll:
              nll_hi = nll + D,  q_hi = 1 - exp(-nll_hi),  p_hi = exp(-max(nll - D, 0)),  t_hi = q_hi^(gamma - 1),
              G_hi = t_hi q_hi,  T_hi = gamma t_hi p_hi nll_hi,  m_hi = G_hi + T_hi
          (gamma >= 1: t, G are increasing in q and bounded; gamma = 0: G = m = 1, T = 0).
row_loss  = w_y G nll.  d(G nll)/dd = -m, so moving d inside I costs at most D m_hi.  Roundings at a fixed point: q (1,
          amplified gamma times by the power), the power R(gamma), the two products and w_y (3):
              R = 0 (gamma 0 or 1), 1 (gamma = 2: q q), else 6 (gamma - 1) (L + 1) + 3 for t = exp((gamma - 1) log q):
              log within 2u (|log q| + 1), times gamma - 1 (rounded: 2), the exp's own scaling of its argument and result
              (2 |arg| + 2), t q (1); L = |log q_lo| with q_lo = max(1 - p_hi, 2^-24), the smallest non-zero q^ in I.
          K = C + 12,  S = w_y (A m_hi + G_hi nll_hi (gamma + R + 3) / K).
          Where q^ = 0 the kernel returns 0 = the exact value at d = 0, a point of I (|d^| <= 3u there): same bound.
partial[:, 0]  K = ceil(rows / (256 x 1024)) + 10 + (C + 12), S = sum of the rows' S; [:, 1]: K = ceil(...) + 10,
          S = sum of w_y (both as in tests/test_loss_options_gpu.py).
dlogits   = f (p_c - [c == y]),  f = g w_y m.  |dm/dd| <= gamma t p_y (gamma + 1 + nll) =: M1, using p_y nll <= q in the
          term (gamma - 1) q^(gamma - 2) p_y^2 nll (this is what fails for 0 < gamma < 1, where t itself is unbounded);
          over I: M1_hi = gamma t_hi p_hi (gamma + 1 + nll_hi).  Roundings of m at a fixed point (gamma + R + 5), of f (2),
          the final product (1).  p_c = exp(x_c - l^): (C + 11) u (|x_c| + |l| + 1) relative, as in the plain kernels.
              K = C + 12,  S = |g| w_y [ m_hi p_c (|x_c| + |l| + 1) + (p_c + [c == y]) (A M1_hi + m_hi (gamma + R + 8) / K) ]
                                + 2^-125 (1 + |g| w_y m_hi) / (K u):
          the last term is the underflow threshold of fp32 -- at the rows raised by 150 p_c ~ 1e-66 is 0 in fp32, and a
          product p_c f below 2^-126 may be flushed.
Through ``focal_cross_entropy`` with 'mean', g = upstream / den is formed on the device: K + 13, as in the option route.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.focal_fp64_twin import twin

IGNORE = 255
U = 2.0 ** -24
GAMMAS = (0.0, 1.0, 2.0, 3.5)
SIGMA_CE_BLOCKS = 1024
# rows, classes, pitch: the padded-pitch cases of tests/test_head_classes_gpu.py (CE_LD_CASES) the issue lists -- registers up
# to 64 classes, walking above, one class, one row, a pitch above 4 ceil(classes / 4) -- and the contiguous pair
CASES = [(3001, 9, 12), (198, 37, 40), (257, 1, 4), (1, 3, 4), (4099, 63, 64), (1031, 65, 68), (1031, 67, 68), (513, 5, 16),
         (3001, 40, 40), (1031, 68, 68)]
CASE_IDS = [f"{r}x{c}@{l}" for r, c, l in CASES]


def focal_inputs(rows, nc, ld, seed):
    """CPU tensors: buf (rows, ld) fp32 with NaN in the pad, lab (rows,) int64, sat (<= 8,) the rows raised by 150"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, nc, generator=g) * 3.0
    lab = torch.randint(0, nc, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.1] = IGNORE
    r = torch.arange(rows)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = nc - 1
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    up = valid & (r % 5 == 0)
    down = valid & (r % 13 == 7) & ~up
    rest = torch.nonzero(valid & ~up & ~down)[:, 0]
    sat = rest[torch.linspace(0, rest.numel() - 1, 8).long()].unique() if rest.numel() >= 8 else rest[:0]
    shift = torch.zeros(rows)
    shift[up] = (5.0 + 5.0 * ((r // 5) % 8)).float()[up]
    shift[down] = -30.0
    shift[sat] = 150.0
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    x[r, safe] += shift                                   # zero at rows that are not valid
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = x
    return buf, lab, sat


def focal_weights(nc, seed):
    """fp32 class weights in [0.1, 2.1], class nc // 2 with an exact zero (not where there is one class only)"""
    w = torch.rand(nc, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.1
    if nc > 1:
        w[nc // 2] = 0.0
    return w


def k_sum(rows):
    return -(-rows // (256 * SIGMA_CE_BLOCKS)) + 10


def bounds(x64, lab, nc, weight, gamma, g):
    """The fp64 twin of (x64, lab, weight, gamma) with the per-row upstream g (a float or (rows,)) under reduction 'none',
    plus K = C + 12 and the S of each bound of the module docstring: S_lse (K_lse = C + 8), S_row, S_dl."""
    t = twin(x64, lab, IGNORE, gamma, weight=weight, reduction="none", upstream=g)
    K = nc + 12
    l, xy, nll, wy, sm, oh = t["lse"], t["xy"], t["nll"], t["wy"], t["sm"], t["oh"]
    A = l.abs() + 1.0 + xy.abs()
    D = K * U * A
    nll_hi = nll + D
    nll_lo = (nll - D).clamp_min(0.0)
    q_hi, p_hi = -torch.expm1(-nll_hi), torch.exp(-nll_lo)
    q_lo = (-torch.expm1(-nll_lo)).clamp_min(2.0 ** -24)
    if gamma == 0.0:
        G_hi, T_hi, M1, R = torch.ones_like(l), torch.zeros_like(l), torch.zeros_like(l), torch.zeros_like(l)
    else:
        t_hi = q_hi ** (gamma - 1.0)
        G_hi = t_hi * q_hi
        T_hi = gamma * t_hi * p_hi * nll_hi
        M1 = gamma * t_hi * p_hi * (gamma + 1.0 + nll_hi)
        if gamma == 1.0:
            R = torch.zeros_like(l)
        elif gamma == 2.0:
            R = torch.ones_like(l)
        else:
            R = 6.0 * (gamma - 1.0) * (q_lo.log().abs() + 1.0) + 3.0
    m_hi = G_hi + T_hi
    gr = t["gr"].abs()
    S_row = wy * (A * m_hi + G_hi * nll_hi * (gamma + R + 3.0) / K)
    f_hi = (gr * wy * m_hi)[:, None]
    S_dl = ((gr * wy)[:, None] * (m_hi[:, None] * sm * (x64.abs() + l.abs()[:, None] + 1.0)
                                  + (sm + oh) * (A * M1 + m_hi * (gamma + R + 8.0) / K)[:, None])
            + 2.0 ** -125 * (1.0 + f_hi) / (K * U))
    S_dl = torch.where(t["valid"][:, None], S_dl, torch.zeros_like(S_dl))
    t.update(K=K, K_lse=nc + 8, S_lse=l.abs() + 1.0, S_row=S_row, S_dl=S_dl)
    return t


def emulate_fp32(x32, lab, nc, weight, gamma, g, variant=None, form="reg"):
    """The kernels' formulas step by step in fp32 torch ops (csrc/pointwise.hip: focal_row and the four focal kernels):
    lse, row_loss, w_y and dlogits for the per-row upstream g.  ``variant`` as in the twin: the wrong kernels.  ``form``:
    lse with the row maximum first ("reg") or by the walk with the online rescale ("walk"), tests/loss_regimes.lse_fp32."""
    from tests.loss_regimes import lse_fp32
    f32 = torch.float32
    rows = x32.shape[0]
    gamma_p = 2.0 if variant == "square" else gamma
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    l = lse_fp32(x32, form)
    d = torch.minimum(x32.gather(1, safe[:, None])[:, 0] - l, torch.zeros_like(l))
    w = weight.to(f32) if weight is not None else torch.ones(nc, dtype=f32)
    wy = torch.where(valid, w[safe], torch.zeros_like(l))
    if gamma_p == 0.0:
        qg, m = torch.ones_like(l), torch.ones_like(l)
    else:
        py = torch.exp(d)
        q = (1.0 - py).clamp_min(0.0)
        pos = q > 0
        qs = torch.where(pos, q, torch.ones_like(q))
        t = qs if gamma_p == 2.0 else torch.ones_like(q) if gamma_p == 1.0 else torch.exp(torch.tensor(gamma_p - 1.0, dtype=f32) * torch.log(qs))
        qg = torch.where(pos, t * q, torch.zeros_like(q))
        m = qg if variant == "detached" else torch.where(pos, qg + ((torch.tensor(gamma_p, dtype=f32) * t) * py) * (0.0 - d), torch.zeros_like(q))
    row = torch.where(valid, wy * (qg * (0.0 - d)), torch.zeros_like(l))
    gr = g.to(f32) if torch.is_tensor(g) else torch.full((rows,), float(g), dtype=f32)
    f = torch.where(valid, (gr * wy) * m, torch.zeros_like(l))
    dl = (torch.exp(x32 - l[:, None]) - F.one_hot(safe, nc).to(f32)) * f[:, None]
    assert l.dtype == f32 and row.dtype == f32 and dl.dtype == f32
    return dict(lse=l, row=row, wy=wy, dl=dl, valid=valid)
