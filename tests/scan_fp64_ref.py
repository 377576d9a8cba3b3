"""fp64 reference of the selective scan with error companions (plain torch, any device; no fp32 operation, no CPU oracle).

``reference`` takes the operator's operands in the operator's layout -- u (b, KD >> u_gshift, L), delta (b, KD, L),
A (KD, N), B / C (b, G, N, L), D / delta_bias (KD,), dout (b, KD >> dout_gshift, L), with the fused path's ``rev_mask``
(bit g: group g runs over the sequence backwards) -- and returns dicts of float64 tensors over the keys ``OUTPUTS``:
the values and, for each, the companion S of the test  |got - ref| <= U S,  U = 2^-24.  It works a batch image and a
block of rows at a time (``elems`` caps rows x N x L of a block), every recurrence as a scan over (a, x) pairs
(``lin_scan``: blocks walked side by side, their ends joined by a doubling scan; no loop over the sequence).

The model (scan order; a reversed group is flipped on the way in and out).  delta_t = softplus(raw_t) (threshold 20) or
raw_t, a_t = exp(delta_t A_n), w_t = delta_t B_t u_t:

    x_t = a_t x_{t-1} + w_t                                    out_t = sum_n C_t x_t + D u_t
    X_t = a_t X_{t-1} + |w_t|                                  what the state is summed from
    E_t = a_t (E_{t-1} + k_t |delta_t A| X_{t-1}) + c X_t + esp_t |w_t| + under_t       error budget of x_t, units of U
    lambda_t = C_t g_t + a_{t+1} lambda_{t+1},   Lambda_t the same over |C_t g_t|
    F_t = a_{t+1} (F_{t+1} + k_{t+1} |delta_{t+1} A| Lambda_{t+1}) + c_b Lambda_t + under_t

    S_out    = sum_n |C| (E + c_o X) + c_o |D u| + |out| + ETA (N + 2)
    S_du     = delta sum_n |B| (F + (c_g + esp) Lambda) + c_g |D g| + |du| + ETA (sum_n |B| Lambda + N + 2)
    dd_pre   = u sum_n B lambda + sum_n A (a x_{t-1}) lambda
    S_ddpre  = |u| sum_n |B| (F + c_g Lambda) + sum_n |A| (aE Lambda + aX F + c_g aX Lambda),  aX = a X_{t-1},
               aE = a (E_{t-1} + k |delta A| X_{t-1}) + 2 aX
    S_ddelta = sigma S_ddpre + c_sig |ddelta| + |ddelta| + ETA (|dd_pre| + N + 2)          (sigma = 1 without softplus)
    S_dA     = sum_{b,t} |delta| (aE Lambda + aX F + (3 + esp) aX Lambda) + K_row sum |delta| aX Lambda + |dA|
    S_dB     = sum_rows |delta u| (F + (c_g + esp) Lambda) + K_rows sum_rows |delta u| Lambda + |dB|
    S_dC     = sum_rows |g| (E + c_o X) + K_rows sum_rows |g| X + |dC|
    S_dD     = K_row sum |g u| ,   S_ddelta_bias = sum S_ddelta + K_row sum |ddelta|

Constants (``constants``).  Every line is a rounding of the kernels, U each unless noted; v_exp_f32 / v_log_f32 /
v_rcp_f32 are 1 ulp = 2 U.  They are counted from the source, not fitted to what a kernel achieves.

  c = 3, per position a contribution travels (the larger of the two ways into x_t):
      the carried part a x:  v_exp_f32 result 2 (scan_fwd.hip:170, scan_fwd4.hip:118, scan_fwdr.hip:194/435,
      scan_bwd.hip:232, scan_bwd2.hip:214, scan_bwd3.hip:184, scan_bwd4.hip:232, scan_bwdr.hip:318) + the fma 1
      (scan_fwd.hip:172/205, scan_fwd4.hip:120/134, scan_fwdr.hip:195/436, scan_bwd4.hip:235/245);
      the injected part w:   delta * u 1 (scan_fwd.hip:121, scan_fwd4.hip:87, scan_fwdr.hip:152, scan_bwd4.hip:173)
      + times B 1 (scan_fwd.hip:171, scan_fwd4.hip:119, scan_fwdr.hip:195, scan_bwd4.hip:233) + the fma 1.
      A lane that is skipped by the scan network instead of walked costs v_exp 2 + one product 1 for its T >= 4
      positions (scan_fwd.hip:178, scan_device.h:289-290 SIGMA_MSTEP), which the same 3 per position covers.
  c_b = 5, the adjoint step e = a (g C + e) (scan_bwd4.hip:250/264-265, scan_bwdr.hip:491): g * C 1
      (scan_bwd4.hip:234), the add 1, the product 1, v_exp 2.
  k = 2.5 + (T - 1) + levels_log, roundings that land in the exponent, relative to sum |delta A|:
      A * log2(e) 1 and the constant itself 0.5 (scan_bwd4.hip:218; scan_device.h:12), the product with delta or with
      the lane's sum of delta 1 (scan_fwd.hip:170/178), the serial sum of the lane's T deltas T - 1 (scan_fwd.hip:126,
      scan_fwd4.hip:89, scan_bwd4.hip:181, scan_bwd2.hip:220), and where the decay travels as a sum of log2 (the
      wave-split forward, scan_device.h:216-231: 6 adds; the row-lane segment summaries, scan_fwdr.hip:199 and
      scan_bwdr.hip:501: one fma per tile of the segment, after a 16-term serial sum scan_fwdr.hip:174) those adds.
      T and the segment geometry come from the planner's report.
  c_0 = levels + 2, once per output: the fma of each level of the scan network (scan_device.h:297-308: 6;
      scan_quad.h:81-100: 4; none in the row-lane kernels), the hand-over of the state entering the lane
      (scan_fwd.hip:194, scan_fwd4.hip:125) 1 and, with sequence segments, the fma that applies a summary 1 per segment.
  c_r = N + 1: the sum over the states is a serial fma chain started from D u (scan_fwd.hip:122/206,
      scan_fwd4.hip:88/135; the row-lane kernels add NS = N / waves states serially, then the waves and D u,
      scan_fwdr.hip:196/214/403, at most as deep).  c_o = c_0 + c_r; c_g = c_0 + c_r + 2 (the gradient forms
      dx = g C + e 1, scan_bwd4.hip:264, and the product with delta or u 1, scan_bwd4.hip:366/382).
  esp_t, the relative error of delta from softplus_ref (scan_device.h:181-191), with kappa = |raw| sigmoid / softplus
      the condition of softplus: raw = delta + bias 1 kappa (scan_fwd.hip:117), raw * log2(e) 1.5 kappa (:183),
      v_exp 2 (:183), v_log 2 and * ln 2 1.5 (:185), v_rcp 2, the two products 2 (:187); 1 + e is undone by w - 1
      (Kahan).  esp = 9.5 + 2.5 kappa, rounded up to 10 + 2.5 kappa.  It enters w (esp |w|) and the exponent (k_t = k + esp).
  c_sig = esp + 15, softplus' (the largest over the families): scan_bwd4.hip:349-361 rebuilds u sdxB from
      (delta u) sdxB / delta (v_rcp 2, two products 2, delta u 1: 5) and sigmoid as 1 - exp(-delta) (the error of delta,
      esp, at a condition <= 1; v_exp and the subtraction near 0.25, or the degree-7 series: 10 at most,
      scan_bwd4.hip:347); the others take e / (1 + e) (scan_bwd2.hip:319-320, scan_bwd3.hip:278-279,
      scan_bwd.hip:347: 2.5 (1 - sigmoid) |raw| + 7 <= esp + 15).
  under_t = ETA (4 + |u B| + (1 + |A|) max_t X), ETA = 2^-126 / U: a delta, a decay (or a product of decays) or a
      product below 2^-126 may be flushed to zero by v_exp_f32 / v_rcp_f32 / the multipliers; the allowance of each
      travels through the same recurrence.  scan_bwd4.hip:351 returns ddelta = 0 where delta < 2^-126: ETA |dd_pre|.
  K_rows (dB, dC: the sum over the rows of a group): rows / P + P, the rows a workgroup adds (order taken as serial:
      fold16 / fold32 / colsum1, scan_bwd4.hip:274/292) and the P slabs reduce_partials_kernel adds
      (scan_bwd.hip:409-460); P = workgroups / (batch G segments) from the planner's report.
  K_row (dA, dD, ddelta_bias): row_sum_depth of tests/test_deterministic_cpu.py, default and deterministic form; dA
      takes the same road as dD (scan_bwd4.hip:269/279/335, scan_bwd2.hip:270/301, scan_bwd3.hip:218/230,
      scan_bwdr.hip:398); scan_bwd.hip adds its tiles in LDS first (:279/296/299): T + 6 + tiles + batch.
  16-bit IO: the operands are exact, the arithmetic is fp32, and out / du / ddelta -- through the binding dB / dC too,
      which it returns in the dtype of B / C (selective_scan_cuda_core.py bwd_ext, ``io_bc``); the C ABI writes them in
      fp32 -- are rounded to the IO format: half a unit in the last place of their own format (2^-8 bf16, 2^-11 f16, and
      2^-25 absolute for f16 denormals) on |ref|.
"""
from __future__ import annotations

import dataclasses
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
ETA = TINY / U
OUTPUTS = ("out", "du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")
IO_HALF_ULP = {"float32": 0.0, "bfloat16": 2.0 ** -8 / U, "float16": 2.0 ** -11 / U}


@dataclasses.dataclass(frozen=True)
class Constants:
    k: float            # exponent roundings (without esp)
    c_0: float          # scan network + hand-over, once per output
    K_rows: float       # depth of the sum over the rows of a group (dB, dC)
    K_row: float        # depth of the per-row sums over batch and sequence (dA, dD, ddelta_bias)
    c: float = 3.0
    c_b: float = 5.0


def constants(fwd_family, bwd_family, fwd_plan, bwd_plan, batch, KD, L, N, G, det=False):
    """the constants of a launch from the two plan reports {items, rows per workgroup, workgroups, lds, tiles, states};
    the forward and the backward recompute the same states, so k and c_0 take the larger of the two kernels"""
    from tests.test_deterministic_cpu import row_sum_depth, segments_of

    def k_c0(family, plan, segs):
        if family in ("Fwdr", "Bwdr"):                       # a lane is a row: serial walk, summaries across segments
            seg_tiles = -(-(-(-L // 16)) // segs)
            return 2.5 + ((15 + seg_tiles) if segs > 1 else 0), 2 + (segs if segs > 1 else 0)
        if family in ("Fwd4", "Bwd4"):                       # 16 lanes x 10 positions, 4 levels
            return 2.5 + 9, 4 + 2 + (segs if segs > 1 else 0)
        T = max(int(plan[0]), 1)                             # 64 lanes x T positions, 6 levels (+ 6 adds of log2 decays)
        return 2.5 + (T - 1) + 6, 6 + 2 + max(int(plan[4]), 1)

    fsegs = max(int(fwd_plan[4]), 1) if fwd_family == "Fwdr" else 1
    kf, cf = k_c0(fwd_family, fwd_plan, fsegs)
    if bwd_plan is None:
        return Constants(k=kf, c_0=cf, K_rows=0.0, K_row=0.0)
    segs = segments_of(list(bwd_plan))
    kb, cb = k_c0(bwd_family, bwd_plan, segs)
    rows = KD // G
    P = max(int(bwd_plan[2]) // (batch * G * segs), 1)
    if bwd_family == "Bwd":
        T = max(int(bwd_plan[0]), 1)
        K_row = T + 6 + -(-L // (64 * T)) + batch
    elif bwd_family == "Bwd3":                               # the road of Bwd2: T per lane, wave_sum, one result per tile
        T = max(int(bwd_plan[0]), 1)
        tiles = -(-L // (64 * T))
        K_row = (T + 6 + tiles + batch) if det else (T + 6 + batch * tiles)
    else:
        K_row = row_sum_depth(list(bwd_plan), batch, L)[1 if det else 0]
    return Constants(k=max(kf, kb), c_0=max(cf, cb), K_rows=-(-rows // P) + P, K_row=float(K_row))


# ---------------------------------------------------------------------------------------------------------------------
def _doubling(a, ws):
    """x_t = a_t x_{t-1} + w_t along the last dimension, in place in ``ws`` (``a`` is consumed): after the step of
    distance d, (a_t, w_t) is the composition of positions t - 2d + 1 .. t"""
    L = a.shape[-1]
    d = 1
    while d < L:
        for w in ws:
            w[..., d:] += a[..., d:] * w[..., :-d]
        if 2 * d < L:
            a[..., d:] = a[..., d:] * a[..., :-d]
        d *= 2
    return ws


def lin_scan(a, ws, block=32):
    """x_t = a_t x_{t-1} + w_t along the last dimension (x_{-1} = 0) for every w of ``ws``; returns new tensors.
    Short rows: a doubling scan over (a, x) pairs.  Long rows: blocks of ``block`` positions laid out position-major --
    the blocks are walked side by side (block - 1 steps on contiguous slices, with the running product of a), the
    block ends are scanned by doubling, and every position takes its block's incoming state times that product."""
    L = a.shape[-1]
    if L < 4 * block:
        return _doubling(a.clone(), [w.clone() for w in ws])
    nb = -(-L // block)

    def blocks(t, fill):                                 # (..., L) -> (block, ..., nb), padded with the identity
        if nb * block != L:
            t = torch.nn.functional.pad(t, (0, nb * block - L), value=fill)
        return t.reshape(*t.shape[:-1], nb, block).movedim(-1, 0).contiguous()

    at, wts = blocks(a, 1.0), [blocks(w, 0.0) for w in ws]
    for j in range(1, block):
        for wt in wts:
            wt[j].addcmul_(at[j], wt[j - 1])
        at[j].mul_(at[j - 1])
    ends = _doubling(at[block - 1].clone(), [wt[block - 1].clone() for wt in wts])
    out = []
    for wt, e in zip(wts, ends):
        wt.addcmul_(at, _shift_right(e)[None])
        out.append(wt.movedim(0, -1).reshape(*a.shape[:-1], nb * block)[..., :L])
    return out


def lin_scan_rev(a_next, ws):
    """y_t = a_next_t y_{t+1} + w_t (y_L = 0); returns new tensors"""
    return [f.flip(-1) for f in lin_scan(a_next.flip(-1), [w.flip(-1) for w in ws])]


def _shift_right(t):                       # t_{t-1}, zero at the first position
    out = torch.zeros_like(t)
    out[..., 1:] = t[..., :-1]
    return out


def _shift_left(t, fill=0.0):              # t_{t+1}
    out = torch.full_like(t, fill)
    out[..., :-1] = t[..., 1:]
    return out


def softplus64(raw, threshold=20.0):
    """the operator's softplus in fp64: raw above the threshold, log1p(exp(raw)) below; and its derivative"""
    sp = torch.where(raw > threshold, raw, torch.log1p(torch.exp(torch.clamp(raw, max=threshold))))
    sig = torch.where(raw > threshold, torch.ones_like(raw), torch.sigmoid(raw))
    return sp, sig


def reference(u, delta, A, B, C, D, bias, dout, softplus, consts: Constants, *, rev_mask=0, u_gshift=0, dout_gshift=0,
              io="float32", io_bc=True, elems=1 << 25, wrong=None, wrong_at=0, finite=True):
    """(ref, S, sums): dicts of float64 tensors in the operator's layout (du one row per channel row), ref and S over
    OUTPUTS, sums = sum |terms| of the five deep sums (for ``rebound``).  ``wrong``
    names a plausible defect (negative controls; only this reference code runs in them):
    bf16_decay, exp_1e-5, drop_carry (the last state's carry into position ``wrong_at``), threshold10, sigmoid1_10,
    adjoint_at, rev_skip_first, dB_last_row, dC_last_row, dA_last_image, out_D, du_D.  ``finite=False``: operands with
    planted non-finite elements (tests/scan_footprint.py); only WHERE ref is non-finite means anything then, S does not."""
    dev = delta.device
    f8 = lambda t: None if t is None else t.detach().to(torch.float64)
    u, delta, A, B, C, D, bias, dout = map(f8, (u, delta, A, B, C, D, bias, dout))
    batch, KD, L = delta.shape
    G, N = B.shape[1], B.shape[2]
    rows = KD // G
    cs = consts
    c_r = N + 1
    c_o, c_g = cs.c_0 + c_r, cs.c_0 + c_r + 2
    ref = {"out": torch.empty_like(delta), "du": torch.empty_like(delta), "ddelta": torch.empty_like(delta),
           "dA": torch.zeros(KD, N, dtype=torch.float64, device=dev), "dB": torch.zeros_like(B), "dC": torch.zeros_like(C),
           "dD": torch.zeros(KD, dtype=torch.float64, device=dev), "ddelta_bias": torch.zeros(KD, dtype=torch.float64, device=dev)}
    S = {k: torch.zeros_like(v) for k, v in ref.items()}
    sums = {k: torch.zeros_like(ref[k]) for k in ("dA", "dB", "dC", "dD", "ddelta_bias")}      # sum |terms| of the deep sums
    step = max(1, min(rows, elems // max(N * L, 1)))
    for b in range(batch):
        for g in range(G):
            rev = bool((rev_mask >> g) & 1)
            fl = (lambda t: t.flip(-1)) if rev else (lambda t: t)
            Bg, Cg = fl(B[b, g])[None], fl(C[b, g])[None]                               # (1, N, L)
            for r0 in range(g * rows, (g + 1) * rows, step):
                r1 = min(r0 + step, (g + 1) * rows)
                ur = slice(r0 - (g - (g >> u_gshift)) * rows, r1 - (g - (g >> u_gshift)) * rows)
                gr = slice(r0 - (g - (g >> dout_gshift)) * rows, r1 - (g - (g >> dout_gshift)) * rows)
                uu, gg = fl(u[b, ur]), fl(dout[b, gr])                                  # (R, L)
                raw = fl(delta[b, r0:r1]) + (bias[r0:r1, None] if bias is not None else 0.0)
                An = A[r0:r1, :, None]                                                   # (R, N, 1)
                Dd = D[r0:r1, None] if D is not None else torch.zeros(r1 - r0, 1, dtype=torch.float64, device=dev)
                if softplus:
                    dl, sig = softplus64(raw, 10.0 if wrong == "threshold10" else 20.0)
                    kappa = raw.abs() * torch.sigmoid(raw) / torch.clamp(softplus64(raw)[0], min=1e-300)
                    esp = 10.0 + 2.5 * kappa
                    if wrong == "sigmoid1_10":
                        sig = torch.where(raw > 10.0, torch.ones_like(sig), sig)
                else:
                    dl, sig, esp = raw, None, torch.zeros_like(raw)
                if wrong == "rev_skip_first" and rev:
                    dl = dl.clone()
                    dl[:, 0] = 0.0
                dl_decay = dl.to(torch.bfloat16).to(torch.float64) if wrong == "bf16_decay" else dl
                a = torch.exp(dl_decay[:, None, :] * An)                                # (R, N, L)
                if wrong == "exp_1e-5":
                    a = a * (1.0 + 1e-5)
                if wrong == "drop_carry":
                    a[:, N - 1, wrong_at] = 0.0
                zA = (dl[:, None, :] * An).abs()
                kt = (cs.k + esp)[:, None, :] * zA                                      # k_t |delta_t A|
                w = (dl * uu)[:, None, :] * Bg
                w[..., 0] += a[..., 0] * 0.0                    # a_0 x_{-1}, x_{-1} = 0: exact, and a non-finite a_0 is seen
                # ---- forward: x, X, then E
                x, X = lin_scan(a, [w, w.abs()])
                Xmax = X.amax(-1, keepdim=True)
                under = ETA * (4.0 + (uu[:, None, :] * Bg).abs() + (1.0 + An.abs()) * Xmax)
                aX = a * _shift_right(X)
                (E,) = lin_scan(a, [kt * aX + cs.c * X + esp[:, None, :] * w.abs() + under])
                aE = a * _shift_right(E) + kt * aX + 2.0 * aX
                Du = Dd * uu
                y = (Cg * x).sum(1) + Du * ((1.0 + 1e-4) if wrong == "out_D" else 1.0)
                S_y = (Cg.abs() * (E + c_o * X)).sum(1) + c_o * Du.abs() + y.abs() * (1.0 + IO_HALF_ULP[io]) + ETA * (N + 2)
                ref["out"][b, r0:r1], S["out"][b, r0:r1] = fl(y), fl(S_y)
                # ---- adjoint: lambda, Lambda, then F
                an = _shift_left(a, 1.0)
                if wrong == "adjoint_at":
                    an = a.clone()
                src = gg[:, None, :] * Cg
                lam, Lam = lin_scan_rev(an, [src, src.abs()])
                anL = an * _shift_left(Lam)
                (F,) = lin_scan_rev(an, [_shift_left(kt) * anL + cs.c_b * Lam + ETA * (4.0 + (1.0 + An.abs()) * Lam.amax(-1, keepdim=True))])
                # ---- gradients
                sB = (Bg * lam).sum(1)
                du = dl * sB + Dd * gg * ((1.0 + 1e-4) if wrong == "du_D" else 1.0)
                BL = (Bg.abs() * Lam).sum(1)
                S_du = (dl.abs() * (Bg.abs() * (F + c_g * Lam)).sum(1) + dl.abs() * esp * BL + c_g * (Dd * gg).abs() +
                        du.abs() * (1.0 + IO_HALF_ULP[io]) + ETA * (BL + N + 2))
                ref["du"][b, r0:r1], S["du"][b, r0:r1] = fl(du), fl(S_du)
                ax = a * _shift_right(x)
                pre = uu * sB + (An * ax * lam).sum(1)
                S_pre = (uu.abs() * (Bg.abs() * (F + c_g * Lam)).sum(1) +
                         (An.abs() * (aE * Lam + aX * F + c_g * aX * Lam)).sum(1))
                if softplus:
                    dd = pre * sig
                    S_dd = sig * S_pre + (esp + 15.0) * dd.abs()
                else:
                    dd, S_dd = pre, S_pre
                S_dd = S_dd + dd.abs() * (1.0 + IO_HALF_ULP[io]) + ETA * (pre.abs() + N + 2)
                ref["ddelta"][b, r0:r1], S["ddelta"][b, r0:r1] = fl(dd), fl(S_dd)
                if not (wrong == "dA_last_image" and b == batch - 1 and batch > 1):
                    tA = dl[:, None, :] * ax * lam
                    ref["dA"][r0:r1] += tA.sum(-1)
                    dlA = dl.abs()[:, None, :]
                    S["dA"][r0:r1] += (dlA * (aE * Lam + aX * F + (3.0 + esp[:, None, :]) * aX * Lam)).sum(-1) + ETA * L
                    sums["dA"][r0:r1] += (dlA * aX * Lam).sum(-1)
                keepB = slice(0, r1 - r0 - (1 if wrong == "dB_last_row" and r1 == (g + 1) * rows else 0))
                keepC = slice(0, r1 - r0 - (1 if wrong == "dC_last_row" and r1 == (g + 1) * rows else 0))
                dlu = (dl * uu)[:, None, :]
                ref["dB"][b, g] += fl((dlu * lam)[keepB].sum(0))
                S["dB"][b, g] += fl((dlu.abs() * (F + (c_g + esp[:, None, :]) * Lam)).sum(0)) + ETA * (r1 - r0)
                sums["dB"][b, g] += fl((dlu.abs() * Lam).sum(0))
                ref["dC"][b, g] += fl((gg[:, None, :] * x)[keepC].sum(0))
                S["dC"][b, g] += fl((gg.abs()[:, None, :] * (E + c_o * X)).sum(0)) + ETA * (r1 - r0)
                sums["dC"][b, g] += fl((gg.abs()[:, None, :] * X).sum(0))
                ref["dD"][r0:r1] += (gg * uu).sum(-1)
                sums["dD"][r0:r1] += (gg * uu).abs().sum(-1)
                ref["ddelta_bias"][r0:r1] += dd.sum(-1)
                S["ddelta_bias"][r0:r1] += S_dd.sum(-1)
                sums["ddelta_bias"][r0:r1] += dd.abs().sum(-1)
                del x, X, E, aE, aX, a, an, anL, lam, Lam, F, w, src, ax, kt, zA, under
    for name in sums:
        S[name] += _depth(cs, name) * sums[name] + ref[name].abs()
    rounded = ("out", "du", "ddelta") + (("dB", "dC") if io_bc else ())
    for name in ("dB", "dC") if io_bc else ():
        S[name] += IO_HALF_ULP[io] * ref[name].abs()
    if io == "float16":
        for name in rounded:
            S[name] += 2.0 ** -25 / U
    for name in OUTPUTS if finite else ():
        assert bool(torch.isfinite(ref[name]).all()) and bool(torch.isfinite(S[name]).all()), f"reference {name}: not finite"
    return ref, S, sums


def _depth(cs, name):
    return (cs.K_rows if name in ("dB", "dC") else cs.K_row) + 1.0


def rebound(S, sums, old: Constants, new: Constants):
    """the companions of the same problem under other depths of the deep sums (the deterministic form of a backward)"""
    assert (old.k, old.c_0, old.c, old.c_b) == (new.k, new.c_0, new.c, new.c_b)
    return {k: (v + (_depth(new, k) - _depth(old, k)) * sums[k] if k in sums else v) for k, v in S.items()}


def ratio(got, ref, S):
    """max |got - ref| / (U S) over EVERY element; a non-finite element of ``got`` gives inf"""
    got = got.detach().to(torch.float64).to(ref.device)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / (U * S + 1e-300)).max()) if got.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# value regimes: name -> generator(batch, KD, L, N, G, ush, seed, device, dtype) -> (u, delta, A, B, C, D, bias, dout,
# softplus); u / dout hold the rows of every 2^ush-th group.  Seeded; 16-bit-exact operands when dtype is a 16-bit type
# (u, delta, B, C, dout are rounded to it; A, D, bias stay fp32 as the operator takes them).

def _base(batch, KD, L, N, G, ush, seed, device, dtype):
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=device)
    q = lambda *s: torch.rand(*s, generator=g, device=device)
    t = dict(u=r(batch, KD >> ush, L), B=r(batch, G, N, L), C=r(batch, G, N, L), dout=r(batch, KD >> ush, L),
             D=1.0 + 0.1 * r(KD), A=-torch.arange(1, N + 1, dtype=torch.float32, device=device).repeat(KD, 1) * (1 + 0.05 * q(KD, N)))
    return t, r, q


def _finish(t, delta, bias, softplus, dtype):
    c = lambda v: v.to(dtype).contiguous()
    return (c(t["u"]), c(delta), t["A"].contiguous(), c(t["B"]), c(t["C"]), t["D"], bias, c(t["dout"]), softplus)


def _init(batch, KD, L, N, G, ush, seed, device, dtype, dt_lo=1e-3):
    """magnitudes of a freshly initialised SS2D block (_model_like of tests/test_scan_gpu.py): dt in [dt_lo, 0.1]"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    tgt = torch.exp(q(KD) * (math.log(0.1) - math.log(dt_lo)) + math.log(dt_lo))
    bias = tgt + torch.log(-torch.expm1(-tgt))
    return _finish(t, 0.5 * r(batch, KD, L), bias, True, dtype)


def _grid(batch, KD, L, N, G, ush, seed, device, dtype):
    """the reference unit test's distributions: A = -0.5 rand, delta = 0.5 rand, bias 0.5 rand, softplus on"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    t["A"] = -0.5 * q(KD, N)
    return _finish(t, 0.5 * q(batch, KD, L), 0.5 * q(KD), True, dtype)


def _large_dt(batch, KD, L, N, G, ush, seed, device, dtype):
    """raw + bias ~ N(2, 3), A = -(1..N): decays that underflow, memoryless fast states beside live slow ones"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    return _finish(t, 3.0 * r(batch, KD, L), torch.full((KD,), 2.0, device=device), True, dtype)


def _threshold(batch, KD, L, N, G, ush, seed, device, dtype):
    """raw + bias over [8, 25], with a block at 20 exactly, just below and just above (bias 0, so raw is what is stored),
    and a stretch just above 10 on which u = 0: there the output is what the decay leaves of the state, so that delta
    is seen through the exponent alone.  A ~ -0.3 on every state: |delta A| in 2.4 .. 7.5, about 3 on that stretch"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    d = 8.0 + 17.0 * q(batch, KD, L)
    n = min(L // 4, 48)
    edge = torch.tensor([20.0, 20.0 - 2.0 ** -19, 20.0 + 2.0 ** -19] if dtype == torch.float32 else [20.0, 19.875, 20.125], device=device)
    d[..., L // 2:L // 2 + n] = edge.repeat(n // 3 + 1)[:n]
    lo = L // 4
    d[..., lo:lo + n] = 10.0625 + 0.5 * q(batch, KD, n)
    t["u"][..., lo:lo + n] = 0.0
    t["A"] = -0.3 * (1 + 0.05 * q(KD, N))
    return _finish(t, d, torch.zeros(KD, device=device), True, dtype)


def _dead(batch, KD, L, N, G, ush, seed, device, dtype):
    """stretches with raw <= -90 (softplus denormal) and <= -110 (exactly zero in fp32) between live stretches: a whole
    160-position tile, the first and the last position of every second row"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    d = 0.5 * r(batch, KD, L) - 3.0
    if L >= 8:
        d[:, ::2, 0] = -95.0
        d[:, ::2, L - 1] = -112.0
    if L >= 640:
        d[:, :, 160:320] = -92.0                             # a whole 160-tile (ten 16-tiles), denormal
        d[:, :, 480:560] = -115.0                            # exactly zero
        d[:, 1::2, 330:340] = -100.0
    return _finish(t, d, torch.zeros(KD, device=device), True, dtype)


def _long_memory(batch, KD, L, N, G, ush, seed, device, dtype):
    """|A| ~ 1e-3, delta ~ 1e-2: every checkpoint, tile and segment hand-over carries the whole state"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    t["A"] = -1e-3 * (0.1 + q(KD, N))
    return _finish(t, 0.01 * q(batch, KD, L) + 1e-3, None, False, dtype)


def _neg_delta(batch, KD, L, N, G, ush, seed, device, dtype):
    """softplus off, delta in [-0.1, 0.3] (mean positive: the state stays bounded), no bias: decay factors above one"""
    t, r, q = _base(batch, KD, L, N, G, ush, seed, device, dtype)
    t["A"] = -0.5 * q(KD, N)
    return _finish(t, 0.4 * q(batch, KD, L) - 0.1, None, False, dtype)


def _sparse(batch, KD, L, N, G, ush, seed, device, dtype):
    """B, C or u zero on whole states, rows and stretches"""
    out = list(_init(batch, KD, L, N, G, ush, seed, device, dtype))
    u, B, C = out[0].clone(), out[3].clone(), out[4].clone()
    B[:, :, 0] = 0
    C[:, :, N - 1] = 0
    B[:, 0, :, L // 3:2 * L // 3] = 0
    C[:, -1, :, :L // 4] = 0
    u[:, ::3] = 0
    u[:, :, L // 2:L // 2 + 200] = 0
    out[0], out[3], out[4] = u, B, C
    return tuple(out)


REGIMES = {"init": _init, "grid": _grid, "large_dt": _large_dt, "threshold": _threshold, "dead": _dead,
           "long_memory": _long_memory, "neg_delta": _neg_delta, "sparse": _sparse}


def make(regime, batch, KD, L, N, G, ush=0, seed=0, device="cpu", dtype=torch.float32, **kw):
    return REGIMES[regime](batch, KD, L, N, G, ush, seed, device, dtype, **kw)
