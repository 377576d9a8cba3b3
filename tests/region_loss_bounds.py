"""Inputs, derived error bounds and an fp32 emulation of the region-loss kernels (csrc/region.hip), shared by
tests/test_region_loss_gpu.py (the kernels against the fp64 twin) and tests/test_region_loss_cpu.py (the emulation against
the same bounds on the same inputs, and the wrong variants of the twin against them, so that the GPU test cannot pass
vacuously).  No GPU is needed to import or run anything here.

Bounds, |got - ref| <= u S with u = 2^-24; every S below is computed from the fp64 twin, no number is fixed by hand.
C = classes; l = lse; exp / log within 2 ulp.  Preconditions: fewer than 2^24 rows (the counts Y_c and n are then exact in
fp32 at every stage), and rho_c < 1 below (asserted).

1. Row error (the family's, tests/focal_bounds.py and tests/loss_regimes.py).  The forward forms l as the register kernels
   of pointwise.hip do: |l^ - l| <= (C + 8) u (|l| + 1).  p_c^ = exp(x_c - l^): one subtraction, the error of l^ and the
   exp give |p_c^ - p_c| <= e_p(r, c) = (C + 11) u (|x_c| + |l| + 1) p_c.  A -inf logit gives p = 0 exactly (e_p = 0).
   The row's nll^ = l^ - x_y: <= (C + 9) u (|l| + 1 + |x_y|).
2. Summation.  A sum of non-negative terms v_r over the rows is taken in two stages: the thread's running sum over its
   m = ceil(rows / (256 x 1024)) rows (m - 1 additions), the tree over the wave (6 levels) and the four waves in order (3),
   all fp32; then 1024 slots in fp64 (2^-53 per addition: below u^2 x 1024, not counted) and one rounding to fp32 of what is
   stored.  First order: k_sum = m + 9 roundings, error <= k_sum u sum v.  Hence
       E_P(c) = u [ (C + 11) sum_valid p_c (|x_c| + |l| + 1) + k_sum P_c ],   E_I(c) the same over the rows with y = c,
       E_nll  = u [ (C + 9) sum_valid (|l| + 1 + |x_y|) + k_sum sum nll ],    Y_c and n exact.
   `sums` is held to E_I, E_P and 0.
3. Propagation.  N = I + s, D = (1 - a - b) I + a P + b Y + s, so E_N = E_I and E_D = |1 - a - b| E_I + a E_P; let
   rho = E_D / D.  Every computed D^ lies in D [1 - rho, 1 + rho], so 1 / D^ <= 1 / (D (1 - rho)) and
   |1 / D^2 - 1 / D^^2| <= (2 + rho) rho / (D^2 (1 - rho)^2).  These are exact inequalities, not first-order ones: the
   coefficient table is formed in fp64, whose own rounding (a few 2^-53) is not counted.
       T = N / D:            E_T = (E_N + T E_D) / (D (1 - rho))
       region = mean of 1 - T over K:   E_region = (1 / |K|) sum_K E_T + u |region|             (the store rounds once)
       ce = sum nll / n:     E_ce = E_nll / n + u |ce|
       loss:                 E_loss = rw (E_region - u |region|) + cw (E_ce - u |ce|) + u |loss|
       W = D - (1 - a - b) N = a P + b Y + (a + b) s does not depend on I: E_W = a E_P.  With f = rw / |K|:
       A = -f W / D^2:       E_A = f [ E_W + W (2 + rho) rho ] / (D^2 (1 - rho)^2) + u |A|
       B = f a N / D^2:      E_B = f a [ E_N + N (2 + rho) rho ] / (D^2 (1 - rho)^2) + u |B|
       cwn = cw / n:         exact in fp64, rounded once: u cwn.
4. The gradient, fp32 per row: g_c = B_c + A_y [c = y] (one addition), dot = the sequential sum of p_c g_c over the C
   columns, dx_c = G (p_c (g_c - dot) + cwn (p_c - [c = y])).  First order in the roundings:
       E_g(c)  = E_B(c) + [c = y] E_A(y) + u |g_c|
       E_dot   = sum_c [ e_p |g_c| + p_c E_g(c) ] + (C + 1) u sum_c p_c |g_c|
       E_dx(c) = |G| [ e_p |g_c - dot| + p_c (E_g(c) + E_dot) + cwn e_p
                       + u (2 p_c |g_c - dot| + 3 cwn |p_c - [c = y]| + 2 |p_c (g_c - dot) + cwn (p_c - [c = y])|) ] + flush
   flush = 8 x 2^-126 (1 + |G|) (1 + cwn + |g_c - dot|): a product below the smallest normal fp32 may be flushed to zero.
   Rows that are not valid and pad columns must be exact zeros (bound 0).
"""
from __future__ import annotations

import numpy as np
import torch

from tests.region_loss_twin import is_valid, twin

IGNORE = 255
U = 2.0 ** -24
SIGMA_CE_BLOCKS = 1024
THREADS = 256 * SIGMA_CE_BLOCKS
# (classes, ld) and the row counts of the issue; the last row count makes the grid-stride loop take a ragged second trip
CLASS_CASES = [(5, 8), (9, 12), (37, 40), (40, 40), (64, 64)]
ROW_COUNTS = [1, 255, 256, 257]
BIG_ROWS = THREADS + 257
# kind / (a, b), s, rw, cw, upstream: every kind, s = 0 and s > 0, cw = 0 and cw > 0, a non-unit upstream gradient
PARAM_CASES = [("dice", 0.0, 1.0, 0.0, 1.0), ("jaccard", 1.0, 1.0, 0.5, 0.37), ((0.3, 0.7), 0.5, 0.8, 1.25, -2.5)]


def ab_of(kind):
    from tests.region_loss_twin import KINDS
    return KINDS[kind] if isinstance(kind, str) else kind


def region_inputs(rows, nc, ld, seed, absent=True, masked=True):
    """CPU tensors: buf (rows, ld) fp32 with NaN in the pad, lab (rows,) int64.  N(0, 3^2) logits; ~10 % ignore_index, every
    7th row a label inside the pad (ld > nc), every 11th a negative one; `absent`: class nc - 1 is never a label (nc > 2), so
    it is predicted and stays outside K; `masked`: every 5th row has one -inf logit away from its label (nc > 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, nc, generator=g) * 3.0
    hi = nc - 1 if (absent and nc > 2) else nc
    lab = torch.randint(0, hi, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.1] = IGNORE
    r = torch.arange(rows)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = 0
    if masked and nc > 1:
        valid = is_valid(lab, nc, IGNORE)
        col = (torch.where(valid, lab, torch.zeros_like(lab)) + 1 + r % (nc - 1)) % nc      # never the label's column
        hit = r % 5 == 2
        x[r[hit], col[hit]] = float("-inf")
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = x
    return buf, lab


def k_sum(rows):
    return -(-rows // THREADS) + 9


def bounds(x64, lab, nc, a, b, s, rw, cw, G):
    """The fp64 twin of the arguments plus the S (absolute bounds / u) of the module docstring: S_sums (3, C), S_region, S_ce,
    S_loss, S_coef (2 C + 1), S_lse (rows) and S_dl (rows, C)."""
    t = twin(x64, lab, IGNORE, a, b, s, rw, cw, upstream=G)
    rows = x64.shape[0]
    assert rows < 2 ** 24
    ks = k_sum(rows)
    l, sm, oh, valid = t["lse"], t["sm"], t["oh"], t["valid"]
    vf = valid.double()[:, None]
    I, P, Y = t["sums"]
    xa = torch.where(torch.isfinite(x64), x64.abs(), torch.zeros_like(x64))          # -inf: p = 0 exactly
    e_p = (nc + 11) * (xa + l.abs()[:, None] + 1.0) * sm                             # / u
    E_P = (e_p * vf).sum(0) + ks * P
    E_I = (e_p * oh).sum(0) + ks * I
    xy = (xa * oh).sum(1)
    nll_sum = float(t["ce"] * t["n"])
    E_nll = float(((nc + 9) * (l.abs() + 1.0 + xy) * valid.double()).sum()) + ks * nll_sum
    present = Y > 0
    k = max(int(t["kcount"]), 1)
    D = torch.where(present, t["D"], torch.ones_like(P))
    N, T = t["N"], t["T"]
    E_N, E_D = E_I, abs(1.0 - a - b) * E_I + a * E_P
    rho = U * E_D / D
    assert bool((rho[present] < 1.0).all())
    z = torch.zeros_like(P)
    E_T = torch.where(present, (E_N + T * E_D) / (D * (1.0 - rho)), z)
    S_region = float(E_T.sum()) / k + abs(float(t["region"]))
    n = float(t["n"])
    S_ce = (E_nll / n if n > 0 else 0.0) + abs(float(t["ce"]))
    S_loss = rw * float(E_T.sum()) / k + cw * (E_nll / n if n > 0 else 0.0) + abs(float(t["loss"]))
    f = rw / k
    W = a * P + b * Y + (a + b) * s
    den = D * D * (1.0 - rho) ** 2
    E_A = torch.where(present, f * (a * E_P + W * (2.0 + rho) * E_D / D) / den + t["A"].abs(), z)
    E_B = torch.where(present, f * a * (E_N + N * (2.0 + rho) * E_D / D) / den + t["B"].abs(), z)
    cwn = float(t["cwn"])
    g, dot = t["g"], t["dot"][:, None]
    E_g = (E_B[None, :] + oh * E_A[None, :] + g.abs()) * vf
    E_dot = (e_p * g.abs() + sm * E_g).sum(1, keepdim=True) + (nc + 1) * (sm * g.abs()).sum(1, keepdim=True)
    t1, t2 = sm * (g - dot), cwn * (sm - oh)
    flush = 8.0 * 2.0 ** -126 * (1.0 + abs(G)) * (1.0 + cwn + (g - dot).abs()) / U
    S_dl = abs(G) * (e_p * (g - dot).abs() + sm * (E_g + E_dot) + cwn * e_p
                     + 2.0 * t1.abs() + 3.0 * t2.abs() + 2.0 * (t1 + t2).abs()) + flush
    t.update(S_sums=torch.stack([E_I, E_P, z]), S_region=S_region, S_ce=S_ce, S_loss=S_loss,
             S_coef=torch.cat([E_A, E_B, torch.tensor([cwn])]), S_lse=(nc + 8) * (l.abs() + 1.0),
             S_dl=torch.where(valid[:, None], S_dl, torch.zeros_like(S_dl)))
    return t


def ratio(got, ref, S):
    """max |got - ref| / (u S) (0 / 0 counts as 0: an exact value held to the bound 0); NaN where got is not finite"""
    got = torch.as_tensor(got, dtype=torch.float64)
    ref, S = torch.as_tensor(ref, dtype=torch.float64), torch.as_tensor(S, dtype=torch.float64)
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * S + 1e-300))
    return float(r.max()) if r.numel() else 0.0


def worst_ratio(out, t, nc):
    """the largest ratio over everything a forward + backward returns: out = dict(loss, terms (2), sums (3, C), dl (rows, ld))"""
    dl = torch.as_tensor(out["dl"])
    rs = dict(loss=ratio(out["loss"], t["loss"], t["S_loss"]),
              region=ratio(torch.as_tensor(out["terms"])[0], t["region"], t["S_region"]),
              ce=ratio(torch.as_tensor(out["terms"])[1], t["ce"], t["S_ce"]),
              sums=ratio(out["sums"], t["sums"], t["S_sums"]),
              dl=ratio(dl[:, :nc], t["dl"], t["S_dl"]))
    return rs


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the three kernels, in numpy: the same order of operations and the same two-stage sum

F32 = np.float32


def _tree(v):
    """the wave's tree (wave_sum of csrc/scan_device.h): adjacent pairs, six levels, over axis -2 of (..., 64, cols)"""
    while v.shape[-2] > 1:
        v = v[..., 0::2, :] + v[..., 1::2, :]
    return v[..., 0, :]


def emulate_sums(x32, lab, nc):
    """region_sums: (lse (rows,), partial (SIGMA_CE_BLOCKS, 3 nc + 2)) in fp32"""
    x = x32.numpy().astype(F32)
    rows = x.shape[0]
    y = lab.numpy()
    m = x.max(1)
    e = np.exp(x - m[:, None], dtype=F32)
    pad = (-nc) % 4
    e4 = np.concatenate([e, np.zeros((rows, pad), F32)], 1).reshape(rows, -1, 4)      # exp(-inf - m) = 0 in the pad
    s = np.zeros(rows, F32)
    for c in range(e4.shape[1]):
        s = s + ((e4[:, c, 0] + e4[:, c, 1]) + (e4[:, c, 2] + e4[:, c, 3]))
    l = (m + np.log(s, dtype=F32)).astype(F32)
    valid = (y != IGNORE) & (y >= 0) & (y < nc)
    safe = np.where(valid, y, 0)
    p = np.exp(x - l[:, None], dtype=F32)
    hit = (safe[:, None] == np.arange(nc)[None, :]) & valid[:, None]
    ncol = 3 * nc + 2
    row = np.zeros((rows, ncol), F32)                                                  # what a valid row adds to its thread
    row[:, :nc] = np.where(hit, p, F32(0))
    row[:, nc:2 * nc] = p
    row[:, 2 * nc:3 * nc] = hit.astype(F32)
    row[:, 3 * nc] = l - np.take_along_axis(x, safe[:, None], 1)[:, 0]
    row[:, 3 * nc + 1] = 1.0
    row[~valid] = 0.0
    threads = min(rows, THREADS)
    blocks = -(-threads // 256)
    acc = np.zeros((blocks * 256, ncol), F32)
    for trip in range(-(-rows // THREADS)):                                            # the thread's running sum, trip by trip
        part = row[trip * THREADS:(trip + 1) * THREADS]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    waves = _tree(acc.reshape(blocks, 4, 64, ncol))
    partial = np.zeros((SIGMA_CE_BLOCKS, ncol), F32)
    partial[:blocks] = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    return l, partial


def emulate_coef(partial, nc, a, b, s, rw, cw):
    """region_coef: dict(loss, terms (2), coef (2 nc + 1), sums (3, nc)), fp64 inside, fp32 out"""
    ncol = 3 * nc + 2
    cols = 8
    while cols < ncol:
        cols <<= 1
    parts = 1024 // cols
    per = SIGMA_CE_BLOCKS // parts
    q = partial.astype(np.float64).reshape(parts, per, ncol)
    runs = np.zeros((parts, ncol))
    for k in range(per):
        runs = runs + q[:, k]
    tot = np.zeros(ncol)
    for i in range(parts):
        tot = tot + runs[i]
    I, P, Y = tot[:nc], tot[nc:2 * nc], tot[2 * nc:3 * nc]
    present = Y > 0
    N = np.where(present, I + s, 0.0)
    D = np.where(present, (1.0 - a - b) * I + a * P + b * Y + s, 1.0)
    miss = np.where(present, 1.0 - N / D, 0.0)
    k = int(present.sum())
    f = np.where(present, rw / max(k, 1), 0.0)
    A = np.where(present, -f * (D - (1.0 - a - b) * N) / (D * D), 0.0)
    B = np.where(present, f * a * N / (D * D), 0.0)
    region = 0.0
    for v in miss:
        region += v
    region = region / k if k > 0 else 0.0
    n = tot[3 * nc + 1]
    ce = tot[3 * nc] / n if n > 0 else 0.0
    coef = np.concatenate([A, B, [cw / n if n > 0 else 0.0]]).astype(F32)
    return dict(loss=F32(rw * region + cw * ce), terms=np.array([region, ce], F32), coef=coef,
                sums=np.stack([I, P, Y]).astype(F32))


def emulate_bwd(x32, lab, l, coef, nc, ld, G):
    """region_bwd: dlogits (rows, ld) in fp32"""
    x = x32.numpy().astype(F32)
    rows = x.shape[0]
    y = lab.numpy()
    valid = (y != IGNORE) & (y >= 0) & (y < nc)
    safe = np.where(valid, y, 0)
    G, cw = F32(G), coef[2 * nc]
    ay = coef[safe]
    p = np.exp(x - l[:, None], dtype=F32)
    hit = safe[:, None] == np.arange(nc)[None, :]
    g = (coef[nc:2 * nc][None, :] + np.where(hit, ay[:, None], F32(0))).astype(F32)
    dot = np.zeros(rows, F32)
    for c in range(nc):
        dot = dot + p[:, c] * g[:, c]
    d = G * (p * (g - dot[:, None]) + cw * (p - hit.astype(F32)))
    assert d.dtype == F32
    out = np.zeros((rows, ld), F32)
    out[:, :nc] = np.where(valid[:, None], d, F32(0))
    return out


def emulate(buf32, lab, nc, a, b, s, rw, cw, G):
    """the three kernels on buf32 (rows, ld) fp32: dict(loss, terms, sums, coef, lse, dl)"""
    ld = buf32.shape[1]
    x32 = buf32[:, :nc].contiguous()
    l, partial = emulate_sums(x32, lab, nc)
    out = emulate_coef(partial, nc, a, b, s, rw, cw)
    out.update(lse=l, dl=emulate_bwd(x32, lab, l, out["coef"], nc, ld, G))
    return out
