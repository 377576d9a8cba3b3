"""Inputs, derived error bounds and an fp32 emulation of the distillation-loss kernels (csrc/distill.hip), shared by
tests/test_distill_loss_gpu.py (the kernels against the fp64 twin) and tests/test_distill_loss_cpu.py (the emulation against
the same bounds on the same inputs, and the wrong variants of the twin against them, so that the GPU test cannot pass
vacuously).  No GPU is needed to import or run anything here; ``bounds`` runs on whatever device its inputs are on.

Bounds, |got - ref| <= u S with u = 2^-24; every S below is computed from the fp64 twin, no number is fixed by hand.
C = classes; exp / log within 2 ulp; first order in u.  Precondition: fewer than 2^24 rows (the counts |S| and n are then
exact in fp32 at every stage).

1. Row errors (the family's, tests/loss_regimes.py and tests/region_loss_bounds.py).  z = v / T is formed as z^ = fl(v k^),
   k^ = fl(1 / T): two roundings, |z^_c - z_c| <= 2 u |z_c| (both vanish for T a power of two; the bound does not use that).
   lse is a softmax-weighted function of its arguments, so the scaled arguments move it by at most 2 u M(v), M(v) = sum_c
   w_c |z_c| with w = softmax(z); on top comes the register kernels' own error (C + 8) u (|l| + 1):
       E_l(v) = (C + 8) (|l| + 1) + 2 M(v)          for lse(x / T) and lse(t / T);        (C + 8) (|l| + 1) for lse(x).
   A log-probability a_c = fl(z^_c - l^):  e_a(c) = 2 |z_c| + E_l + |a_c|.  Its exponential adds the exp's 2 u and the
   rounding of the argument inside __expf, u |a_c| <= u (|z_c| + |l|); collecting terms (C >= 1):
       |w^_c - w_c| <= u r(c) w_c,    r(c) = (C + 11) (|z_c| + |l| + 1) + 2 M(v)
   -- the family's (C + 11) u (|x_c| + |l| + 1) p_c with the scaling term added.  P1 = exp(x_c - lse(x)) has no scaling
   term.  A -inf logit gives w = 0 exactly (r w = 0).
2. kl_r = sum_c [q_c > 0] q_c (a_c - b_c), a = log q, b = log p.  Per column: the error of q^, the errors of a^ and b^, the
   subtraction and the product; then the C terms are added, four to a chunk and the chunks in turn (at most C / 4 + 3 <= C + 1
   roundings on sum |term|).  A q_c below the smallest normal fp32 may be flushed to zero and its term dropped:
       E_kl(r) = sum_c [ r_q(c) q_c |a_c - b_c| + q_c (e_a(c) + e_b(c) + 2 |a_c - b_c|) ] + (C + 1) sum_c q_c |a_c - b_c|
                 + 2^-126 sum_c (1 + |a_c - b_c|) / u
   Columns with q_c = 0 contribute exactly 0 in the kernel and in the twin (bound 0).
   nll_r = l^ - x_y: (C + 9) (|l| + 1 + |x_y|), as tests/region_loss_bounds.py.
3. Summation, as tests/region_loss_bounds.py: the thread's running sum over its m = ceil(rows / (256 x 1024)) rows, the tree
   over the wave (6 levels), the four waves in order (3), all fp32: k_sum = m + 9 roundings on sum |v_r|; then 1024 slots in
   fp64 (not counted) and one rounding of what is stored.
       E_klsum = sum_S E_kl(r) + k_sum sum_S |kl_r|        E_nll = sum_valid (C + 9) (|l| + 1 + |x_y|) + k_sum sum nll
       kd = T^2 klsum / |S|:   E_kd = T^2 E_klsum / |S| + |kd|          ce:   E_ce = E_nll / n + |ce|
       loss:                   E_loss = kw T^2 E_klsum / |S| + cw E_nll / n + |loss|
       c0 = kw T / |S| and c1 = cw / n: exact in fp64, rounded once.
4. The gradient, fp32 per element, from the lse the forward kept: dx_c = G (dk + dc), dk = c0 (p_c - q_c) on S,
   dc = c1 (P1_c - [c = y]) on valid rows.  The subtraction, the rounded coefficient and the product are three roundings on
   each term; the sum, the product with G and G's own conversion to fp32 three on the total:
       E_dx(c) = |G| [ c0 (r_p p_c + r_q q_c) + 3 c0 |p_c - q_c| + c1 r_P1 P1_c + 3 c1 |P1_c - [c = y]| + 3 |dk + dc| ] + flush
   flush = 8 x 2^-126 (1 + |G|) (1 + c0 + c1) / u: an exponential or a product below the smallest normal fp32 may be flushed to
   zero.  Rows outside both sets and pad columns must be exact zeros (bound 0).
"""
from __future__ import annotations

import numpy as np
import torch

from tests.distill_loss_twin import is_valid, twin

IGNORE = 255
U = 2.0 ** -24
SIGMA_CE_BLOCKS = 1024
THREADS = 256 * SIGMA_CE_BLOCKS
# (classes, ld, ld_t) and the row counts of the issue; BIG_ROWS makes the grid-stride loop take a ragged second trip
CLASS_CASES = [(1, 4, 4), (3, 4, 8), (5, 8, 12), (9, 12, 12), (37, 40, 44), (40, 40, 44), (63, 64, 64), (64, 64, 68)]
ROW_COUNTS = [1, 255, 256, 257]
BIG_ROWS = THREADS + 257
BIG_CASE = (37, 40, 44)
# T, kw, cw, kd_all, upstream: every temperature of the issue, both kd_all values, cw = 0 and cw > 0, a non-unit upstream
PARAM_CASES = [(1.0, 1.0, 0.0, False, 1.0), (2.0, 0.7, 0.5, True, 0.37), (4.0, 1.5, 1.25, False, -2.5), (0.5, 1.0, 0.0, True, 1.0),
               (3.0, 0.0, 1.0, False, 1.0)]

# the value regimes: (rows, classes, ld, ld_t) -- 300 rows are two workgroups, one partly filled -- on the finite regimes of
# tests/loss_regimes.py without -inf, and the -inf regime with the mask in both tensors or in the teacher alone
REGIME_CASES = [(300, 9, 12, 12), (300, 40, 40, 44)]
UNMASKED_REGIMES = ("confident", "offset", "sweep", "ascending", "descending", "ties")
MASK_KINDS = ("both", "teacher")
REGIME_PARAMS = [(0.5, 1.0, 0.5, False, 1.0), (2.0, 1.0, 0.0, True, -2.5)]


def distill_inputs(rows, nc, ld, ld_t, seed):
    """CPU tensors: buf (rows, ld) and tbuf (rows, ld_t) fp32 with NaN in the pad, lab (rows,) int64.  Student N(0, 3^2); the
    teacher 0.7 x + N(0, 2^2): correlated, as a teacher is; ~10 % ignore_index, every 7th row a label inside the pad (ld >
    nc), every 11th a negative one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, nc, generator=g) * 3.0
    t = 0.7 * x + torch.randn(rows, nc, generator=g) * 2.0
    lab = torch.randint(0, nc, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.1] = IGNORE
    r = torch.arange(rows)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = 0
    return pad_to(x, ld), pad_to(t, ld_t), lab


def pad_to(x, ld):
    """(rows, ld) with x in the first columns and NaN behind them"""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=x.dtype)
    buf[:, :x.shape[1]] = x
    return buf


def regime_pair(regime, rows, nc, ld, ld_t, seed):
    """student and teacher buffers of one finite, unmasked regime of tests/loss_regimes.py (two seeds) and the student's labels"""
    from tests.loss_regimes import regime_inputs
    buf, lab = regime_inputs(regime, rows, nc, ld, seed)
    tbuf, _ = regime_inputs(regime, rows, nc, ld_t, seed + 1)
    return buf, tbuf, lab


def masked_pair(kind, rows, nc, ld, ld_t, seed):
    """the -inf regime: the mask of the "masked" regime of tests/loss_regimes.py (never the label's column of a valid row,
    never a whole row) applied to "both" tensors, to the "teacher" only, or to the "student" only (a +inf loss)"""
    from tests.loss_regimes import regime_inputs
    assert kind in ("both", "teacher", "student")
    mbuf, lab = regime_inputs("masked", rows, nc, ld, seed)
    mask = torch.isinf(mbuf[:, :nc])
    g = torch.Generator().manual_seed(seed + 100)
    fill = torch.randn(rows, nc, generator=g) * 3.0
    t = torch.randn(rows, nc, generator=g) * 3.0
    x = mbuf[:, :nc] if kind != "teacher" else torch.where(mask, fill, mbuf[:, :nc])
    if kind != "student":
        t = t.masked_fill(mask, float("-inf"))
    return pad_to(x, ld), pad_to(t, ld_t), lab


def k_sum(rows):
    return -(-rows // THREADS) + 9


def _fin_abs(z):
    return torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))          # -inf: the weight is 0 exactly


def bounds(x64, t64, lab, nc, T, kw, cw, kd_all, G):
    """The fp64 twin of the arguments plus the S (absolute bounds / u) of the module docstring: S_lse (rows, 3), S_kd, S_ce,
    S_loss, S_coef (2) and S_dl (rows, C)."""
    t = twin(x64, t64, lab, IGNORE, T, kw, cw, kd_all, upstream=G)
    rows = x64.shape[0]
    assert rows < 2 ** 24
    ks = k_sum(rows)
    valid, in_s = t["valid"], t["in_s"]
    vf, sf = valid.double()[:, None], in_s.double()[:, None]
    l1, lx, lt = t["lse"][:, 0:1], t["lse"][:, 1:2], t["lse"][:, 2:3]
    p, q, P1, oh = t["p"], t["q"], t["P1"], t["oh"]
    zx, zt, xa = _fin_abs(x64 / T), _fin_abs(t64 / T), _fin_abs(x64)
    Mx, Mt = (p * zx).sum(1, keepdim=True), (q * zt).sum(1, keepdim=True)
    El_1 = (nc + 8) * (l1.abs() + 1.0)
    El_x, El_t = (nc + 8) * (lx.abs() + 1.0) + 2.0 * Mx, (nc + 8) * (lt.abs() + 1.0) + 2.0 * Mt
    r_p = (nc + 11) * (zx + lx.abs() + 1.0) + 2.0 * Mx
    r_q = (nc + 11) * (zt + lt.abs() + 1.0) + 2.0 * Mt
    r_1 = (nc + 11) * (xa + l1.abs() + 1.0)
    live = q > 0
    z = torch.zeros_like(q)
    a, b = torch.where(live, t["lq"], z), torch.where(live, t["lp"], z)
    ab = (a - b).abs()
    e_a, e_b = 2.0 * zt + El_t + a.abs(), 2.0 * zx + El_x + b.abs()
    E_kl = (torch.where(live, r_q * q * ab + q * (e_a + e_b + 2.0 * ab), z).sum(1) + (nc + 1) * torch.where(live, q * ab, z).sum(1)
            + 2.0 ** -126 * torch.where(live, 1.0 + ab, z).sum(1) / U)
    E_klsum = float((E_kl * in_s.double()).sum()) + ks * float(t["klr"].abs().sum())
    xy = (xa * oh).sum(1)
    E_nll = float(((nc + 9) * (l1[:, 0].abs() + 1.0 + xy) * valid.double()).sum()) + ks * float(t["nll"].sum())
    ns, n = float(t["ns"]), float(t["n"])
    kd_err = T * T * E_klsum / ns if ns > 0 else 0.0
    ce_err = E_nll / n if n > 0 else 0.0
    c0, c1 = float(t["c0"]), float(t["c1"])
    dk, dc = c0 * (p - q) * sf, c1 * (P1 - oh) * vf
    flush = 8.0 * 2.0 ** -126 * (1.0 + abs(G)) * (1.0 + c0 + c1) / U
    S_dl = abs(G) * (sf * (c0 * (r_p * p + r_q * q) + 3.0 * c0 * (p - q).abs()) + vf * (c1 * r_1 * P1 + 3.0 * c1 * (P1 - oh).abs())
                     + 3.0 * (dk + dc).abs()) + flush
    t.update(S_lse=torch.cat([El_1, El_x, El_t], 1), S_kd=kd_err + abs(float(t["kd"])), S_ce=ce_err + abs(float(t["ce"])),
             S_loss=kw * kd_err + cw * ce_err + abs(float(t["loss"])), S_coef=torch.tensor([c0, c1], dtype=torch.float64),
             S_dl=torch.where((in_s | valid)[:, None], S_dl, torch.zeros_like(S_dl)))
    return t


def ratio(got, ref, S):
    """max |got - ref| / (u S) (0 / 0 counts as 0: an exact value held to the bound 0); NaN where got is not finite"""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    S = torch.as_tensor(S, dtype=torch.float64).to(ref.device)
    got = torch.as_tensor(got).to(device=ref.device, dtype=torch.float64)
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * S + 1e-300))
    return float(r.max()) if r.numel() else 0.0


def worst_ratio(out, t, nc):
    """the ratios of everything a forward + backward returns: out = dict(loss, terms (2), coef (2), lse (rows, 3), dl (rows, ld))"""
    terms, dl = torch.as_tensor(out["terms"]), torch.as_tensor(out["dl"])
    return dict(loss=ratio(out["loss"], t["loss"], t["S_loss"]), kd=ratio(terms[0], t["kd"], t["S_kd"]),
                ce=ratio(terms[1], t["ce"], t["S_ce"]), coef=ratio(out["coef"], torch.stack([t["c0"], t["c1"]]), t["S_coef"]),
                lse=ratio(out["lse"], t["lse"], t["S_lse"]), dl=ratio(dl[:, :nc], t["dl"], t["S_dl"]))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the three kernels, in numpy: the same order of operations and the same two-stage sum

F32 = np.float32


def _tree(v):
    """the wave's tree (wave_sum of csrc/scan_device.h): adjacent pairs, six levels, over axis -2 of (..., 64, cols)"""
    while v.shape[-2] > 1:
        v = v[..., 0::2, :] + v[..., 1::2, :]
    return v[..., 0, :]


def _chunked(v):
    """(rows, nc) -> (rows, NC4, 4) with -inf behind the classes, as mask_tail leaves the last chunk"""
    rows, nc = v.shape
    return np.concatenate([v, np.full((rows, (-nc) % 4), -np.inf, F32)], 1).reshape(rows, -1, 4)


def _row_lse(v4, k):
    """row_lse: the maximum of the scaled row, the exponentials added four to a chunk and the chunks in turn"""
    z = (v4 * k).astype(F32)
    m = z.max((1, 2))
    e = np.exp(z - m[:, None, None], dtype=F32)
    s = np.zeros(v4.shape[0], F32)
    for c in range(v4.shape[1]):
        s = s + ((e[:, c, 0] + e[:, c, 1]) + (e[:, c, 2] + e[:, c, 3]))
    return (m + np.log(s, dtype=F32)).astype(F32), z


def emulate_sums(x32, t32, lab, nc, T, kd_all):
    """distill_sums: (lse (rows, 3), partial (SIGMA_CE_BLOCKS, 4)) in fp32"""
    x4, t4 = _chunked(x32.numpy().astype(F32)), _chunked(t32.numpy().astype(F32))
    rows = x4.shape[0]
    y = lab.numpy()
    k = F32(1.0 / T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l1, _ = _row_lse(x4, F32(1.0))
        lx, zx = _row_lse(x4, k)
        lt, zt = _row_lse(t4, k)
        a, b = zt - lt[:, None, None], zx - lx[:, None, None]
        q = np.exp(a, dtype=F32)
        term = np.where(q > 0, q * (a - b), F32(0))
    kl = np.zeros(rows, F32)
    for c in range(x4.shape[1]):
        kl = kl + ((term[:, c, 0] + term[:, c, 1]) + (term[:, c, 2] + term[:, c, 3]))
    valid = (y != IGNORE) & (y >= 0) & (y < nc)
    in_s = np.ones_like(valid) if kd_all else valid
    safe = np.where(valid, y, 0)
    row = np.zeros((rows, 4), F32)                                                     # what a row adds to its thread
    row[:, 0] = np.where(in_s, kl, F32(0))
    row[:, 1] = in_s
    row[:, 2] = np.where(valid, l1 - np.take_along_axis(x4.reshape(rows, -1), safe[:, None], 1)[:, 0], F32(0))
    row[:, 3] = valid
    threads = min(rows, THREADS)
    blocks = -(-threads // 256)
    acc = np.zeros((blocks * 256, 4), F32)
    for trip in range(-(-rows // THREADS)):                                            # the thread's running sum, trip by trip
        part = row[trip * THREADS:(trip + 1) * THREADS]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    waves = _tree(acc.reshape(blocks, 4, 64, 4))
    partial = np.zeros((SIGMA_CE_BLOCKS, 4), F32)
    partial[:blocks] = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    return np.stack([l1, lx, lt], 1), partial


def emulate_coef(partial, T, kw, cw):
    """distill_coef: dict(loss, terms (2), coef (2)), fp64 inside, fp32 out"""
    q = partial.astype(np.float64).reshape(16, 16, 4, 4)          # group, run, slot of the run, column
    runs = np.zeros((16, 16, 4))
    for i in range(4):
        runs = runs + q[:, :, i]
    groups = np.zeros((16, 4))
    for i in range(16):
        groups = groups + runs[:, i]
    tot = np.zeros(4)
    for h in range(16):
        tot = tot + groups[h]
    S, n = tot[1], tot[3]
    with np.errstate(invalid="ignore"):
        kd = T * T * tot[0] / S if S > 0 else 0.0
        ce = tot[2] / n if n > 0 else 0.0
        loss = F32(kw * kd + cw * ce)
    return dict(loss=loss, terms=np.array([kd, ce], F32), coef=np.array([kw * T / S if S > 0 else 0.0, cw / n if n > 0 else 0.0], F32))


def emulate_bwd(x32, t32, lab, lse, coef, nc, ld, T, kd_all, G):
    """distill_bwd: dlogits (rows, ld) in fp32"""
    x, t = x32.numpy().astype(F32), t32.numpy().astype(F32)
    rows = x.shape[0]
    y = lab.numpy()
    valid = (y != IGNORE) & (y >= 0) & (y < nc)
    in_s = np.ones_like(valid) if kd_all else valid
    k, G = F32(1.0 / T), F32(G)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp((x * k).astype(F32) - lse[:, 1:2], dtype=F32)
        q = np.exp((t * k).astype(F32) - lse[:, 2:3], dtype=F32)
        p1 = np.exp(x - lse[:, 0:1], dtype=F32)
        hit = (np.where(valid, y, -1)[:, None] == np.arange(nc)[None, :]).astype(F32)
        dk = np.where(in_s[:, None], coef[0] * (p - q), F32(0))
        dc = np.where(valid[:, None], coef[1] * (p1 - hit), F32(0))
        d = G * (dk + dc)
    assert d.dtype == F32
    out = np.zeros((rows, ld), F32)
    out[:, :nc] = np.where(in_s[:, None], d, F32(0))
    return out


def emulate(buf32, tbuf32, lab, nc, T, kw, cw, kd_all, G):
    """the three kernels on buf32 (rows, ld) and tbuf32 (rows, ld_t) fp32: dict(loss, terms, coef, lse, dl)"""
    ld = buf32.shape[1]
    x32, t32 = buf32[:, :nc].contiguous(), tbuf32[:, :nc].contiguous()
    lse, partial = emulate_sums(x32, t32, lab, nc, T, kd_all)
    out = emulate_coef(partial, T, kw, cw)
    out.update(lse=lse, dl=emulate_bwd(x32, t32, lab, lse, out["coef"], nc, ld, T, kd_all, G))
    return out
