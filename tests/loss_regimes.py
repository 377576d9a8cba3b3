"""Named value regimes for the loss family (csrc/pointwise.hip: plain, option and focal cross entropy, the register and the
walking kernels; csrc/deepsup.hip and the OHEM route on top), fp64 restatements that survive -inf logits, an fp32 emulation
of the plain and option kernels in both forms, and the wrong variants that each regime must reject.  Shared by
tests/test_loss_regimes_cpu.py (the emulation under the bounds, so that the GPU tests cannot pass vacuously) and
tests/test_loss_regimes_gpu.py (the kernels).  No GPU is needed to import or run anything here.

Every other test of the family draws its logits from N(0, 3^2).  There the running maximum of a walk almost never rises
after the first chunks, no exponent comes near +-88, the largest logit never sits in the last valid column of a padded
tail, p_y never rounds to 1 and nothing is infinite.  The regimes (``regime_inputs``), all on top of x = 3 randn with the
labels of tests/test_head_classes_gpu._labels (~10 % ignore_index, every 7th row a label inside the pad, every 11th a
negative one; "valid": 0 <= y < nc and y != ignore_index):

confident   valid rows: x_y += 16, 17, 18, 30, 90, 150, 1000 in turn (16 - 18: p_y rounds to 1 in fp32; above, lse == x_y
            and the other classes' products go subnormal, then zero); every fourth valid row x_y -= 30, 90, 1000 instead
            (confident and wrong: nll ~ the margin, exp(x_y - lse) underflows).
offset      a per-row constant of +-1e2, +-1e3, +-1e4, +-3e4 on the whole row: exp without the max overflows, lse - x_y
            cancels at 1e4.
sweep       row r: x[r mod nc] += 60 -- the largest logit visits every column, the last valid one of a masked tail chunk
            and every position of the label pick included.
ascending   30 randn, every row sorted: the maximum rises in every chunk of a walk (ceil(nc / 4) rescales).
descending  the same rows sorted the other way: no rescale after the first chunk, most exponents underflow.
ties        whole rows equal to one of 0, -0.0, 1, -1e4, 3e4, 1e-42 (subnormal): lse = v + log C; rows with two and with
            four columns tied at the maximum.
masked      -inf (a masked class) in (a) columns 0 - 3, (b) the last full chunk, (c) every column but the label's and one
            other, (d) a random 30 % of the columns; the label's column of a valid row is never masked and no row is masked
            whole.  (a) and (b) need nc >= 5; nc == 1 has no such regime.
nonfinite   the base rows with twelve poisoned rows among the first 256, six with a valid label and six ignored, one of
            each kind: NaN in column 0, NaN in the last valid column, +inf in one column, +inf in two, all -inf, -inf at
            the label's own column (``NONFINITE_KINDS``).

Bounds.  The existing ones, unchanged, applied with ``check`` / ``rejects`` of tests/test_stream_fp64_gpu.py (|got - ref| <=
K u S, u = 2^-24): lse K = C + 8 on |l| + 1; the plain kernels' loss sum and dlogits (C + 16) of
tests/test_head_classes_gpu.py; the option kernels' row (2C + 16), dlogits (2C + 24) and sums of
tests/test_loss_options_gpu.py (restated in ``opt_ref``: its ``_ref`` needs a device, and forms 0 * inf at a masked column);
tests/focal_bounds.bounds; tests/deepsup_bounds.bounds.  Their S carry |x| + |l| + 1, which covers the argument error of
__expf at large |x - l|.  At a masked column every S is zero: p_c = exp(-inf) is exactly 0 and so is the gradient.

Two additions:

Underflow term (``underflow_S``; the regimes that make products subnormal -- ``confident``, ``descending`` and ``ascending``,
which holds the rows of ``descending`` in the other order -- plain and option dlogits alone).  A term f p_c of
the gradient, f = |g| (plain) or |g| ((1 - eps) w_y + (eps / C) W) (option), has p_c = exp(x_c - l) as small as e^-1000.
Relative bounds say nothing below fp32's normal range: an exp result below 2^-126 may come back subnormal (absolute error
<= 2^-150) or flushed to zero (error < 2^-126), and so may the product f p_c.  Both together are below
2^-126 (1 + f) <= 2^-125 (1 + f); divided by K u it joins S, the term tests/focal_bounds.py already carries.

Sharper lse bound on ``offset`` (``lse_offset_bound``).  (C + 8) u (|l| + 1) is 0.045 at |l| = 1e4 and tests nothing.
There m = max_c x_c is an input, exact, and l = m + log s with s = sum_c exp(x_c - m) in [1, C].  The subtractions x_c - m are
exact or round on |x_c - m| <= ~40, which exp turns into a relative error d e^-d u <= u / e of a term; each term carries the
exp's 2 u, the sum at most C / 4 + 3 u (pairs, then the chunks in turn), a rescale of the walk the same as a term.  So
s^ = s (1 + theta), |theta| <= (C + 4) u, and log s^ = log s + theta, with the log's own 2 u (log s + 1) on top: the
constant C + 8 of the existing bound, now acting on the magnitude of log s <= log C.  The final add m + log s rounds once
on |l|:
    |l^ - l| <= u |l| + (C + 8) u (log C + 1).
The GPU tests assert it in addition to the existing bound, the CPU test confirms that the emulation stays under it.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

IGNORE = 255
U = 2.0 ** -24
NEG_INF = float("-inf")
REGIMES = ("confident", "offset", "sweep", "ascending", "descending", "ties", "masked", "nonfinite")
FINITE_REGIMES = REGIMES[:-1]
SUBNORMAL_REGIMES = ("confident", "ascending", "descending")      # where the plain and option S_dl get the underflow term
NONFINITE_KINDS = ("nan_first", "nan_last", "inf_one", "inf_two", "all_neg_inf", "neg_inf_label")
# (rows, classes, pitch): 300 rows are two workgroups, one partly filled.  Up to 64 classes the row is held in registers,
# above it is walked; (300, 130, 132) walks 33 chunks.
REG_CASES = [(300, 2, 4), (300, 9, 12), (300, 5, 16), (300, 40, 40), (300, 63, 64), (300, 64, 64)]
WALK_CASES = [(300, 65, 68), (300, 67, 68), (300, 68, 68), (300, 130, 132)]
CASES = REG_CASES + WALK_CASES
CASE_IDS = [f"{r}x{c}@{l}" for r, c, l in CASES]
# (class weights?, label smoothing) of the option kernels
OPTS = [(True, 0.0), (False, 0.1), (True, 0.1)]
OPT_IDS = ["w", "eps", "w+eps"]
GAMMAS = (0.0, 1.0, 2.0, 3.5)
# rows of the nonfinite regime: one per kind and set, all inside workgroup 0
POISON_VALID = (10, 50, 90, 130, 170, 210)
POISON_IGNORED = (20, 60, 100, 140, 180, 220)


def form_of(nc):
    """the kernel form the host picks: registers up to 64 classes, the walk above"""
    return "reg" if nc <= 64 else "walk"


def is_valid(lab, nc):
    return (lab != IGNORE) & (lab >= 0) & (lab < nc)


def _labels(rows, nc, ld, g):
    lab = torch.randint(0, nc, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.1] = IGNORE
    r = torch.arange(rows)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = nc - 1
    return lab


def weights(nc, seed):
    """fp32 class weights in [0.1, 2.1], class nc // 2 with an exact zero (not where there is one class only)"""
    w = torch.rand(nc, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.1
    if nc > 1:
        w[nc // 2] = 0.0
    return w


def has_regime(regime, nc):
    return not (regime == "masked" and nc == 1)


def regime_inputs(regime, rows, nc, ld, seed, poison=("valid", "ignored")):
    """CPU tensors (buf, lab): buf (rows, ld) fp32 with NaN behind the classes, lab (rows,) int64.  ``nonfinite`` returns
    (buf, lab, base, poisoned): base is buf before the poison, poisoned maps "valid" / "ignored" to the row indices of the
    set (in the order of NONFINITE_KINDS; empty for a set ``poison`` leaves out -- the labels are the same either way)."""
    assert regime in REGIMES and has_regime(regime, nc)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, nc, generator=g) * 3.0
    lab = _labels(rows, nc, ld, g)
    r = torch.arange(rows)
    poisoned = None
    if regime == "nonfinite":
        assert rows > max(POISON_VALID + POISON_IGNORED) and nc >= 2
        lab[list(POISON_VALID)] = 0                      # class 0 never has the zero weight (that is class nc // 2 >= 1)
        lab[list(POISON_IGNORED)] = IGNORE
    valid = is_valid(lab, nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    k = torch.cumsum(valid.long(), 0) - 1                # the index of a valid row among the valid rows
    if regime == "confident":
        up = torch.tensor([16.0, 17.0, 18.0, 30.0, 90.0, 150.0, 1000.0])[k % 7]
        down = torch.tensor([30.0, 90.0, 1000.0])[(k // 4) % 3]
        wrong = valid & (k % 4 == 3)
        x[r, safe] += torch.where(wrong, -down, up) * valid.float()
    elif regime == "offset":
        x += torch.tensor([1e2, -1e2, 1e3, -1e3, 1e4, -1e4, 3e4, -3e4])[r % 8][:, None]
    elif regime == "sweep":
        x[r, r % nc] += 60.0
    elif regime in ("ascending", "descending"):
        x = torch.sort(x * 10.0, dim=1, descending=regime == "descending").values
    elif regime == "ties":
        vals = torch.tensor([0.0, -0.0, 1.0, -1e4, 3e4, 1e-42])
        assert float(vals[5]) != 0.0                     # the subnormal survived
        whole = r % 4 == 0
        x = torch.where(whole[:, None], vals[(r // 4) % 6][:, None].expand(rows, nc), x)
        top = x.max(1).values + 1.0
        for n_tied, sel in ((2, r % 4 == 1), (4, r % 4 == 2)):
            for j in range(n_tied):
                col = (r + j * max(1, nc // 4)) % nc
                x[r[sel], col[sel]] = top[sel]
    elif regime == "masked":
        mask = torch.zeros(rows, nc, dtype=torch.bool)
        kinds = "abcd" if nc >= 5 else "cd"
        kind = r % len(kinds)
        rnd = torch.rand(rows, nc, generator=g) < 0.3
        cols = torch.arange(nc)[None, :]
        for i, name in enumerate(kinds):
            sel = (kind == i)[:, None]
            if name == "a":
                mask |= sel & (cols < 4)
            elif name == "b":
                c0 = 4 * (nc // 4 - 1)
                mask |= sel & (cols >= c0) & (cols < c0 + 4)
            elif name == "c":
                other = (safe + 1 + r % (nc - 1)) % nc
                mask |= sel & (cols != safe[:, None]) & (cols != other[:, None])
            else:
                mask |= sel & rnd
        mask[r, safe] = mask[r, safe] & ~valid           # the label's column of a valid row is never masked
        mask[mask.all(1), nc - 1] = False                # no row is masked whole
        x = x.masked_fill(mask, NEG_INF)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = x
    if regime != "nonfinite":
        return buf, lab
    base = buf.clone()
    nan, inf = float("nan"), float("inf")
    poisoned = {"valid": torch.tensor(POISON_VALID if "valid" in poison else (), dtype=torch.long),
                "ignored": torch.tensor(POISON_IGNORED if "ignored" in poison else (), dtype=torch.long)}
    for name in ("valid", "ignored"):
        for kind, row in zip(NONFINITE_KINDS, poisoned[name].tolist()):
            if kind == "nan_first":
                buf[row, 0] = nan
            elif kind == "nan_last":
                buf[row, nc - 1] = nan
            elif kind == "inf_one":
                buf[row, nc // 2] = inf
            elif kind == "inf_two":
                buf[row, 0] = buf[row, nc - 1] = inf
            elif kind == "all_neg_inf":
                buf[row, :nc] = NEG_INF
            else:
                buf[row, 0] = NEG_INF                     # the label of a row of the valid set is 0
    return buf, lab, base, poisoned


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references on any device; -inf logits allowed (a masked column has p = 0 and S = 0)

def _pmag(p, x, l):
    """p_c (|x_c| + |l| + 1), zero at a masked column (where it would be 0 * inf)"""
    return torch.where(torch.isinf(x) & (p == 0), torch.zeros_like(p), p * (x.abs().clamp_max(1e300) + l.abs()[:, None] + 1.0))


def _rowvec(g, rows, like):
    return g.double().to(like.device) if torch.is_tensor(g) else torch.full((rows,), float(g), device=like.device, dtype=torch.float64)


def plain_ref(x, lab, nc, sc):
    """fp64 of the plain kernels (``_ce_ref`` of tests/test_head_classes_gpu.py): validity, lse and S_lse, the row losses
    and their S, dlogits = sc (softmax - onehot) on valid rows and S_dl, and f = |sc| per valid row"""
    rows = x.shape[0]
    valid = is_valid(lab, nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    lse = torch.logsumexp(x, 1)
    xl = x.gather(1, safe[:, None])[:, 0]
    p = torch.softmax(x, 1)
    oh = F.one_hot(safe, nc).double()
    zero, zeros = torch.zeros_like(lse), torch.zeros_like(p)
    gr = _rowvec(sc, rows, x)[:, None]
    dl = torch.where(valid[:, None], gr * (p - oh), zeros)
    S_dl = torch.where(valid[:, None], gr.abs() * (_pmag(p, x, lse) + oh), zeros)
    S_lse = lse.abs() + 1.0
    return dict(valid=valid, lse=lse, S_lse=S_lse, row=torch.where(valid, lse - xl, zero), S_row=torch.where(valid, S_lse + xl.abs(), zero),
                wy=valid.double(), dl=dl, S_dl=S_dl, f=torch.where(valid, gr[:, 0].abs(), zero))


def opt_ref(x, lab, nc, w, eps, g):
    """fp64 of the option kernels, the formulas and S of ``_ref`` of tests/test_loss_options_gpu.py.  The smoothing terms
    are formed only for eps > 0 (0 * inf otherwise at a masked column).  f = |g| ((1 - eps) w_y + (eps / C) W)."""
    rows = x.shape[0]
    valid = is_valid(lab, nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    w64 = w.double().to(x.device) if w is not None else torch.ones(nc, device=x.device, dtype=torch.float64)
    W = w64.sum()
    lse = torch.logsumexp(x, 1)
    xl = x.gather(1, safe[:, None])[:, 0]
    p = torch.softmax(x, 1)
    oh = F.one_hot(safe, nc).double()
    zero, zeros = torch.zeros_like(lse), torch.zeros_like(p)
    wy = torch.where(valid, w64[safe], zero)
    a, b = (1.0 - eps) * wy, eps / nc
    S_lse = lse.abs() + 1.0
    row, S_row = a * (lse - xl), a * (S_lse + xl.abs())
    gr = _rowvec(g, rows, x)[:, None]
    dl = gr * a[:, None] * (p - oh)
    coef = a[:, None]
    S_dl = a[:, None] * oh
    if eps > 0:
        row = row + b * (W * lse - (w64 * x).sum(1))
        S_row = S_row + b * (W * S_lse + (w64 * x.abs()).sum(1))
        dl = dl + gr * b * (W * p - w64[None, :])
        coef = coef + b * W
        S_dl = S_dl + b * w64[None, :]
    S_dl = gr.abs() * (coef * _pmag(p, x, lse) + S_dl)
    return dict(valid=valid, lse=lse, S_lse=S_lse, row=torch.where(valid, row, zero), S_row=torch.where(valid, S_row, zero), wy=wy,
                dl=torch.where(valid[:, None], dl, zeros), S_dl=torch.where(valid[:, None], S_dl, zeros),
                f=torch.where(valid, (gr * coef)[:, 0].abs(), zero))


def focal_ref(x, lab, nc, w, gamma, g):
    """tests/focal_bounds.bounds, with S_dl zero at a masked column (its p_c |x_c| is 0 * inf there) and S_row zero at an
    ignored row whose column 0 is masked (0 * inf as well)"""
    from tests import focal_bounds
    t = focal_bounds.bounds(x, lab, nc, w, gamma, g)
    t["S_row"] = torch.where(t["valid"], t["S_row"], torch.zeros_like(t["S_row"]))
    t["S_dl"] = torch.where(torch.isinf(x) & (t["sm"] == 0), torch.zeros_like(t["S_dl"]), t["S_dl"])
    return t


def underflow_S(f, K):
    """(rows, 1): 2^-125 (1 + f) / (K u), the term of the module docstring that the plain and option S_dl get on the regimes
    of SUBNORMAL_REGIMES; zero at rows with f = 0 (ignored rows: exact zeros are asked for)"""
    return torch.where(f > 0, 2.0 ** -125 * (1.0 + f) / (K * U), torch.zeros_like(f))[:, None]


def lse_offset_bound(lse, nc):
    """the absolute bound on lse of the ``offset`` regime (module docstring)"""
    return U * lse.abs() + (nc + 8) * U * (math.log(nc) + 1.0)


def ratio(got, ref, S, K):
    """max |got - ref| / (K u S), as ``_ratio`` of tests/test_stream_fp64_gpu.py; NaN where got is not finite"""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - ref).abs() / (K * U * S + 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels (csrc/pointwise.hip), chunk by chunk

VARIANTS = ("no_max", "no_rescale", "first_chunk")


def _chunks(x32):
    """the row as the kernels read it: chunks of four columns, -inf over the tail of the last one"""
    rows, nc = x32.shape
    out = []
    for c in range(0, nc, 4):
        v = x32[:, c:c + 4]
        if v.shape[1] < 4:
            v = torch.cat([v, torch.full((rows, 4 - v.shape[1]), NEG_INF)], 1)
        out.append(v)
    return out


def _fmax4(v):
    return torch.fmax(torch.fmax(v[:, 0], v[:, 1]), torch.fmax(v[:, 2], v[:, 3]))       # fmaxf: a NaN operand is dropped


def _exp_sum4(v, m):
    e = torch.exp(v - m[:, None])
    return (e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])


def lse_fp32(x32, form="reg", variant=None):
    """lse as the forward kernels form it.  form "reg": the maximum of the whole row first (softmax_ce_fwd_reg_kernel);
    "walk": chunks of four with the online rescale, the exponents taken against 0 while the maximum is still -inf
    (softmax_ce_fwd_kernel).  The wrong variants: "no_max" exponentiates without subtracting a maximum; "no_rescale" walks
    without s *= exp(m - vm); "first_chunk" is the walk before the fix, exp(v - m) with m = -inf."""
    assert x32.dtype == torch.float32 and form in ("reg", "walk") and variant in (None,) + VARIANTS
    rows = x32.shape[0]
    chunks = _chunks(x32)
    s = torch.zeros(rows)
    m = torch.full((rows,), NEG_INF)
    if variant == "no_max":
        for v in chunks:
            s = s + _exp_sum4(v, torch.zeros(rows))
        return torch.log(s)
    if form == "reg":
        for v in chunks:
            m = torch.fmax(m, _fmax4(v))
        for v in chunks:
            s = s + _exp_sum4(v, m)
        return m + torch.log(s)
    for v in chunks:
        vm = _fmax4(v)
        up = vm > m
        if variant != "no_rescale":
            s = torch.where(up, s * torch.exp(m - vm), s)
        m = torch.where(up, vm, m)
        mz = m if variant == "first_chunk" else torch.where(m > NEG_INF, m, torch.zeros_like(m))
        s = s + _exp_sum4(v, mz)
    return m + torch.log(s)


def emulate_ce_fp32(x32, lab, nc, w, eps, g, form, variant=None, kind="opt"):
    """The plain (kind "plain": w and eps are not read) and option kernels step by step in fp32 torch ops: lse, row_loss,
    w_y and dlogits for the per-row upstream g (a float or (rows,))."""
    f32 = torch.float32
    rows = x32.shape[0]
    valid = is_valid(lab, nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    l = lse_fp32(x32, form, variant)
    xy = x32.gather(1, safe[:, None])[:, 0]
    oh = F.one_hot(safe, nc).to(f32)
    zero = torch.zeros(rows)
    gr = g.to(f32) if torch.is_tensor(g) else torch.full((rows,), float(g), dtype=f32)
    gr = torch.where(valid, gr, zero)
    p = torch.exp(x32 - l[:, None])
    if kind == "plain":
        row, wy = torch.where(valid, l - xy, zero), valid.to(f32)
        dl = (p - oh) * gr[:, None]
    else:
        wv = w.to(f32) if w is not None else torch.ones(nc, dtype=f32)
        W = torch.tensor(float(nc), dtype=f32)
        if w is not None:
            W = torch.zeros((), dtype=f32)
            for c in range(nc):
                W = W + wv[c]
        e = torch.tensor(eps, dtype=f32)
        inv_c = torch.tensor(1.0, dtype=f32) / torch.tensor(float(nc), dtype=f32)
        wy = torch.where(valid, wv[safe], zero)
        a = (1.0 - e) * wy
        row = a * (l - xy)
        if eps > 0:
            sx = torch.zeros(rows)
            for c in range(0, nc, 4):
                t = wv[c:c + 4] * x32[:, c:c + 4]
                if t.shape[1] == 4:
                    sx = sx + ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3]))
                else:
                    u = t[:, 0]
                    for j in range(1, t.shape[1]):
                        u = u + t[:, j]
                    sx = sx + u
            row = row + (e * inv_c) * (W * l - sx)
        row = torch.where(valid, row, zero)
        b = e * inv_c
        fp, fa, fb = gr * (a + b * W), gr * a, gr * b
        dl = fp[:, None] * p - oh * fa[:, None] - fb[:, None] * wv[None, :]
    assert l.dtype == f32 and row.dtype == f32 and dl.dtype == f32
    return dict(lse=l, row=row, wy=wy, dl=dl, valid=valid)


# ---------------------------------------------------------------------------------------------------------------------
# the routes on top of the family

DEEPSUP_CASES = [(2, 5, 4, 4, 37, 40), (1, 4, 6, 16, 64, 64)]      # (B, h, w, s, nc, ld); the fused kernels end at 64 classes
DEEPSUP_REGIMES = ("confident", "offset", "sweep", "ascending")    # no -inf: a clamped border computes fma(0, -inf, ...)


def deepsup_regime_inputs(case, regime, seed):
    """coarse logits (B, h, w, ld) of the regime (its rows are the coarse pixels) and the fine labels of
    tests/deepsup_bounds.deepsup_inputs"""
    from tests.deepsup_bounds import deepsup_inputs
    B, h, w, s, nc, ld = case
    buf, _ = regime_inputs(regime, B * h * w, nc, ld, seed)
    return buf.view(B, h, w, ld), deepsup_inputs(case)[1]


OHEM_CASES = [(300, 9, 12), (300, 68, 68)]
OHEM_REGIMES = ("confident", "offset")
OHEM_THRESH, OHEM_MIN_KEPT = 0.7, 16
# seeds at which no valid row lies within delta_r of tau (``ohem_gap_violations``), found on the CPU with the twin
OHEM_SEEDS = {("confident", (300, 9, 12)): 720, ("confident", (300, 68, 68)): 720, ("offset", (300, 9, 12)): 812,
              ("offset", (300, 68, 68)): 720}


def ohem_gap_violations(t, nc):
    """valid rows within delta_r = max(64, C + 10) u (|lse_r| + |x_{r,y}| + 1) of tau (tests/test_ohem_gpu.py: a condition
    on the inputs, not a tolerance -- such a row could change sides by rounding alone)"""
    delta = max(64, nc + 10) * U * (t["lse"].abs() + t["xy"].abs() + 1.0)
    return int((t["valid"] & (t["dist"] <= delta)).sum())
