"""Class weights, label smoothing and the reductions 'sum' / 'none' of the segmentation loss on the project's kernels:
sigma_softmax_ce_opt_fwd / _bwd against fp64 at both pitches and in both regimes, pointwise.cross_entropy on the padded
view, the hand-off to gemm.classifier's backward, the model, deterministic mode and graph capture; run with -m gpu.

Bounds (``check`` / ``rejects`` of tests/test_stream_fp64_gpu.py: |got - ref| <= K u S, u = 2^-24).  With w the class
weights (ones without), W = sum_c w_c, a = (1 - eps) w_y, b = eps / C, p = softmax(x), l = lse, everything below first
order in u, exp / log / rcp within 2 ulp:

lse       the code of the plain kernels: K = C + 8, S = |l| + 1.
row_loss  = a (l - x_y) + b (W l - sum_c w_c x_c).  S = a (|l| + 1 + |x_y|) + b (W (|l| + 1) + sum_c w_c |x_c|), the
          magnitudes of the terms.  First term: eps rounded to fp32, 1 - eps, times w_y (3), l (C + 8), the subtraction
          and the product (2): C + 13.  Second term: W is a serial sum of C weights (C), l (C + 8), W l (1) -- 2C + 9 on
          W |l|; sum_c w_c x_c is a product and a sum of depth <= C (C + 1) on its own magnitude; their difference (1),
          b = eps * (1 / C) (3), the product (1): 2C + 14.  The final add (1).  K = 2C + 16.
partial[:, 0]  the row losses of a thread added serially (ceil(rows / (256 x 1024)) of them), six butterfly levels in the
          wave and four serial adds in the workgroup; the 1024 partials are added in fp64 here:
          K = ceil(rows / (256 x 1024)) + 10 + (2C + 16), S = sum of the rows' S.
partial[:, 1]  = sum of w_y over the valid rows, a FLOAT sum now: K = ceil(rows / (256 x 1024)) + 10, S = sum of w_y.
dlogits   = (g (a + b W)) p_c - [c == y] g a - (g b) w_c.  S = |g| ((a + b W) p_c (|x_c| + |l| + 1) + a [c == y] + b w_c).
          p_c = exp(x_c - l): l (C + 8), the subtraction (1, on |x| + |l|), exp (2): C + 11 on p (|x| + |l| + 1).
          g (a + b W): a (3), b (3), W (C), b W, the add, times g (3): C + 9.  Their product (1): 2C + 21 on the first
          term; g a (4) and g b w_c (5) on theirs; two subtractions (2).  K = 2C + 24.
Through ``pointwise.cross_entropy`` with 'mean', g = upstream / den is formed on the device from the fp32 den: its K
(above, one row per thread: 11), the division and the product with the loss' own upstream gradient (2) come on top:
K = 2C + 37.  The tests there have at most 256 rows, so that only workgroup 0 holds non-zero partials and torch's sum of
the 1024 adds zeros (exact).
"""
from __future__ import annotations

import collections
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gemm_gpu import _assert_close, _bound
from tests.test_head_classes_gpu import CE_LD_CASES, IGNORE, _boom, _head_inputs, _image_labels, _labels, _padded_logits
from tests.test_stream_fp64_gpu import U, _guarded, _intact, check, rejects  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = "cross entropy options"
# (class weights?, label smoothing)
OPTS = [(True, 0.0), (False, 0.1), (True, 0.1)]
OPT_IDS = ["w", "eps", "w+eps"]
# the padded-pitch cases of tests/test_head_classes_gpu.py (registers up to 64 classes, walking above; one class; one row;
# a pitch above 4 ceil(classes / 4)) and the contiguous kernels in both regimes
CASES = CE_LD_CASES + [(3001, 40, 40), (1031, 68, 68)]


def _weights(nc, seed):
    """fp32 class weights in [0.1, 2.1], class nc // 2 with an exact zero (not where there is one class only: every loss,
    denominator and gradient would be zero)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.rand(nc, generator=g, device=DEV) * 2.0 + 0.1
    if nc > 1:
        w[nc // 2] = 0.0
    return w


def _params(buf, lab, w, eps, nc, ld, lse):
    from sigma_amd import _capi
    p = _capi.CeOptParams()
    p.rows, p.classes, p.ld, p.ignore_index, p.label_smoothing = buf.shape[0], nc, ld, IGNORE, eps
    p.logits, p.labels, p.lse = buf.data_ptr(), lab.data_ptr(), lse.data_ptr()
    p.weight = w.data_ptr() if w is not None else None
    return p


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ref(x, lab, nc, w, eps, g, smooth_w=True, grad_w_term=True, ignored_as_class0=False):
    """fp64 of the formulas in include/sigma_ops.h: validity, lse, row_loss and its S, w_y, dlogits for the upstream g (a
    float or a (rows,) tensor) and its S.  The three flags build the WRONG variants of the negative controls."""
    rows = x.shape[0]
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    if ignored_as_class0:
        valid = torch.ones_like(valid)
    w64 = w.double() if w is not None else torch.ones(nc, device=DEV, dtype=torch.float64)
    ws = w64 if smooth_w else torch.ones_like(w64)
    W, Ws = w64.sum(), ws.sum()
    lse = torch.logsumexp(x, 1)
    xl = x.gather(1, safe[:, None])[:, 0]
    p = torch.softmax(x, 1)
    oh = F.one_hot(safe, nc).double()
    wy = torch.where(valid, w64[safe], torch.zeros_like(lse))
    a, b = (1.0 - eps) * wy, eps / nc
    zero = torch.zeros_like(lse)
    row = torch.where(valid, a * (lse - xl) + b * (Ws * lse - (ws * x).sum(1)), zero)
    S_row = torch.where(valid, a * (lse.abs() + 1.0 + xl.abs()) + b * (W * (lse.abs() + 1.0) + (w64 * x.abs()).sum(1)), zero)
    gr = (g.double() if torch.is_tensor(g) else torch.full((rows,), float(g), device=DEV, dtype=torch.float64))[:, None]
    wterm = w64[None, :] if grad_w_term else torch.zeros(1, nc, device=DEV, dtype=torch.float64)
    dl = torch.where(valid[:, None], gr * (a[:, None] * (p - oh) + b * (W * p - wterm)), torch.zeros_like(p))
    S_dl = torch.where(valid[:, None], gr.abs() * ((a[:, None] + b * W) * p * (x.abs() + lse.abs()[:, None] + 1.0) + a[:, None] * oh
                                                   + b * w64[None, :]), torch.zeros_like(p))
    return dict(valid=valid, lse=lse, row=row, S_row=S_row, wy=wy, dl=dl, S_dl=S_dl)


def _k_row(nc):
    return 2 * nc + 16


def _k_sum(rows):
    from sigma_amd import _capi
    return -(-rows // (256 * _capi.SIGMA_CE_BLOCKS)) + 10


def _k_dl(nc):
    return 2 * nc + 24


@pytest.mark.parametrize("opt", OPTS, ids=OPT_IDS)
@pytest.mark.parametrize("case", CASES, ids=[f"{r}x{c}@{l}" for r, c, l in CASES])
def test_option_kernels_against_fp64(case, opt):
    """NaN in the pad columns, labels inside the pad and negative labels (ignored), one class with weight zero.  lse,
    row_loss, both columns of the summed partials and dlogits -- with the device scalar and with a per-row gradient --
    under the bounds of the module docstring; exact zeros in the pad of dlogits; guard bands intact; the partials do not
    depend on whether row_loss is asked for.  Negative controls (reference code only), each of which the kernel's output
    must FAIL: the mean's denominator taken as the pixel count (with weights); the smoothing term summed without w_c
    (weights and eps; not for one class, where lse = x and the term is zero either way); the gradient without its
    -(eps / C) w_c term (eps); ignored pixels counted as class 0 (where the case has ignored rows: all but the one-row
    case; with one class only the denominator can tell: p = 1 and lse = x there)."""
    from sigma_amd import _capi
    rows, nc, ld = case
    has_w, eps = opt
    lib = _capi.load()
    buf = _padded_logits(rows, nc, ld, seed=301)
    lab = _labels(rows, nc, ld, seed=302)
    w = _weights(nc, seed=303) if has_w else None
    x = buf[:, :nc].double()
    glse, grow = _guarded((rows,), 64), _guarded((rows,), 64)
    part, part2 = _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2), _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2)
    p = _params(buf, lab, w, eps, nc, ld, glse[1])
    p.row_loss, p.partial = grow[1].data_ptr(), part[1].data_ptr()
    _capi.check(lib.sigma_softmax_ce_opt_fwd(ctypes.byref(p), _stream()), "ce opt fwd")
    lse2 = torch.empty(rows, device=DEV)
    p2 = _params(buf, lab, w, eps, nc, ld, lse2)
    p2.partial = part2[1].data_ptr()                                         # row_loss = NULL
    _capi.check(lib.sigma_softmax_ce_opt_fwd(ctypes.byref(p2), _stream()), "ce opt fwd without row_loss")
    torch.cuda.synchronize()
    r0 = _ref(x, lab, nc, w, eps, 0.0)
    den = float(r0["wy"].sum())
    assert den > 0
    scale = torch.tensor([0.7 / den], device=DEV)
    row_grad = torch.randn(rows, generator=torch.Generator(device=DEV).manual_seed(304), device=DEV)
    gdl_s, gdl_r = _guarded((rows, ld), ld), _guarded((rows, ld), ld)
    p.scale, p.row_grad, p.dlogits = scale.data_ptr(), None, gdl_s[1].data_ptr()
    _capi.check(lib.sigma_softmax_ce_opt_bwd(ctypes.byref(p), _stream()), "ce opt bwd (scale)")
    p.scale, p.row_grad, p.dlogits = None, row_grad.data_ptr(), gdl_r[1].data_ptr()
    _capi.check(lib.sigma_softmax_ce_opt_bwd(ctypes.byref(p), _stream()), "ce opt bwd (row gradient)")
    torch.cuda.synchronize()
    for gg, what in ((glse, "lse"), (grow, "row_loss"), (part, "partial"), (part2, "partial (no row_loss)"), (gdl_s, "dlogits"),
                     (gdl_r, "dlogits (row gradient)")):
        _intact(gg, what)
    assert torch.isfinite(part[1]).all(), "NaN of the pad reached the partial sums"
    assert torch.equal(part[1], part2[1]) and torch.equal(glse[1], lse2)

    ratios = {}
    ratios["lse"] = check(FAMILY, glse[1], r0["lse"], r0["lse"].abs() + 1.0, nc + 8, "lse")
    ratios["row_loss"] = check(FAMILY, grow[1], r0["row"], r0["S_row"], _k_row(nc), "row_loss")
    assert bool((grow[1][~r0["valid"]] == 0).all()), "row_loss of an ignored row is not zero"
    got_sum, got_den = part[1][:, 0].double().sum().view(1), part[1][:, 1].double().sum().view(1)
    K_sum = _k_sum(rows) + _k_row(nc)
    S_sum, S_den = r0["S_row"].sum().view(1), r0["wy"].sum().view(1)
    ratios["loss sum"] = check(FAMILY, got_sum, r0["row"].sum().view(1), S_sum, K_sum, "loss sum")
    ratios["den"] = check(FAMILY, got_den, S_den, S_den, _k_sum(rows), "sum of w_y")
    grads = ((gdl_s, float(scale), "scale"), (gdl_r, row_grad, "row gradient"))
    for gdl, g, what in grads:
        r = _ref(x, lab, nc, w, eps, g)
        ratios["dlogits " + what] = check(FAMILY, gdl[1][:, :nc], r["dl"], r["S_dl"], _k_dl(nc), f"dlogits ({what})")
        pad = gdl[1][:, nc:]
        assert pad.numel() == rows * (ld - nc) and bool((pad == 0).all()), "pad columns of dlogits are not exact zeros"
        assert bool((gdl[1][~r0["valid"]] == 0).all()), "dlogits of an ignored row are not exact zeros"
    print(f"\n{case} {opt}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of the bound")

    # negative controls
    if has_w:
        count = r0["valid"].double().sum().view(1)
        rejects(got_den, count, S_den, _k_sum(rows), "mean denominator = pixel count")
    if has_w and eps > 0 and nc > 1:
        wrong = _ref(x, lab, nc, w, eps, 0.0, smooth_w=False)
        rejects(grow[1], wrong["row"], r0["S_row"], _k_row(nc), "smoothing term without w_c")
        rejects(got_sum, wrong["row"].sum().view(1), S_sum, K_sum, "smoothing term without w_c (sum)")
    if eps > 0:
        for gdl, g, what in grads:
            r = _ref(x, lab, nc, w, eps, g)
            wrong = _ref(x, lab, nc, w, eps, g, grad_w_term=False)
            rejects(gdl[1][:, :nc], wrong["dl"], r["S_dl"], _k_dl(nc), f"gradient without -(eps / C) w_c ({what})")
    if rows > 8:
        assert not bool(r0["valid"].all())
    if not bool(r0["valid"].all()):
        wrong = _ref(x, lab, nc, w, eps, float(scale), ignored_as_class0=True)
        wrong_den = wrong["wy"].sum().view(1)                 # the wrong variant's own magnitudes where the right one has none
        rejects(got_den, wrong_den, wrong_den, _k_sum(rows), "ignored pixels counted as class 0 (sum of w_y)")
        if nc > 1:                                            # one class: p = 1 and lse = x, loss and gradient vanish either way
            r = _ref(x, lab, nc, w, eps, float(scale))
            S0 = torch.maximum(r["S_dl"], wrong["S_dl"])
            rejects(gdl_s[1][:, :nc], wrong["dl"], S0, _k_dl(nc), "ignored pixels counted as class 0 (dlogits)")
            rejects(grow[1], wrong["row"], torch.maximum(r0["S_row"], wrong["S_row"]), _k_row(nc), "ignored pixels counted as class 0")


@pytest.mark.parametrize("case", [(3001, 9, 12), (3001, 40, 40), (1031, 68, 68)], ids=lambda c: f"{c[0]}x{c[1]}@{c[2]}")
def test_all_ones_weight_and_no_smoothing_is_the_plain_loss(case):
    """weight = ones, eps = 0 through the option entry points against the PLAIN entry points' output, under the plain
    kernels' own bounds (tests/test_stream_fp64_gpu.py: lse C + 8, loss sum ceil(rows / 2^18) + 8 + C + 8, dlogits
    C + 16); the denominator is the pixel count, exactly (a sum of ones below 2^24)"""
    from sigma_amd import _capi
    rows, nc, ld = case
    lib = _capi.load()
    buf = _padded_logits(rows, nc, ld, seed=311)
    lab = _labels(rows, nc, ld, seed=312)
    ones = torch.ones(nc, device=DEV)
    lse, lse0 = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    part, part0 = (torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=DEV) for _ in range(2))
    dl, dl0 = torch.empty(rows, ld, device=DEV), torch.empty(rows, ld, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _capi.check(lib.sigma_softmax_ce_fwd_ld(vp(buf), vp(lab), rows, nc, ld, IGNORE, vp(lse0), vp(part0), _stream()), "ce fwd ld")
    cnt = part0[:, 1].sum()
    scale = (0.7 / cnt).reshape(1)
    _capi.check(lib.sigma_softmax_ce_bwd_ld(vp(buf), vp(lab), vp(lse0), vp(scale), rows, nc, ld, IGNORE, vp(dl0), _stream()), "ce bwd ld")
    p = _params(buf, lab, ones, 0.0, nc, ld, lse)
    p.partial, p.scale, p.dlogits = part.data_ptr(), scale.data_ptr(), dl.data_ptr()
    _capi.check(lib.sigma_softmax_ce_opt_fwd(ctypes.byref(p), _stream()), "ce opt fwd")
    _capi.check(lib.sigma_softmax_ce_opt_bwd(ctypes.byref(p), _stream()), "ce opt bwd")
    torch.cuda.synchronize()
    x = buf[:, :nc].double()
    r = _ref(x, lab, nc, None, 0.0, float(scale))
    check(FAMILY, lse, lse0.double(), r["lse"].abs() + 1.0, nc + 8, "lse against the plain kernel")
    K = -(-rows // (256 * _capi.SIGMA_CE_BLOCKS)) + 8 + nc + 8
    check(FAMILY, part[:, 0].double().sum().view(1), part0[:, 0].double().sum().view(1), r["S_row"].sum().view(1), K, "loss sum against the plain kernel")
    assert float(part[:, 1].double().sum()) == float(cnt) == float(r["valid"].sum())
    S = torch.where(r["valid"][:, None], float(scale) * (torch.softmax(x, 1) * (x.abs() + r["lse"].abs()[:, None] + 1.0)
                                                           + F.one_hot(torch.where(r["valid"], lab, torch.zeros_like(lab)), nc)), torch.zeros_like(x))
    check(FAMILY, dl[:, :nc], dl0[:, :nc].double(), S, nc + 16, "dlogits against the plain kernel")
    assert torch.equal(dl[:, nc:], dl0[:, nc:]) and bool((dl[:, nc:] == 0).all())


def _criterion(w, eps, reduction):
    return nn.CrossEntropyLoss(weight=w, ignore_index=IGNORE, reduction=reduction, label_smoothing=eps)


def _upstream(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV) if len(shape) else torch.tensor(1.7, device=DEV)


@pytest.mark.parametrize("opt", OPTS, ids=OPT_IDS)
@pytest.mark.parametrize("nc", [5, 9, 37, 40])
def test_cross_entropy_takes_the_options_on_the_padded_view(nc, opt):
    """pointwise.cross_entropy on the (B, nc, H, W) view of a (2, 9, 11, ld) buffer whose pad holds NaN (40 classes:
    contiguous), every reduction.  'mean' and 'sum' against fp64 F.cross_entropy at rtol 1e-5; 'none' returns (B, H, W):
    every pixel under the row_loss bound (a pixel whose class has nearly all the probability has a loss near zero, which no
    relative tolerance fits) and the map's sum at rtol 1e-5.  The gradient under the dlogits bound (K of the module
    docstring), zeros in the pad, and the same bits from a second call."""
    from sigma_amd.pointwise import SoftmaxCEOptFn, cross_entropy
    has_w, eps = opt
    B, H, W = 2, 9, 11
    ld = (nc + 3) // 4 * 4
    label = _image_labels(B, H, W, nc, seed=322)
    w = _weights(nc, seed=323) if has_w else None
    w64 = w.double() if has_w else None
    for red in ("mean", "sum", "none"):
        crit = _criterion(w, eps, red)
        up = _upstream((B, H, W) if red == "none" else (), seed=324)

        def run():
            buf = _padded_logits(B * H * W, nc, ld, seed=321).view(B, H, W, ld).requires_grad_()
            loss = cross_entropy(crit, buf[..., :nc].permute(0, 3, 1, 2), label)
            assert loss is not None and type(loss.grad_fn).__name__.startswith(SoftmaxCEOptFn.__name__)
            (loss * up).sum().backward()
            return buf, loss.detach(), buf.grad.view(-1, ld)

        buf, loss, g = run()
        x = buf.detach()[..., :nc].double().reshape(-1, nc)
        want = F.cross_entropy(x, label.view(-1), weight=w64, ignore_index=IGNORE, reduction=red, label_smoothing=eps)
        lab = label.view(-1)
        r0 = _ref(x, lab, nc, w, eps, 0.0)
        if red == "none":
            assert tuple(loss.shape) == (B, H, W)
            torch.testing.assert_close(r0["row"], want, rtol=1e-12, atol=1e-12)          # the formulas ARE torch's
            check(FAMILY, loss.view(-1), want, r0["S_row"], _k_row(nc), "per-pixel loss")
            torch.testing.assert_close(loss.double().sum(), want.sum(), rtol=1e-5, atol=0.0)
            gup, K = up.view(-1), _k_dl(nc)
        else:
            assert loss.dim() == 0
            torch.testing.assert_close(loss.double(), want, rtol=1e-5, atol=0.0)
            den = float(r0["wy"].sum())
            gup, K = (float(up) / den, _k_dl(nc) + 13) if red == "mean" else (float(up), _k_dl(nc))
        r = _ref(x, lab, nc, w, eps, gup)
        z = x.clone().requires_grad_()
        (F.cross_entropy(z, lab, weight=w64, ignore_index=IGNORE, reduction=red, label_smoothing=eps) * up.double().view(-1 if red == "none" else ())).sum().backward()
        torch.testing.assert_close(r["dl"], z.grad, rtol=1e-10, atol=1e-12)               # the gradient formula IS torch's
        check(FAMILY, g[:, :nc], z.grad, r["S_dl"], K, f"gradient of the padded view ({red})")
        assert bool((g[:, nc:] == 0).all())
        _, loss2, g2 = run()
        assert torch.equal(loss2, loss) and torch.equal(g2, g)


@pytest.mark.parametrize("red", ["mean", "none"])
@pytest.mark.parametrize("nc", [5, 9, 37])
def test_option_route_hands_its_padded_gradient_to_the_classifier(nc, red, monkeypatch):
    """x (2, 9, 11, 96) through gemm.classifier and the weighted, smoothed loss, then backward, with torch.mm and F.linear
    raising: the classifier's backward CLAIMS the loss backward's (rows, ld) buffer (no zero-padding copy), and x.grad /
    weight.grad agree with fp64 linear + F.cross_entropy under the GEMM tests' bound."""
    from sigma_amd import _handoff, gemm
    from sigma_amd.pointwise import cross_entropy
    C = 96
    x0, w0, label = _head_inputs(nc, C, seed=331)
    cw = _weights(nc, seed=332)
    crit = _criterion(cw, 0.1, red)
    up = _upstream(tuple(label.shape) if red == "none" else (), seed=333)
    x64, w64 = x0.double().reshape(-1, C), w0.double().view(nc, C)
    z64 = (x64 @ w64.t()).requires_grad_()
    (F.cross_entropy(z64, label.view(-1), weight=cw.double(), ignore_index=IGNORE, reduction=red, label_smoothing=0.1)
     * up.double().view(-1 if red == "none" else ())).sum().backward()
    dl64 = z64.grad
    claimed = []
    real_claim = _handoff.claim_padded_grad_buffer

    def claim(dy, ld):
        full = real_claim(dy, ld)
        claimed.append(full is not None)
        return full

    x = x0.clone().requires_grad_()
    w = nn.Parameter(w0.clone())
    with monkeypatch.context() as m:
        m.setattr(torch, "mm", _boom)
        m.setattr(torch.nn.functional, "linear", _boom)
        m.setattr(_handoff, "claim_padded_grad_buffer", claim)
        assert gemm.classifier_ok(x.reshape(-1, C), w)
        logits = gemm.classifier(x, w)
        loss = cross_entropy(crit, logits.permute(0, 3, 1, 2), label)
        assert loss is not None
        (loss * up).sum().backward()
        torch.cuda.synchronize()
    assert claimed == [True], claimed
    _assert_close(x.grad.reshape(-1, C), dl64 @ w64, _bound(dl64, w64), "x.grad")
    _assert_close(w.grad.view(nc, C), dl64.t() @ x64, _bound(dl64.t(), x64), "weight.grad")
    assert w.grad.is_contiguous() and tuple(w.grad.shape) == (nc, C, 1, 1)


OLD = ("sigma_softmax_ce_fwd", "sigma_softmax_ce_bwd", "sigma_softmax_ce_fwd_ld", "sigma_softmax_ce_bwd_ld")
NEW = ("sigma_softmax_ce_opt_fwd", "sigma_softmax_ce_opt_bwd")


class _Counting:
    """stands in for the ctypes library: counts the calls of the loss entry points by name, forwards everything"""

    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in OLD + NEW:
            return fn

        def call(*args):
            self._counts[name] += 1
            return fn(*args)
        return call


@pytest.mark.parametrize("nc", [9, 40])
def test_model_step_with_a_weighted_smoothed_criterion(nc, monkeypatch):
    """sigma_tiny 64x96, batch 1, criterion with class weights and eps = 0.1.  One train step calls the option entry points
    once each and the four plain ones never; every parameter has a finite gradient.  In eval mode model(rgb, x, label) is
    fp64 F.cross_entropy of model(rgb, x) at rtol 1e-5, and reduction 'none' returns (B, H, W)."""
    from sigma_amd import _capi
    from tests.model_utils import build_model, fill
    model = build_model("sigma_tiny", nc, 64, 96).cuda().train()
    cw = _weights(nc, seed=341)
    model.criterion = _criterion(cw, 0.1, "mean")
    rgb, x, label = (t.cuda() for t in fill.make_inputs(1, 64, 96, nc, seed=5))
    counts = collections.Counter()
    rec = _Counting(_capi.load(), counts)
    with monkeypatch.context() as m:
        m.setattr(_capi, "load", lambda: rec)
        loss = model(rgb, x, label)
        loss.backward()
        torch.cuda.synchronize()
    assert [counts[s] for s in NEW] == [1, 1] and [counts[s] for s in OLD] == [0, 0, 0, 0], dict(counts)
    assert torch.isfinite(loss)
    bad = [n for n, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not bad, bad
    model.eval()
    with torch.no_grad():
        out = model(rgb, x)
        got = model(rgb, x, label)
        want = F.cross_entropy(out.double(), label, weight=cw.double(), ignore_index=IGNORE, label_smoothing=0.1)
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=0.0)
        model.criterion = _criterion(cw, 0.1, "none")
        rows = model(rgb, x, label)
        assert tuple(rows.shape) == (1, 64, 96) and rows.dtype == torch.float32
        want = F.cross_entropy(out.double(), label, weight=cw.double(), ignore_index=IGNORE, label_smoothing=0.1, reduction="none")
        torch.testing.assert_close(rows.double().sum(), want.sum(), rtol=1e-5, atol=0.0)
        assert bool((rows[label == IGNORE] == 0).all())


def test_weighted_step_under_the_deterministic_flag():
    """tests/loss_options_deterministic_worker.py: under torch.use_deterministic_algorithms(True) the weighted, smoothed
    step of sigma_tiny (9 and 40 classes) runs, and two runs give the same loss and gradient bits.  In a child process: the
    flag stays out of this one."""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    r = subprocess.run([sys.executable, "-m", "tests.loss_options_deterministic_worker"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[loss_options_deterministic_worker] done" in r.stdout


@pytest.mark.parametrize("red", ["mean", "none"])
def test_option_route_is_captured_into_a_graph(red):
    """forward + backward of the option route (9 classes at pitch 12, weights, eps = 0.1) captured by torch.cuda.graph after
    a warm-up on a side stream: the replay gives the bits of the eager run -- nothing on the route waits for the host"""
    from sigma_amd.pointwise import cross_entropy
    nc, ld, B, H, W = 9, 12, 2, 9, 11
    label = _image_labels(B, H, W, nc, seed=352)
    crit = _criterion(_weights(nc, seed=353), 0.1, red)
    up = _upstream((B, H, W) if red == "none" else (), seed=354)
    buf = _padded_logits(B * H * W, nc, ld, seed=351).view(B, H, W, ld).requires_grad_()

    def step():
        loss = cross_entropy(crit, buf[..., :nc].permute(0, 3, 1, 2), label)
        (grad,) = torch.autograd.grad((loss * up).sum(), buf)
        return loss.detach(), grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    loss_e, grad_e = (t.clone() for t in step())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = step()
    loss_g.zero_()
    grad_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_e).all() and bool((grad_e.view(-1, ld)[:, nc:] == 0).all())
    assert torch.equal(loss_g, loss_e) and torch.equal(grad_g, grad_e)
