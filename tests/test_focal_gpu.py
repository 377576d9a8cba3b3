"""The focal loss on the project's kernels: sigma_softmax_focal_fwd / _bwd against the fp64 twin (tests/focal_fp64_twin.py)
at both pitches and in both regimes, ``pointwise.focal_cross_entropy`` / ``utils.loss_opr.FocalLoss2d`` on the padded view,
the hand-off to gemm.classifier's backward, the model, deterministic mode and graph capture; run with -m gpu.

Bounds, |got - ref| <= K u S with u = 2^-24 (``check`` / ``rejects`` of tests/test_stream_fp64_gpu.py); the derivation is
written once, next to the code that evaluates it, in the docstring of tests/focal_bounds.py, and tests/test_focal_cpu.py
holds an fp32 emulation of the kernels against the same bounds on the same inputs.  In short, with l = lse, d = x_y - l,
nll = -d, p_y = exp(d), q = 1 - p_y, t = q^(gamma - 1), G = t q, T = gamma t p_y nll, m = G + T, A = |l| + 1 + |x_y|:

lse       K = C + 8, S = |l| + 1 (the code of the plain kernels).
interval  the kernel evaluates the exact functions at points of I = [d - D, min(d + D, 0)], D = (C + 12) u A (l: C + 8, the
          subtraction, exp within 2 ulp taken as a shift of its argument), with relative roundings on top.  Rows whose q is
          within D of zero have a relative error of order one in q (second order in u at the reference point), so every
          sensitivity is evaluated at the end of I with the larger q and nll (index hi), using p_y nll <= q.
row_loss  K = C + 12,  S = w_y (A m_hi + G_hi nll_hi (gamma + R + 3) / K):  |d(G nll)/dd| = m;  R = roundings of the power
          (0 for gamma 0 and 1, 1 for the square, 6 (gamma - 1) (|log q_lo| + 1) + 3 for exp((gamma - 1) log q) q).
partials  K = ceil(rows / (256 x 1024)) + 10 (+ C + 12 for the loss), S = sum of the rows' S / sum of w_y.
dlogits   K = C + 12,  S = |g| w_y [ m_hi p_c (|x_c| + |l| + 1) + (p_c + [c == y]) (A M1_hi + m_hi (gamma + R + 8) / K) ]
          + 2^-125 (1 + |g| w_y m_hi) / (K u),  M1 = gamma t p_y (gamma + 1 + nll) >= |dm/dd|; the last term is fp32's
          underflow threshold (rows raised by 150: p_c ~ 1e-66).
Through ``focal_cross_entropy`` with 'mean', g = upstream / den is formed on the device from the fp32 den: K + 13, as in
tests/test_loss_options_gpu.py; the tests there have at most 256 rows, so only workgroup 0 holds non-zero partials.
Worst error / bound seen on an MI355X over the 80 kernel cases: lse 0.14, row_loss 0.12, loss sum 0.03, sum of w_y 0.14,
dlogits 0.39 (scalar and per-row gradient alike).
"""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import focal_bounds as fb
from tests.focal_fp64_twin import twin
from tests.test_gemm_gpu import _assert_close, _bound
from tests.test_head_classes_gpu import _boom, _head_inputs, _image_labels, _padded_logits
from tests.test_stream_fp64_gpu import _guarded, _intact, check, rejects

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGNORE = fb.IGNORE
FAMILY = "focal loss"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(buf, lab, w, nc, ld, lse):
    from sigma_amd import _capi
    p = _capi.CeOptParams()
    p.rows, p.classes, p.ld, p.ignore_index, p.label_smoothing = buf.shape[0], nc, ld, IGNORE, 0.0
    p.logits, p.labels, p.lse = buf.data_ptr(), lab.data_ptr(), lse.data_ptr()
    p.weight = w.data_ptr() if w is not None else None
    return p


_INPUTS = {}


def _inputs(case):
    """the case's inputs on the device and their fp64 logits, made once and shared by its eight parametrisations"""
    if case not in _INPUTS:
        rows, nc, ld = case
        buf, lab, sat = fb.focal_inputs(rows, nc, ld, seed=401)
        _INPUTS[case] = (buf.to(DEV), lab.to(DEV), sat.to(DEV), buf[:, :nc].double().to(DEV), fb.focal_weights(nc, seed=403).to(DEV))
    return _INPUTS[case]


@pytest.mark.parametrize("has_w", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("gamma", fb.GAMMAS)
@pytest.mark.parametrize("case", fb.CASES, ids=fb.CASE_IDS)
def test_focal_kernels_against_fp64(case, gamma, has_w):
    """NaN in the pad columns, labels inside the pad and negative labels (ignored), one class with weight zero, rows with
    the label's logit raised by 5 ... 40, lowered by 30 and raised by 150 (tests/focal_bounds.focal_inputs).  EVERY row
    and column of lse, row_loss and dlogits (device scalar and per-row gradient) and both summed partials under the bounds
    of the module docstring; exact zeros in the pad, at invalid rows and -- loss, and for gamma > 0 gradient -- at the rows
    raised by 150; guard bands intact; the partials do not depend on whether row_loss is asked for.  Negative controls, each
    of which the kernel's output must FAIL: the gradient with the modulating factor detached (gamma > 0, more than one
    class), the reference's fixed exponent 2 where gamma = 3.5, 'mean' divided by the pixel count (weighted)."""
    from sigma_amd import _capi
    rows, nc, ld = case
    lib = _capi.load()
    buf, lab, sat, x, w_all = _inputs(case)
    w = w_all if has_w else None
    glse, grow = _guarded((rows,), 64), _guarded((rows,), 64)
    part, part2 = _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2), _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2)
    p = _params(buf, lab, w, nc, ld, glse[1])
    p.row_loss, p.partial = grow[1].data_ptr(), part[1].data_ptr()
    _capi.check(lib.sigma_softmax_focal_fwd(ctypes.byref(p), gamma, _stream()), "focal fwd")
    lse2 = torch.empty(rows, device=DEV)
    p2 = _params(buf, lab, w, nc, ld, lse2)
    p2.partial = part2[1].data_ptr()                                         # row_loss = NULL
    _capi.check(lib.sigma_softmax_focal_fwd(ctypes.byref(p2), gamma, _stream()), "focal fwd without row_loss")
    torch.cuda.synchronize()
    r0 = fb.bounds(x, lab, nc, w, gamma, 0.0)
    den = float(r0["wy"].sum())
    assert den > 0
    scale = torch.tensor([0.7 / den], device=DEV)
    row_grad = torch.randn(rows, generator=torch.Generator().manual_seed(404)).to(DEV)
    gdl_s, gdl_r = _guarded((rows, ld), ld), _guarded((rows, ld), ld)
    p.scale, p.row_grad, p.dlogits = scale.data_ptr(), None, gdl_s[1].data_ptr()
    _capi.check(lib.sigma_softmax_focal_bwd(ctypes.byref(p), gamma, _stream()), "focal bwd (scale)")
    p.scale, p.row_grad, p.dlogits = None, row_grad.data_ptr(), gdl_r[1].data_ptr()
    _capi.check(lib.sigma_softmax_focal_bwd(ctypes.byref(p), gamma, _stream()), "focal bwd (row gradient)")
    torch.cuda.synchronize()
    for gg, what in ((glse, "lse"), (grow, "row_loss"), (part, "partial"), (part2, "partial (no row_loss)"), (gdl_s, "dlogits"),
                     (gdl_r, "dlogits (row gradient)")):
        _intact(gg, what)
    assert torch.isfinite(part[1]).all(), "NaN of the pad reached the partial sums"
    assert torch.equal(part[1], part2[1]) and torch.equal(glse[1], lse2)

    K = r0["K"]
    ratios = {}
    ratios["lse"] = check(FAMILY, glse[1], r0["lse"], r0["S_lse"], r0["K_lse"], "lse")
    ratios["row_loss"] = check(FAMILY, grow[1], r0["row"], r0["S_row"], K, "row_loss")
    assert bool((grow[1][~r0["valid"]] == 0).all()), "row_loss of an ignored row is not zero"
    assert bool((grow[1][sat] == 0).all()), "row_loss of a saturated row (q = 0) is not exactly zero"
    got_sum, got_den = part[1][:, 0].double().sum().view(1), part[1][:, 1].double().sum().view(1)
    S_sum, S_den = r0["S_row"].sum().view(1), r0["wy"].sum().view(1)
    ratios["loss sum"] = check(FAMILY, got_sum, r0["row"].sum().view(1), S_sum, fb.k_sum(rows) + K, "loss sum")
    ratios["den"] = check(FAMILY, got_den, S_den, S_den, fb.k_sum(rows), "sum of w_y")
    grads = ((gdl_s, float(scale), "scale"), (gdl_r, row_grad, "row gradient"))
    for gdl, g, what in grads:
        r = fb.bounds(x, lab, nc, w, gamma, g)
        ratios["dlogits " + what] = check(FAMILY, gdl[1][:, :nc], r["dl"], r["S_dl"], K, f"dlogits ({what})")
        pad = gdl[1][:, nc:]
        assert pad.numel() == rows * (ld - nc) and bool((pad == 0).all()), "pad columns of dlogits are not exact zeros"
        assert bool((gdl[1][~r0["valid"]] == 0).all()), "dlogits of an ignored row are not exact zeros"
        if gamma > 0:
            assert bool((gdl[1][sat] == 0).all()), "dlogits of a saturated row (q = 0) are not exact zeros"
    print(f"\n{case} gamma {gamma} {'w' if has_w else 'plain'}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of the bound")

    # negative controls
    for gdl, g, what in grads:
        r = fb.bounds(x, lab, nc, w, gamma, g)
        if gamma > 0 and nc > 1:
            wrong = twin(x, lab, IGNORE, gamma, weight=w, reduction="none", upstream=g, variant="detached")
            rejects(gdl[1][:, :nc], wrong["dl"], r["S_dl"], K, f"modulating factor detached ({what})")
        if gamma == 3.5 and nc > 1:
            wrong = twin(x, lab, IGNORE, gamma, weight=w, reduction="none", upstream=g, variant="square")
            rejects(gdl[1][:, :nc], wrong["dl"], r["S_dl"], K, f"exponent 2 at gamma 3.5 ({what})")
    if gamma == 3.5 and nc > 1:
        wrong = twin(x, lab, IGNORE, gamma, weight=w, reduction="none", variant="square")
        rejects(grow[1], wrong["row"], r0["S_row"], K, "exponent 2 at gamma 3.5 (row_loss)")
        rejects(got_sum, wrong["row"].sum().view(1), S_sum, fb.k_sum(rows) + K, "exponent 2 at gamma 3.5 (sum)")
    if has_w:
        count = r0["valid"].double().sum().view(1)
        rejects(got_den, count, S_den, fb.k_sum(rows), "mean denominator = pixel count")


def _upstream(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV) if len(shape) else torch.tensor(1.7, device=DEV)


def _focal(exponent, w, red):
    from sigma_amd.utils.loss_opr import FocalLoss2d
    return FocalLoss2d(weight=w, reduction=red, ignore_index=IGNORE, exponent=exponent).to(DEV)


@pytest.mark.parametrize("has_w", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("nc", [5, 9, 37, 40])
def test_class_takes_the_kernels_on_the_padded_view(nc, has_w, monkeypatch):
    """FocalLoss2d on the (B, nc, H, W) view of a (2, 9, 11, ld) buffer whose pad holds NaN (40 classes: contiguous), every
    reduction, exponent None (= 2) and 3.5, with the torch formulation made to raise: the kernel route ran.  'mean' and
    'sum' against the twin at rtol 1e-5; 'none' returns (B, H, W), every pixel under the row_loss bound and the map's sum at
    rtol 1e-5.  The gradient under the dlogits bound (K + 13 for 'mean'), zeros in the pad, the same bits from a second
    call; 0 < exponent < 1 is declined by ``focal_cross_entropy``."""
    from sigma_amd.pointwise import SoftmaxFocalFn, focal_cross_entropy
    B, H, W = 2, 9, 11
    ld = (nc + 3) // 4 * 4
    label = _image_labels(B, H, W, nc, seed=422)
    w = fb.focal_weights(nc, seed=423) if has_w else None
    lab = label.view(-1)
    monkeypatch.setattr(F, "softmax", _boom)
    monkeypatch.setattr(F, "log_softmax", _boom)
    for exponent in (None, 3.5):
        gamma = 2.0 if exponent is None else exponent
        for red in ("mean", "sum", "none"):
            crit = _focal(exponent, w, red)
            up = _upstream((B, H, W) if red == "none" else (), seed=424)

            def run():
                buf = _padded_logits(B * H * W, nc, ld, seed=421).view(B, H, W, ld).requires_grad_()
                loss = crit(buf[..., :nc].permute(0, 3, 1, 2), label)
                assert type(loss.grad_fn).__name__.startswith(SoftmaxFocalFn.__name__)
                (loss * up).sum().backward()
                return buf, loss.detach(), buf.grad.view(-1, ld)

            buf, loss, g = run()
            x = buf.detach()[..., :nc].double().reshape(-1, nc)
            wd = w.to(DEV) if has_w else None
            r0 = fb.bounds(x, lab, nc, wd, gamma, 0.0)
            want = twin(x, lab, IGNORE, gamma, weight=wd, reduction=red)["loss"]
            K = r0["K"]
            if red == "none":
                assert tuple(loss.shape) == (B, H, W)
                check(FAMILY, loss.view(-1), want, r0["S_row"], K, "per-pixel loss")
                torch.testing.assert_close(loss.double().sum(), want.sum(), rtol=1e-5, atol=0.0)
                gup, Kd = up.view(-1), K
            else:
                assert loss.dim() == 0
                torch.testing.assert_close(loss.double(), want, rtol=1e-5, atol=0.0)
                gup, Kd = (float(up) / r0["den"], K + 13) if red == "mean" else (float(up), K)
            r = fb.bounds(x, lab, nc, wd, gamma, gup)
            check(FAMILY, g[:, :nc], r["dl"], r["S_dl"], Kd, f"gradient of the padded view ({red})")
            assert bool((g[:, nc:] == 0).all())
            _, loss2, g2 = run()
            assert torch.equal(loss2, loss) and torch.equal(g2, g)
    buf = _padded_logits(B * H * W, nc, ld, seed=421).view(B, H, W, ld)
    for gamma in (0.5, 0.999, -1.0, float("nan"), float("inf")):
        assert focal_cross_entropy(buf[..., :nc].permute(0, 3, 1, 2), label, IGNORE, gamma) is None


def test_fractional_exponent_takes_the_torch_formulation():
    """exponent 0.5 on the padded view: declined by the kernels, FocalLoss2d answers with the torch formulation"""
    nc, ld, B, H, W = 9, 12, 2, 9, 11
    label = _image_labels(B, H, W, nc, seed=432)
    buf = _padded_logits(B * H * W, nc, ld, seed=431).view(B, H, W, ld)
    view = buf[..., :nc].permute(0, 3, 1, 2)
    loss = _focal(0.5, None, "mean")(view, label)
    want = F.nll_loss((1 - F.softmax(view.double(), 1)) ** 0.5 * F.log_softmax(view.double(), 1), label, ignore_index=IGNORE)
    assert loss.grad_fn is None or "Focal" not in type(loss.grad_fn).__name__
    torch.testing.assert_close(loss.double(), want, rtol=1e-5, atol=0.0)


@pytest.mark.parametrize("red", ["mean", "none"])
def test_focal_route_hands_its_padded_gradient_to_the_classifier(red, monkeypatch):
    """x (2, 9, 11, 96) through gemm.classifier (9 classes at pitch 12) and the weighted focal loss, then backward, with
    torch.mm and F.linear raising: the classifier's backward CLAIMS the loss backward's (rows, ld) buffer, and x.grad /
    weight.grad agree with fp64 linear + the twin's gradient under the GEMM tests' bound."""
    from sigma_amd import _handoff, gemm
    nc, C = 9, 96
    x0, w0, label = _head_inputs(nc, C, seed=441)
    cw = fb.focal_weights(nc, seed=442).to(DEV)
    crit = _focal(None, cw, red)
    up = _upstream(tuple(label.shape) if red == "none" else (), seed=443)
    x64, w64 = x0.double().reshape(-1, C), w0.double().view(nc, C)
    dl64 = twin(x64 @ w64.t(), label.view(-1), IGNORE, 2.0, weight=cw, reduction=red, upstream=up.view(-1) if red == "none" else float(up))["dl"]
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
        loss = crit(logits.permute(0, 3, 1, 2), label)
        assert "SoftmaxFocalFn" in type(loss.grad_fn).__name__
        (loss * up).sum().backward()
        torch.cuda.synchronize()
    assert claimed == [True], claimed
    _assert_close(x.grad.reshape(-1, C), dl64 @ w64, _bound(dl64, w64), "x.grad")
    _assert_close(w.grad.view(nc, C), dl64.t() @ x64, _bound(dl64.t(), x64), "weight.grad")


def test_model_step_with_the_focal_criterion(monkeypatch):
    """sigma_tiny 64x96, batch 1, 9 classes, criterion = FocalLoss2d(weight=...): one train step calls the focal entry
    points once each, every parameter gets a finite gradient; in eval mode model(rgb, x, label) is the twin on the model's
    own logits at rtol 1e-5."""
    import collections
    from sigma_amd import _capi
    from tests.model_utils import build_model, fill
    nc = 9
    model = build_model("sigma_tiny", nc, 64, 96).cuda().train()
    cw = fb.focal_weights(nc, seed=451)
    model.criterion = _focal(None, cw.tolist(), "mean")
    rgb, x, label = (t.cuda() for t in fill.make_inputs(1, 64, 96, nc, seed=5))
    counts = collections.Counter()
    lib = _capi.load()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if "softmax" not in name:
                return fn

            def call(*args):
                counts[name] += 1
                return fn(*args)
            return call

    with monkeypatch.context() as m:
        m.setattr(_capi, "load", lambda: Counting())
        loss = model(rgb, x, label)
        loss.backward()
        torch.cuda.synchronize()
    assert dict(counts) == {"sigma_softmax_focal_fwd": 1, "sigma_softmax_focal_bwd": 1}, dict(counts)
    assert torch.isfinite(loss)
    bad = [n for n, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not bad, bad
    model.eval()
    with torch.no_grad():
        out = model(rgb, x)
        got = model(rgb, x, label)
    want = twin(out.double().permute(0, 2, 3, 1).reshape(-1, nc), label.view(-1), IGNORE, 2.0, weight=cw.to(DEV), reduction="mean")["loss"]
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=0.0)


def _step(crit, buf, label, up, nc):
    loss = crit(buf[..., :nc].permute(0, 3, 1, 2), label)
    (grad,) = torch.autograd.grad((loss * up).sum(), buf)
    return loss.detach(), grad


@pytest.mark.parametrize("red", ["mean", "none"])
def test_focal_route_is_deterministic_and_captured_into_a_graph(red):
    """9 classes at pitch 12, weights, exponent 3.5: two calls give the same bits; under
    torch.use_deterministic_algorithms(True) the class neither raises nor changes its bits; forward + backward captured by
    torch.cuda.graph after a warm-up on a side stream replays to the bits of the eager run."""
    nc, ld, B, H, W = 9, 12, 2, 9, 11
    label = _image_labels(B, H, W, nc, seed=462)
    crit = _focal(3.5, fb.focal_weights(nc, seed=463), red)
    up = _upstream((B, H, W) if red == "none" else (), seed=464)
    buf = _padded_logits(B * H * W, nc, ld, seed=461).view(B, H, W, ld).requires_grad_()
    loss_e, grad_e = (t.clone() for t in _step(crit, buf, label, up, nc))
    loss_2, grad_2 = _step(crit, buf, label, up, nc)
    assert torch.equal(loss_2, loss_e) and torch.equal(grad_2, grad_e)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        loss_d, grad_d = _step(crit, buf, label, up, nc)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(loss_d, loss_e) and torch.equal(grad_d, grad_e)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _step(crit, buf, label, up, nc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = _step(crit, buf, label, up, nc)
    loss_g.zero_()
    grad_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss_e).all() and bool((grad_e.view(-1, ld)[:, nc:] == 0).all())
    assert torch.equal(loss_g, loss_e) and torch.equal(grad_g, grad_e)


def test_class_under_the_deterministic_flag_where_the_kernels_decline():
    """contiguous (B, 9, H, W) logits (9 % 4 != 0: no kernel route) under the flag: nll_loss2d would raise, the class
    answers with the element-wise formulation, twice with the same bits, and agrees with the twin"""
    nc, B, H, W = 9, 2, 9, 11
    label = _image_labels(B, H, W, nc, seed=472)
    z = (torch.randn(B, nc, H, W, generator=torch.Generator().manual_seed(471)) * 3.0).to(DEV).requires_grad_()
    crit = _focal(None, fb.focal_weights(nc, seed=473), "mean")
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        outs = []
        for _ in range(2):
            loss = crit(z, label)
            (grad,) = torch.autograd.grad(loss, z)
            outs.append((loss.detach(), grad))
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(was)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    t = twin(z.detach().permute(0, 2, 3, 1).reshape(-1, nc), label.view(-1), IGNORE, 2.0, weight=crit.loss.weight, reduction="mean")
    torch.testing.assert_close(outs[0][0].double(), t["loss"], rtol=1e-5, atol=0.0)
    torch.testing.assert_close(outs[0][1].permute(0, 2, 3, 1).reshape(-1, nc).double(), t["dl"], rtol=1e-4, atol=1e-7)
