"""The classifier head and the loss for class counts that are no multiple of 4 (MFNet 9, PST900 5, SUN-RGBD 37) on the
project's kernels: sigma_softmax_ce_fwd_ld / _bwd_ld against fp64, pointwise.cross_entropy on the padded view,
gemm.classifier (forward and both gradients on the split-operand GEMMs at the padded pitch) and the model; run with -m gpu.

Bounds: those of tests/test_stream_fp64_gpu.py::test_softmax_ce_against_fp64 (``check`` / ``rejects``, u = 2^-24; lse
K = classes + 8, loss sum K = ceil(rows / (256 x 1024)) + 8 + classes + 8, dlogits K = classes + 16) and of
tests/test_gemm_gpu.py (``_assert_close`` under ``_bound`` = sum |a||b|).  No tolerance is derived here."""
from __future__ import annotations

import collections
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gemm_gpu import _assert_close, _bound
from tests.test_stream_fp64_gpu import U, _guarded, _intact, check, rejects  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGNORE = 255


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded_logits(rows, nc, ld, seed):
    """(rows, ld) buffer: N(0, 3^2) logits in the first nc columns, NaN behind them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.full((rows, ld), float("nan"), device=DEV)
    buf[:, :nc] = torch.randn(rows, nc, generator=g, device=DEV) * 3.0
    return buf


def _labels(rows, nc, ld, seed):
    """labels in [0, nc), ~10 % ignore_index; every 7th row a label inside the pad [nc, ld), every 11th a negative one"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    lab = torch.randint(0, nc, (rows,), generator=g, device=DEV)
    lab[torch.rand(rows, generator=g, device=DEV) < 0.1] = IGNORE
    r = torch.arange(rows, device=DEV)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = nc - 1                                 # the only row stays a labelled one
    return lab


def _ce_ref(x, lab, nc, sc):
    """fp64: lse, per-row loss, validity, dlogits = sc (softmax - onehot) on labelled rows, and the S of each bound"""
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    lse = torch.logsumexp(x, 1)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    xl = x.gather(1, safe[:, None])[:, 0]
    p = torch.softmax(x, 1)
    oh = F.one_hot(safe, nc).double()
    dl = torch.where(valid[:, None], sc * (p - oh), torch.zeros_like(p))
    S_dl = torch.where(valid[:, None], sc * (p * (x.abs() + lse.abs()[:, None] + 1.0) + oh), torch.zeros_like(p))
    return valid, lse, xl, dl, S_dl


def _run_ld(lib, buf, lab, nc, ld, scale):
    from sigma_amd import _capi
    rows = buf.shape[0]
    glse = _guarded((rows,), 64)
    part = _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2)
    gdl = _guarded((rows, ld), ld)
    _capi.check(lib.sigma_softmax_ce_fwd_ld(_p(buf), _p(lab), rows, nc, ld, IGNORE, _p(glse[1]), _p(part[1]), _stream()), "ce fwd ld")
    _capi.check(lib.sigma_softmax_ce_bwd_ld(_p(buf), _p(lab), _p(glse[1]), _p(scale), rows, nc, ld, IGNORE, _p(gdl[1]), _stream()),
                "ce bwd ld")
    torch.cuda.synchronize()
    return glse, part, gdl


# (rows, classes, ld): 63 / 64 is the last class count held in registers, 65 and 67 / 68 walk the row; (513, 5, 16): a
# pitch above 4 ceil(classes / 4)
CE_LD_CASES = [(3001, 5, 8), (3001, 9, 12), (2 * 9 * 11, 37, 40), (257, 1, 4), (255, 2, 4), (1, 3, 4), (4099, 63, 64),
               (1031, 65, 68), (1031, 67, 68), (513, 5, 16)]


@pytest.mark.parametrize("case", CE_LD_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in CE_LD_CASES])
def test_padded_pitch_kernels_against_fp64(case):
    """Columns >= classes hold NaN in the input: they must reach neither lse nor the partial sums, and the gradient's
    pad is exact zeros.  Labels inside the pad and negative labels count as ignored.  Negative controls (reference code
    only): logsumexp over all ld columns with a zero pad must fail the lse bound; pad labels taken as valid (their
    logit read as the zero of that pad) must fail the bound on the loss sum -- every case with more than 8 rows has such
    labels, the one-row case keeps its row labelled instead."""
    from sigma_amd import _capi
    rows, nc, ld = case
    lib = _capi.load()
    buf = _padded_logits(rows, nc, ld, seed=181)
    lab = _labels(rows, nc, ld, seed=182)
    x = buf[:, :nc].double()
    cnt = float(((lab != IGNORE) & (lab >= 0) & (lab < nc)).sum())
    assert cnt > 0
    scale = torch.tensor([0.7 / cnt], device=DEV)
    glse, part, gdl = _run_ld(lib, buf, lab, nc, ld, scale)
    for gg, w in ((glse, "lse"), (part, "partial"), (gdl, "dlogits")):
        _intact(gg, w)
    valid, lse, xl, dl, S_dl = _ce_ref(x, lab, nc, float(scale))
    S_lse = lse.abs() + 1.0
    r1 = check("cross entropy ld", glse[1], lse, S_lse, nc + 8, "lse")
    loss_rows = torch.where(valid, lse - xl, torch.zeros_like(lse))
    K = -(-rows // (256 * _capi.SIGMA_CE_BLOCKS)) + 8 + nc + 8
    S_loss = torch.where(valid, S_lse + xl.abs(), torch.zeros_like(lse)).sum()
    assert torch.isfinite(part[1]).all(), "NaN of the pad reached the partial sums"
    got_sum = part[1][:, 0].double().sum()
    r2 = check("cross entropy ld", got_sum.view(1), loss_rows.sum().view(1), S_loss.view(1), K, "loss sum")
    assert float(part[1][:, 1].double().sum()) == cnt
    r3 = check("cross entropy ld", gdl[1][:, :nc], dl, S_dl, nc + 16, "dlogits")
    print(f"\n{case}: lse {r1:.3g} loss sum {r2:.3g} dlogits {r3:.3g} of the bound")
    pad = gdl[1][:, nc:]
    assert pad.numel() == rows * (ld - nc) and bool((pad == 0).all()), "pad columns of dlogits are not exact zeros"
    # negative controls
    full = torch.cat([x, torch.zeros(rows, ld - nc, device=DEV, dtype=torch.float64)], 1)
    rejects(glse[1], torch.logsumexp(full, 1), S_lse, nc + 8, "logsumexp over the pad columns")
    in_pad = (lab >= nc) & (lab < ld) & (lab != IGNORE)
    if rows > 8:
        assert bool(in_pad.any())
    if bool(in_pad.any()):
        wrong = loss_rows.sum() + lse[in_pad].sum()                      # lse - 0 for every pad label
        rejects(got_sum.view(1), wrong.view(1), S_loss.view(1), K, "pad labels counted as classes")


@pytest.mark.parametrize("nc", [40, 68])
def test_pitch_equal_to_classes_is_the_contiguous_entry_point(nc):
    """ld == classes: the _ld entry points give the bits of sigma_softmax_ce_fwd / _bwd (register and generic regime)"""
    from sigma_amd import _capi
    lib = _capi.load()
    rows = 3001
    buf = _padded_logits(rows, nc, nc, seed=191)
    lab = _labels(rows, nc, nc, seed=192)
    scale = torch.tensor([0.7 / rows], device=DEV)
    glse, part, gdl = _run_ld(lib, buf, lab, nc, nc, scale)
    lse = torch.full((rows,), float("nan"), device=DEV)
    partial = torch.full((_capi.SIGMA_CE_BLOCKS, 2), float("nan"), device=DEV)
    dlo = torch.full((rows, nc), float("nan"), device=DEV)
    _capi.check(lib.sigma_softmax_ce_fwd(_p(buf), _p(lab), rows, nc, IGNORE, _p(lse), _p(partial), _stream()), "ce fwd")
    _capi.check(lib.sigma_softmax_ce_bwd(_p(buf), _p(lab), _p(lse), _p(scale), rows, nc, IGNORE, _p(dlo), _stream()), "ce bwd")
    torch.cuda.synchronize()
    assert torch.isfinite(lse).all() and torch.isfinite(dlo).all()
    assert torch.equal(glse[1], lse) and torch.equal(part[1], partial) and torch.equal(gdl[1], dlo)


def _image_labels(B, H, W, nc, seed):
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, nc, (B, H, W), generator=g)
    label[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    return label.to(DEV)


@pytest.mark.parametrize("nc", [5, 9, 37])
def test_cross_entropy_takes_the_padded_view(nc):
    """pointwise.cross_entropy on the (B, nc, H, W) view of a (B, H, W, ld) buffer whose pad holds NaN: the loss against
    fp64 F.cross_entropy (rtol 1e-5), the gradient of the valid columns under the dlogits bound of the kernel test, a zero
    gradient in the pad, and the same bits on a second call."""
    from sigma_amd.pointwise import cross_entropy
    B, H, W = 2, 9, 11
    ld = (nc + 3) // 4 * 4
    buf = _padded_logits(B * H * W, nc, ld, seed=201).view(B, H, W, ld).requires_grad_()
    label = _image_labels(B, H, W, nc, seed=202)
    crit = nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    loss = cross_entropy(crit, buf[..., :nc].permute(0, 3, 1, 2), label)
    assert loss is not None
    (loss * 1.7).backward()
    x = buf.detach()[..., :nc].double().reshape(-1, nc)
    want = F.cross_entropy(x, label.view(-1), ignore_index=IGNORE)
    torch.testing.assert_close(loss.detach().double(), want, rtol=1e-5, atol=0.0)
    cnt = float((label != IGNORE).sum())
    _, _, _, dl, S_dl = _ce_ref(x, label.view(-1), nc, 1.7 / cnt)
    g = buf.grad.view(-1, ld)
    check("cross entropy ld", g[:, :nc], dl, S_dl, nc + 16, "gradient of the padded view")
    assert bool((g[:, nc:] == 0).all())
    again = cross_entropy(crit, buf.detach()[..., :nc].permute(0, 3, 1, 2), label)
    assert torch.equal(again, loss.detach())
    # still declined: a plain contiguous tensor of these class counts
    assert cross_entropy(crit, torch.randn(B, H, W, nc, device=DEV).permute(0, 3, 1, 2), label) is None


def _boom(*a, **k):
    raise AssertionError("a vendor GEMM on the classifier route")


def _head_inputs(nc, C, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = 2, 9, 11
    x = torch.randn(B, H, W, C, generator=g).to(DEV)
    w = (torch.randn(nc, C, 1, 1, generator=g) / C ** 0.5).to(DEV)
    return x, w, _image_labels(B, H, W, nc, seed + 1)


def _head_step(x0, w0, label):
    """classifier + loss + backward on the product's route: (logits (M, nc), loss, x.grad, weight.grad)"""
    from sigma_amd import gemm
    from sigma_amd.pointwise import cross_entropy
    x = x0.clone().requires_grad_()
    w = nn.Parameter(w0.clone())
    assert gemm.classifier_ok(x.reshape(-1, x.shape[-1]), w)
    logits = gemm.classifier(x, w)
    loss = cross_entropy(nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE), logits.permute(0, 3, 1, 2), label)
    assert loss is not None
    loss.backward()
    return logits.detach().reshape(-1, w.shape[0]), loss.detach(), x.grad, w.grad


@pytest.mark.parametrize("nc,C", [(5, 96), (9, 96), (37, 96), (5, 128)])
def test_head_runs_on_the_split_gemms_at_the_padded_pitch(nc, C, monkeypatch):
    """x (2, 9, 11, C) through gemm.classifier and the loss, then backward, with torch.mm and F.linear raising: logits,
    x.grad and weight.grad against fp64 linear + cross entropy (the gradient reference uses the fp64 dlogits) under the
    GEMM tests' bound; the logits are the bits of gemm_nt against the unpadded weight; a second run gives the same
    gradient bits (two-stage sums, no atomics); the weight gradient is contiguous in the parameter's shape."""
    from sigma_amd import gemm
    x0, w0, label = _head_inputs(nc, C, seed=211)
    x64, w64 = x0.double().reshape(-1, C), w0.double().view(nc, C)
    z64 = (x64 @ w64.t()).requires_grad_()
    F.cross_entropy(z64, label.view(-1), ignore_index=IGNORE).backward()
    dl64 = z64.grad
    plain = gemm.gemm_nt(x0.reshape(-1, C), w0.view(nc, C))
    with monkeypatch.context() as m:
        m.setattr(torch, "mm", _boom)
        m.setattr(torch.nn.functional, "linear", _boom)
        logits, loss, dx, dw = _head_step(x0, w0, label)
        logits2, loss2, dx2, dw2 = _head_step(x0, w0, label)
        torch.cuda.synchronize()
    _assert_close(logits, z64.detach(), _bound(x64, w64.t()), "logits")
    assert torch.equal(logits, plain), "logits differ from gemm_nt against the unpadded weight"
    _assert_close(dx.reshape(-1, C), dl64 @ w64, _bound(dl64, w64), "x.grad")
    _assert_close(dw.view(nc, C), dl64.t() @ x64, _bound(dl64.t(), x64), "weight.grad")
    assert dw.is_contiguous() and tuple(dw.shape) == (nc, C, 1, 1) and dw.stride() == w0.stride()
    assert torch.equal(loss, loss2) and torch.equal(dx, dx2) and torch.equal(dw, dw2)


@pytest.mark.parametrize("nc", [5, 9, 37])
def test_head_gradient_from_elsewhere_takes_the_copying_path(nc, monkeypatch):
    """logits.backward(g) with a contiguous (B, nc, H, W) g: nobody handed a padded buffer over, so the classifier's
    backward copies g into a zero-padded one.  The pad of the forward's buffer is filled with NaN first: nothing may
    read it.  Same bound."""
    from sigma_amd import gemm
    C = 96
    x0, w0, _ = _head_inputs(nc, C, seed=221)
    B, H, W = x0.shape[:3]
    g = torch.randn(B, nc, H, W, generator=torch.Generator().manual_seed(222)).to(DEV)
    x = x0.clone().requires_grad_()
    w = nn.Parameter(w0.clone())
    with monkeypatch.context() as m:
        m.setattr(torch, "mm", _boom)
        m.setattr(torch.nn.functional, "linear", _boom)
        logits = gemm.classifier(x, w)
        ld = gemm.padded_classes(nc)
        assert logits.stride() == (H * W * ld, W * ld, ld, 1)
        # .data: an alias with a version counter of its own (autograd refuses in-place writes through a view that a
        # custom Function returned)
        whole = torch.as_strided(logits.data, (B * H * W, ld), (ld, 1))
        assert bool((whole[:, nc:] == 0).all()), "pad columns of the logits buffer are not exact zeros"
        whole[:, nc:] = float("nan")
        logits.permute(0, 3, 1, 2).backward(g)
        torch.cuda.synchronize()
    x64, w64 = x0.double().reshape(-1, C), w0.double().view(nc, C)
    g64 = g.double().permute(0, 2, 3, 1).reshape(-1, nc)
    _assert_close(x.grad.reshape(-1, C), g64 @ w64, _bound(g64, w64), "x.grad")
    _assert_close(w.grad.view(nc, C), g64.t() @ x64, _bound(g64.t(), x64), "weight.grad")
    assert w.grad.is_contiguous() and tuple(w.grad.shape) == (nc, C, 1, 1)


CE_SYMBOLS = ("sigma_softmax_ce_fwd", "sigma_softmax_ce_bwd", "sigma_softmax_ce_fwd_ld", "sigma_softmax_ce_bwd_ld")


class _Counting:
    """stands in for the ctypes library: counts the calls of the loss entry points by name, forwards everything"""

    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in CE_SYMBOLS:
            return fn

        def call(*args):
            self._counts[name] += 1
            return fn(*args)
        return call


@pytest.mark.parametrize("nc", [9, 40])
def test_model_step_calls_the_entry_points_of_its_class_count(nc, monkeypatch):
    """sigma_tiny 64x96, batch 1, train mode, one forward + backward: 9 classes call sigma_softmax_ce_fwd_ld / _bwd_ld once
    each and the contiguous entry points never; 40 classes the other way round.  The loss is finite, every parameter has
    a gradient, the classifier's is contiguous in the parameter's shape, and the model grew no parameter or buffer."""
    from sigma_amd import _capi
    from tests.model_utils import build_model, fill
    model = build_model("sigma_tiny", nc, 64, 96).cuda().train()
    keys = sorted(model.state_dict())
    rgb, x, label = fill.make_inputs(1, 64, 96, nc, seed=5)
    counts = collections.Counter()
    rec = _Counting(_capi.load(), counts)
    monkeypatch.setattr(_capi, "load", lambda: rec)
    loss = model(rgb.cuda(), x.cuda(), label.cuda())
    loss.backward()
    torch.cuda.synchronize()
    new, old = CE_SYMBOLS[2:], CE_SYMBOLS[:2]
    used, unused = (new, old) if nc % 4 else (old, new)
    assert [counts[s] for s in used] == [1, 1] and [counts[s] for s in unused] == [0, 0], dict(counts)
    assert torch.isfinite(loss)
    missing = [n for n, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    gw = model.decode_head.output.weight.grad
    assert gw.is_contiguous() and tuple(gw.shape) == (nc, 96, 1, 1) and torch.isfinite(gw).all()
    assert sorted(model.state_dict()) == keys
    model.eval()
    with torch.no_grad():
        out = model(rgb.cuda(), x.cuda())
    assert out.is_contiguous() and tuple(out.shape) == (1, nc, 64, 96)
