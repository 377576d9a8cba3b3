"""ChannelAttention's gate and the segmentation loss on the HIP streams of csrc/pointwise.hip (C ABI: include/sigma_ops.h).

``channel_gate``   y = x * sigmoid(fc(mean(x)) + fc(amax(x)))  for contiguous (B, C, H, W) fp32 activations
                   (ChannelAttention, vmamba.py:1725-1741): one pooling pass, the (2B, C) squeeze/excite MLP in torch,
                   one scaling pass; backward = one plane dot product, the MLP's autograd on (2B, C) tensors, one pass
                   that writes dx.
``cross_entropy``  nn.CrossEntropyLoss(reduction='mean', ignore_index) of models/builder.py:146-166 on the CHANNELS-LAST
                   logits the classifier GEMM produces (MambaDecoder.up_x4): log-sum-exp + loss in one pass, gradient in
                   one pass, no (B, classes, H, W) copy (``SoftmaxCEFn``).  Class weights, label smoothing and the
                   reductions 'sum' / 'none' run on the option kind of the same kernels (``SoftmaxCEOptFn``).
``ohem_cross_entropy``  ProbOhemCrossEntropy2d (utils/loss_opr.py:137-187) on the same logits: the forward of the option
                   kernels writes the per-pixel loss, csrc/ohem.hip selects the hard pixels on the device (a radix select
                   of the min_kept-th largest loss; no host round trip) and the backward of the option kernels runs on
                   the mined labels (``OhemCEFn``).
``focal_cross_entropy``  FocalLoss2d (utils/loss_opr.py:12-23) with a run-time exponent on the same logits: the focal kind
                   of the same kernels (``SoftmaxFocalFn``).

``upsampled_cross_entropy``  the plain mean cross entropy of the bilinear x s upsampling of COARSE channels-last logits --
                   the loss of a deep-supervision head (MambaDecoder.forward_deep) -- with the interpolation inside the
                   loss kernels of csrc/deepsup.hip: no full-size logits exist in either direction (``UpsampledLossFn``, kind
                   "plain").

``upsampled_loss``  the same for the criteria with options -- class weights, label smoothing, 'sum' / 'none', FocalLoss2d and
                   ProbOhemCrossEntropy2d -- on sigma_upsample_loss_fwd / _bwd and, for OHEM, the selection kernels in
                   between (the other kinds of ``UpsampledLossFn``).

``region_loss``    a soft region-overlap loss -- Dice, Jaccard, Tversky, optionally summed with the mean cross entropy -- on the
                   same logits: per-class sums without atomics, the coefficient table on the device, a one-pass backward
                   (csrc/region.hip, C ABI include/sigma_region.h bound by ``_capi_region``; ``RegionLossFn``).

``distill_loss``   the distillation loss against a frozen teacher's logits of the same layout (either pitch each): the KL
                   divergence at a temperature, optionally summed with the mean cross entropy; both rows in registers, sums
                   without atomics, the two scale factors on the device, a one-pass backward (csrc/distill.hip, C ABI
                   include/sigma_distill.h bound by ``_capi_distill``; ``DistillLossFn``).  The teacher gets no gradient.

The three front-ends share their checks (``_loss_rows``); the three Functions with options share one forward
(``_rows_forward`` / ``_rows_finish``: buffers, parameters, saved tensors, reduction) and one backward (``_dlogits``), and
differ in the entry point they name.

GPU tensors only (no fallback); the callers keep the torch formulation for everything these kernels do not take.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi
from ._handoff import offer_padded_grad_buffer
from ._launch import launch, ptr
from ._launch import workspace as _workspace


def _mlp(pooled, w1, w2, batch):
    """fc of ChannelAttention on the stacked [mean; max] rows: conv1x1 - SiLU - conv1x1 (no biases), summed halves"""
    g = F.linear(F.silu(F.linear(pooled, w1)), w2)
    return g[:batch] + g[batch:]


class ChannelGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2):
        B, C, H, W = x.shape
        planes, hw = B * C, H * W
        w1m, w2m = w1.reshape(w1.shape[0], -1), w2.reshape(w2.shape[0], -1)
        pooled = torch.empty(2 * planes, device=x.device, dtype=torch.float32)       # [mean (B, C); max (B, C)]
        cnt = torch.empty(planes, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            launch("sigma_plane_pool", ptr(x), planes, hw, ptr(pooled), ptr(pooled[planes:]), ptr(cnt), device=x.device,
                   what="plane_pool")
            s = torch.sigmoid(_mlp(pooled.view(2 * B, C), w1m, w2m, B)).contiguous()
            y = torch.empty_like(x)
            launch("sigma_plane_scale", ptr(x), ptr(s), ptr(y), planes, hw, device=x.device, what="plane_scale")
        ctx.save_for_backward(x, w1, w2, pooled, cnt, s)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w1, w2, pooled, cnt, s = ctx.saved_tensors
        B, C, H, W = x.shape
        planes, hw = B * C, H * W
        g = g.float().contiguous()
        with torch.cuda.device(x.device):
            ds = torch.empty(B, C, device=x.device, dtype=torch.float32)
            launch("sigma_plane_dot", ptr(g), ptr(x), ptr(ds), planes, hw, device=x.device, what="plane_dot")
            # the (2B, C) squeeze/excite MLP and the sigmoid by hand on tiny tensors (no nested autograd: the step is
            # captured into HIP graphs):  h = P W1^T, a = silu(h), g = a W2^T, gate = g[:B] + g[B:], s = sigmoid(gate)
            w1m, w2m = w1.reshape(w1.shape[0], -1), w2.reshape(w2.shape[0], -1)
            P2 = pooled.view(2 * B, C)
            h = F.linear(P2, w1m)
            sh = torch.sigmoid(h)
            a = h * sh
            dgate = ds * s * (1.0 - s)
            dg = torch.cat([dgate, dgate], dim=0)                       # (2B, C)
            dw2 = (dg.t() @ a).view_as(w2)
            dh = (dg @ w2m) * (sh * (1.0 + h * (1.0 - sh)))
            dw1 = (dh.t() @ P2).view_as(w1)
            dpl = dh @ w1m
            dpl = dpl.contiguous()
            dx = torch.empty_like(x)
            p = _capi.GateBwdParams()
            p.planes, p.hw = planes, hw
            p.g, p.x, p.scale, p.dx = g.data_ptr(), x.data_ptr(), s.data_ptr(), dx.data_ptr()
            p.dmean, p.dmax = dpl.data_ptr(), dpl[B:].data_ptr()
            p.max, p.count = pooled[planes:].data_ptr(), cnt.data_ptr()
            launch("sigma_plane_gate_bwd", ctypes.byref(p), device=x.device, what="plane_gate_bwd")
        return dx, dw1, dw2


def channel_gate_ok(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.numel() > 0
            and w1.dtype == torch.float32 and w2.dtype == torch.float32)


def channel_gate(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """x (B, C, H, W) contiguous; w1 (C/r, C, 1, 1), w2 (C, C/r, 1, 1): the two bias-free 1x1 convolutions of fc"""
    if not channel_gate_ok(x, w1, w2):
        raise RuntimeError("channel_gate: contiguous fp32 (B, C, H, W) GPU tensors only (no fallback)")
    return ChannelGateFn.apply(x, w1, w2)


class ScaleResidualFn(torch.autograd.Function):
    """a + x * scale with a per-channel scale on channels-last tensors -- the two residuals of the decoder block,
    ``x * scale1 + op(norm1(x))`` and ``x * scale2 + conv_blk(norm2(x))`` (vmamba.py:1800-1805).  Forward: torch's
    addcmul (one pass); backward: ONE pass over dy and x for dx = dy * scale and dscale = sum dy * x
    (sigma_colscale_bwd) instead of two multiplies and a column reduction, and dy itself for the branch."""

    @staticmethod
    def forward(ctx, a, x, scale):
        ctx.save_for_backward(x, scale)
        return torch.addcmul(a, x, scale)

    @staticmethod
    def backward(ctx, dy):
        x, scale = ctx.saved_tensors
        C = x.shape[-1]
        g = dy.contiguous()
        if g.data_ptr() % 16:                       # a packed gradient off a 16-byte boundary (a slice of a larger buffer):
            g = g.clone()                           # the kernels load 16 bytes per lane and refuse it
        xc = x.contiguous()
        dx = torch.empty_like(xc)
        if torch.are_deterministic_algorithms_enabled():
            # deterministic mode (sigma_amd/deterministic.py): per-block column sums, added in a fixed order; ds is written
            rows = xc.numel() // C
            ws_bytes = int(_capi.load().sigma_colscale_bwd_workspace_bytes(rows, C))
            ws = torch.empty(max(ws_bytes, 16), device=x.device, dtype=torch.uint8)
            ds = torch.empty(C, device=x.device, dtype=torch.float32)
            launch("sigma_colscale_bwd_ws", ptr(g), ptr(xc), ptr(scale), ptr(dx), ptr(ds), rows, C, ptr(ws), ws_bytes,
                   device=x.device, what="colscale_bwd_ws")
            return dy, dx, ds
        ds = torch.zeros(C, device=x.device, dtype=torch.float32)
        launch("sigma_colscale_bwd", ptr(g), ptr(xc), ptr(scale), ptr(dx), ptr(ds), xc.numel() // C, C, device=x.device,
               what="colscale_bwd")
        return dy, dx, ds


def scale_residual_ok(a: torch.Tensor, x: torch.Tensor, scale: torch.Tensor) -> bool:
    C = x.shape[-1] if x.dim() else 0
    return (a.is_cuda and x.is_cuda and a.dtype == torch.float32 and x.dtype == torch.float32 and scale.dtype == torch.float32
            and tuple(a.shape) == tuple(x.shape) and tuple(scale.shape) == (C,) and C % 4 == 0 and 0 < C <= 1024
            and x.is_contiguous() and x.data_ptr() % 16 == 0 and scale.data_ptr() % 16 == 0 and x.numel() > 0)


def scale_residual(a: torch.Tensor, x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """a + x * scale (channel-wise) -- on the fused backward where it applies, torch.addcmul otherwise"""
    if scale_residual_ok(a, x, scale) and torch.is_grad_enabled() and (x.requires_grad or scale.requires_grad or a.requires_grad):
        return ScaleResidualFn.apply(a, x, scale)
    return torch.addcmul(a, x, scale)


def _hand_off_padded(full, nc):
    """The gradient a loss backward returns for logits of `nc` classes, from the buffer `full` (rows, ld) its kernel
    wrote: at a padded pitch the classifier's backward claims the WHOLE buffer for its GEMMs (_handoff.py) and autograd
    gets the view of the first `nc` columns"""
    if full.shape[1] != nc:
        offer_padded_grad_buffer(full)
        full = full[:, :nc]
    return full


class SoftmaxCEFn(torch.autograd.Function):
    """mean over the non-ignored pixels of -log softmax(logits)[label]; logits2 (rows, classes) with contiguous rows at a
    pitch of `ld` floats: the class count itself (sigma_softmax_ce_fwd / _bwd), or a multiple of 4 above it
    (the padded buffer of gemm.ClassifierPadFn; sigma_softmax_ce_fwd_ld / _bwd_ld, the pad is never read)"""

    @staticmethod
    def _call(direction, ld, nc, before, after, device):
        """sigma_softmax_ce_<direction>(*before, nc, *after, stream), or its _ld form with the pitch after the class count"""
        name, pitch = (f"softmax_ce_{direction}", ()) if ld == nc else (f"softmax_ce_{direction}_ld", (ld,))
        launch("sigma_" + name, *before, nc, *pitch, *after, device=device, what=name)

    @staticmethod
    def forward(ctx, logits2, labels, ignore_index, ld):
        rows, nc = logits2.shape
        lse = torch.empty(rows, device=logits2.device, dtype=torch.float32)
        partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=logits2.device, dtype=torch.float32)
        SoftmaxCEFn._call("fwd", ld, nc, (ptr(logits2), ptr(labels), rows), (int(ignore_index), ptr(lse), ptr(partial)),
                          logits2.device)
        tot = partial.sum(0)
        ctx.save_for_backward(logits2, labels, lse, tot)
        ctx.ignore_index, ctx.ld = int(ignore_index), ld
        return tot[0] / tot[1]

    @staticmethod
    def backward(ctx, g):
        logits2, labels, lse, tot = ctx.saved_tensors
        rows, nc = logits2.shape
        ld = ctx.ld
        scale = (g.float() / tot[1]).reshape(1).contiguous()
        # the gradient at the logits' pitch, pad columns written with zeros: the classifier's backward claims the whole
        # buffer for its GEMMs (_handoff.py) -- no zero fill, no re-laying copy
        full = torch.empty_like(logits2) if ld == nc else torch.empty((rows, ld), device=logits2.device, dtype=torch.float32)
        SoftmaxCEFn._call("bwd", ld, nc, (ptr(logits2), ptr(labels), ptr(lse), ptr(scale), rows), (ctx.ignore_index, ptr(full)),
                          logits2.device)
        return _hand_off_padded(full, nc), None, None, None


def _row_pitch(nhwc: torch.Tensor):
    """the pitch ld (floats) if `nhwc` (B, H, W, nc) is B*H*W rows of nc contiguous floats ld apart, else None"""
    B, H, W, nc = nhwc.shape
    sb, sh, sw, sc = nhwc.stride()
    if nhwc.numel() == 0 or (nc > 1 and sc != 1):
        return None
    ld = sw if W > 1 else sh if H > 1 else sb if B > 1 else (nc + 3) // 4 * 4
    if (W > 1 and sw != ld) or (H > 1 and sh != W * ld) or (B > 1 and sb != H * W * ld):
        return None
    return ld


def _rows_forward(ctx, kind, extra, logits2, labels, weight, ignore_index, ld, eps, reduction, out_shape):
    """The forward of ``SoftmaxCEOptFn`` (kind "ce_opt") and ``SoftmaxFocalFn`` ("focal"): sigma_softmax_<kind>_fwd(params,
    *extra, stream) into a new lse, the partial pairs and, for 'none', the row losses; then ``_rows_finish``"""
    rows = logits2.shape[0]
    dev = logits2.device
    lse = torch.empty(rows, device=dev, dtype=torch.float32)
    partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=dev, dtype=torch.float32)
    row_loss = torch.empty(rows, device=dev, dtype=torch.float32) if reduction == "none" else None
    p = SoftmaxCEOptFn._params(logits2, labels, weight, lse, ignore_index, ld, eps)
    p.partial = partial.data_ptr()
    p.row_loss = row_loss.data_ptr() if row_loss is not None else None
    launch(f"sigma_softmax_{kind}_fwd", ctypes.byref(p), *extra, device=dev, what=f"softmax_{kind}_fwd")
    return _rows_finish(ctx, kind, extra, logits2, labels, weight, lse, partial, row_loss, ignore_index, ld, eps, reduction, out_shape)


def _rows_finish(ctx, kind, extra, logits2, labels, weight, lse, partial, row_loss, ignore_index, ld, eps, reduction, out_shape):
    """What the three loss Functions do with the outputs of their forward kernels: save what ``_dlogits`` takes -- `labels`
    are the labels the backward runs on, `kind` and `extra` name its entry point -- and reduce: 'mean' divides the summed
    row losses by the summed weights of the labelled pixels ON THE DEVICE, 'sum' returns the sum, 'none' the per-pixel
    losses in `out_shape`"""
    tot = partial.sum(0)
    ctx.save_for_backward(logits2, labels, lse, tot, weight)
    ctx.ignore_index, ctx.ld, ctx.eps, ctx.reduction = int(ignore_index), ld, float(eps), reduction
    ctx.kind, ctx.extra = kind, extra
    if reduction == "none":
        return row_loss.view(out_shape)
    return tot[0] / tot[1] if reduction == "mean" else tot[0].clone()


def _dlogits(ctx, g):
    """The backward of the three loss Functions: sigma_softmax_<ctx.kind>_bwd(params, *ctx.extra, stream) on what
    ``_rows_finish`` saved, into a new gradient buffer at the logits' pitch"""
    logits2, labels, lse, tot, weight = ctx.saved_tensors
    rows, nc = logits2.shape
    ld = ctx.ld
    p = SoftmaxCEOptFn._params(logits2, labels, weight, lse, ctx.ignore_index, ld, ctx.eps)
    if ctx.reduction == "none":
        grad = g.float().contiguous().view(-1)
        p.row_grad = grad.data_ptr()
    else:
        grad = g.float().reshape(1)
        if ctx.reduction == "mean":
            grad = torch.where(tot[1:2] > 0, grad / tot[1:2], torch.zeros_like(grad))      # zero denominator: zero gradient
        grad = grad.contiguous()
        p.scale = grad.data_ptr()
    full = torch.empty((rows, ld), device=logits2.device, dtype=torch.float32)
    p.dlogits = full.data_ptr()
    launch(f"sigma_softmax_{ctx.kind}_bwd", ctypes.byref(p), *ctx.extra, device=logits2.device,
           what=f"softmax_{ctx.kind}_bwd")
    return _hand_off_padded(full, nc)


class SoftmaxCEOptFn(torch.autograd.Function):
    """nn.CrossEntropyLoss with class weights, label smoothing and any reduction on the same rows as ``SoftmaxCEFn``
    (sigma_softmax_ce_opt_fwd / _bwd, either pitch).  'mean' divides the summed row losses by the summed weights of the
    labelled pixels ON THE DEVICE; 'sum' returns the sum; 'none' the per-pixel losses in `out_shape` (zeros at ignored
    pixels).  The weight gets no gradient, as in torch.  A zero denominator ('mean' with nothing labelled, or only
    zero-weight classes) gives a NaN loss (0 / 0), as ``SoftmaxCEFn`` does, and an all-zero gradient."""

    @staticmethod
    def _params(logits2, labels, weight, lse, ignore_index, ld, eps):
        p = _capi.CeOptParams()
        p.rows, p.classes, p.ld = logits2.shape[0], logits2.shape[1], ld
        p.ignore_index, p.label_smoothing = int(ignore_index), float(eps)
        p.logits, p.labels, p.lse = logits2.data_ptr(), labels.data_ptr(), lse.data_ptr()
        p.weight = weight.data_ptr() if weight is not None else None
        return p

    @staticmethod
    def forward(ctx, logits2, labels, weight, ignore_index, ld, eps, reduction, out_shape):
        return _rows_forward(ctx, "ce_opt", (), logits2, labels, weight, ignore_index, ld, eps, reduction, out_shape)

    @staticmethod
    def backward(ctx, g):
        return (_dlogits(ctx, g),) + (None,) * 7


def ohem_stages(logits2, labels, weight, ignore_index, ld, thresh, min_kept, want_row_loss=False):
    """The forward of the OHEM route on (rows, classes) logits at pitch `ld`, no autograd: (1) the unweighted
    sigma_softmax_ce_opt_fwd with a row loss -- lse and nll = lse - x_y, the one pass over the logits; (2) sigma_ohem_select
    on nll: tau, (num_valid, kept), the mined labels and, from nll, `weight` and the mined labels alone, the row losses
    and the SIGMA_CE_BLOCKS partial pairs of the weighted cross entropy on them.  Returns a dict of device tensors;
    nothing is read back."""
    rows = logits2.shape[0]
    dev = logits2.device
    f32 = dict(device=dev, dtype=torch.float32)
    lse, nll = torch.empty(rows, **f32), torch.empty(rows, **f32)
    partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, **f32)
    p = SoftmaxCEOptFn._params(logits2, labels, None, lse, ignore_index, ld, 0.0)
    p.row_loss, p.partial = nll.data_ptr(), partial.data_ptr()
    launch("sigma_softmax_ce_opt_fwd", ctypes.byref(p), device=dev, what="softmax_ce_opt_fwd (ohem nll)")
    r = _ohem_select(nll, labels, weight, ignore_index, logits2.shape[1], thresh, min_kept, partial, want_row_loss)
    return dict(lse=lse, nll=nll, partial=partial, **r)


def _ohem_select(nll, labels, weight, ignore_index, nc, thresh, min_kept, partial, want_row_loss):
    """sigma_ohem_select on the flat per-pixel `nll` and `labels` of `nc` classes: new mined labels, tau, counts and (on
    request) the row losses; `partial` is OVERWRITTEN with the pairs of the weighted cross entropy on the mined labels (the
    unweighted sums of the nll pass are not used).  Returns a dict of device tensors; nothing is read back."""
    lib = _capi.load()
    rows = nll.numel()
    dev = nll.device
    mined = torch.empty(rows, device=dev, dtype=torch.int64)
    tau = torch.empty(1, device=dev, dtype=torch.float32)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    row_loss = torch.empty(rows, device=dev, dtype=torch.float32) if want_row_loss else None
    ws_bytes = int(lib.sigma_ohem_workspace_bytes(rows))
    if ws_bytes < 0:
        raise RuntimeError(f"ohem: {rows} rows are more than the selection takes (2^31 - 1)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    q = _capi.OhemParams()
    q.rows, q.ignore_index, q.classes, q.thresh, q.min_kept = rows, int(ignore_index), nc, float(thresh), int(min_kept)
    q.nll, q.labels, q.mined, q.tau, q.counts = nll.data_ptr(), labels.data_ptr(), mined.data_ptr(), tau.data_ptr(), counts.data_ptr()
    q.workspace, q.workspace_bytes = ws.data_ptr(), ws_bytes
    q.weight = weight.data_ptr() if weight is not None else None
    q.row_loss = row_loss.data_ptr() if row_loss is not None else None
    q.partial = partial.data_ptr()
    launch("sigma_ohem_select", ctypes.byref(q), device=dev, what="ohem_select")
    return dict(mined=mined, tau=tau, counts=counts, row_loss=row_loss)


class OhemCEFn(torch.autograd.Function):
    """ProbOhemCrossEntropy2d on the rows of ``SoftmaxCEOptFn``: ``ohem_stages`` in the forward (the logits are read once;
    the selection carries no gradient), sigma_softmax_ce_opt_bwd on the mined labels with the saved lse in the backward.
    Reductions and the zero denominator as in ``SoftmaxCEOptFn``."""

    @staticmethod
    def forward(ctx, logits2, labels, weight, ignore_index, ld, thresh, min_kept, reduction, out_shape):
        r = ohem_stages(logits2, labels, weight, ignore_index, ld, thresh, min_kept, want_row_loss=reduction == "none")
        return _rows_finish(ctx, "ce_opt", (), logits2, r["mined"], weight, r["lse"], r["partial"], r["row_loss"], ignore_index, ld, 0.0,
                            reduction, out_shape)

    @staticmethod
    def backward(ctx, g):
        return (_dlogits(ctx, g),) + (None,) * 8


class SoftmaxFocalFn(torch.autograd.Function):
    """FocalLoss2d on the rows of ``SoftmaxCEOptFn``: w_y (1 - p_y)^gamma (lse - x_y) per pixel (sigma_softmax_focal_fwd /
    _bwd, either pitch; gamma = 0 or >= 1).  Reductions, the device-side 'mean', the zero denominator and the hand-off of
    the padded gradient buffer as in ``SoftmaxCEOptFn``."""

    @staticmethod
    def forward(ctx, logits2, labels, weight, ignore_index, ld, gamma, reduction, out_shape):
        return _rows_forward(ctx, "focal", (float(gamma),), logits2, labels, weight, ignore_index, ld, 0.0, reduction, out_shape)

    @staticmethod
    def backward(ctx, g):
        return (_dlogits(ctx, g),) + (None,) * 7


UPSAMPLED_CE_MAX_CLASSES = 64      # include/sigma_ops.h: sigma_upsample_ce_params.classes
UPSAMPLED_CE_MAX_SCALE = 32


def upsampled_cross_entropy(criterion, coarse: torch.Tensor, scale: int, label: torch.Tensor):
    """criterion(upsample(coarse), label) for the bilinear x `scale` upsampling (align_corners=False) of channels-last
    logits `coarse` (B, h, w, classes), without the upsampled tensor (``UpsampledLossFn``, kind "plain") -- or None when this route does
    not apply: anything but the plain criterion (``criterion_route(...) == "plain"``: weights, smoothing, 'sum' / 'none',
    OHEM and focal take the expansion, MambaDecoder.expand_logits), logits that are not fp32 GPU rows at a pitch
    ``_row_pitch`` accepts (a multiple of 4, 16-byte aligned, every row's last 16-byte chunk inside the storage), more than 64 classes, a scale outside [1, 32], a label that
    is not on the logits' device with the shape (B, h scale, w scale).  Labels outside [0, classes) count as ignored, as in
    ``cross_entropy``."""
    if coarse.dim() != 4 or criterion_route(criterion, coarse.device, coarse.shape[3]) != "plain":
        return None
    args = _upsampled_rows(coarse, scale, label)
    if args is None:
        return None
    logits2, labels, ld, dims = args
    return UpsampledLossFn.apply(logits2, labels, None, criterion.ignore_index, ld, dims, "plain", 0.0, "mean")


def _upsampled_rows(coarse, scale, label):
    """What the two upsampled front ends hand to ``UpsampledLossFn``: (logits2, labels, ld, dims) -- the (B h w, classes) view of
    the coarse logits at its pitch `ld`, the contiguous int64 labels (B, h scale, w scale), dims = (B, h, w, scale) -- or None
    for what the kernels of csrc/deepsup.hip do not take (the list in ``upsampled_cross_entropy``)"""
    if coarse.dim() != 4 or label.dim() != 3 or not (coarse.is_cuda and coarse.dtype == torch.float32):
        return None
    B, h, w, nc = coarse.shape
    scale = int(scale)
    if not 1 <= nc <= UPSAMPLED_CE_MAX_CLASSES:
        return None
    if not 1 <= scale <= UPSAMPLED_CE_MAX_SCALE or label.device != coarse.device or tuple(label.shape) != (B, h * scale, w * scale):
        return None
    ld = nc if coarse.is_contiguous() and nc % 4 == 0 else _row_pitch(coarse)
    if ld is None or ld % 4 != 0 or ld < nc or coarse.data_ptr() % 16 != 0 or coarse.numel() == 0 or label.numel() >= 2 ** 31:
        return None
    # the kernels load whole 16-byte chunks: the last row is read up to column 4 ceil(nc / 4).  A pitch inferred for a
    # single row (``_row_pitch``: strides say nothing there) must lie inside the tensor's storage, else a packed
    # (1, 1, 1, nc) tensor with nc % 4 != 0 would be read past its end
    floats = (B * h * w - 1) * ld + (nc + 3) // 4 * 4
    if coarse.storage_offset() + floats > coarse.untyped_storage().nbytes() // coarse.element_size():
        return None
    return coarse.reshape(-1, nc), label.long().contiguous(), ld, (B, h, w, scale)


def upsampled_ohem_stages(logits2, labels, weight, ignore_index, ld, dims, thresh, min_kept, want_row_loss=False):
    """``ohem_stages`` for coarse logits2 (B h w, classes) at pitch `ld` and labels (B, h s, w s), dims = (B, h, w, s), no
    autograd: (1) the unweighted sigma_upsample_loss_fwd with a row loss -- lse and nll = lse - z^_y per fine pixel; (2)
    sigma_ohem_select on nll, exactly as for full-size logits.  Returns the dict of ``ohem_stages`` (mined in the labels'
    shape, row_loss flat); nothing is read back."""
    dev = logits2.device
    lse = torch.empty(labels.shape, device=dev, dtype=torch.float32)
    nll = torch.empty(labels.shape, device=dev, dtype=torch.float32)
    partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=dev, dtype=torch.float32)
    name, p = UpsampledLossFn._params("options", logits2, labels, None, lse, None, dims, ignore_index, ld, 0.0)
    p.partial, p.row_loss = partial.data_ptr(), nll.data_ptr()
    launch(f"sigma_{name}_fwd", ctypes.byref(p), device=dev, what=f"{name}_fwd (ohem nll)")
    r = _ohem_select(nll.view(-1), labels.view(-1), weight, ignore_index, logits2.shape[1], thresh, min_kept, partial, want_row_loss)
    r["mined"] = r["mined"].view(labels.shape)
    return dict(lse=lse, nll=nll, partial=partial, **r)


class UpsampledLossFn(torch.autograd.Function):
    """Every criterion of a deep-supervision head on coarse logits2 (B h w, classes) at a pitch of `ld` floats and labels
    (B, h s, w s), dims = (B, h, w, s): the kernels of csrc/deepsup.hip.  `kind` "plain" (the mean cross entropy: no weight,
    reduction 'mean'; sigma_upsample_ce_fwd / _bwd), or, on sigma_upsample_loss_fwd / _bwd, "options" (class weights, label
    smoothing `x`), "focal" (exponent `x`, 0 or >= 1) or "ohem" (`x` = (thresh, min_kept)): the forward of the options
    without weight writes the per-pixel nll, sigma_ohem_select mines the labels on the device -- the stages of
    ``ohem_stages`` -- and the backward of the options runs on the mined labels with the weight.  Reductions as in
    ``SoftmaxCEOptFn``: 'mean' divides by the summed weights ON THE DEVICE, a zero denominator (nothing labelled) gives a
    NaN loss and an all-zero gradient; 'none' returns the per-pixel losses (B, h s, w s).  Saved for the backward: the coarse
    logits, the (mined) labels, lse and, for focal, coef per fine pixel.  Nothing is read back."""

    @staticmethod
    def _params(kind, logits2, labels, weight, lse, coef, dims, ignore_index, ld, x):
        """(name, params) of `kind` ("plain", "options" or "focal"): sigma_<name>_fwd / _bwd take `params`"""
        plain, focal = kind == "plain", kind == "focal"
        p = _capi.UpsampleCeParams() if plain else _capi.UpsampleLossParams()
        p.batch, p.height, p.width, p.scale = dims
        p.classes, p.ld, p.ignore_index = logits2.shape[1], ld, int(ignore_index)
        p.logits, p.labels, p.lse = logits2.data_ptr(), labels.data_ptr(), lse.data_ptr()
        if plain:
            return "upsample_ce", p
        p.kind = _capi.SIGMA_UPSAMPLE_LOSS_FOCAL if focal else _capi.SIGMA_UPSAMPLE_LOSS_OPTIONS
        p.label_smoothing, p.gamma = (0.0, float(x)) if focal else (float(x), 0.0)
        p.weight = weight.data_ptr() if weight is not None else None
        p.coef = coef.data_ptr() if coef is not None else None
        return "upsample_loss", p

    @staticmethod
    def forward(ctx, logits2, labels, weight, ignore_index, ld, dims, kind, x, reduction):
        dev = logits2.device
        f32 = dict(device=dev, dtype=torch.float32)
        coef = None
        if kind == "ohem":
            r = upsampled_ohem_stages(logits2, labels, weight, ignore_index, ld, dims, x[0], x[1], want_row_loss=reduction == "none")
            labels, lse, partial, row_loss, kind, x = r["mined"], r["lse"], r["partial"], r["row_loss"], "options", 0.0
        else:
            lse = torch.empty(labels.shape, **f32)
            partial = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, **f32)
            coef = torch.empty(labels.shape, **f32) if kind == "focal" else None
            row_loss = torch.empty(labels.shape, **f32) if reduction == "none" else None
            name, p = UpsampledLossFn._params(kind, logits2, labels, weight, lse, coef, dims, ignore_index, ld, x)
            p.partial = partial.data_ptr()
            if row_loss is not None:
                p.row_loss = row_loss.data_ptr()
            launch(f"sigma_{name}_fwd", ctypes.byref(p), device=dev, what=f"{name}_fwd ({kind})")
        tot = partial.sum(0)
        ctx.save_for_backward(logits2, labels, lse, tot, weight, coef)
        ctx.ignore_index, ctx.ld, ctx.dims, ctx.reduction = int(ignore_index), ld, dims, reduction
        ctx.kind, ctx.x = kind, float(x)
        if reduction == "none":
            return row_loss.view(labels.shape)
        return tot[0] / tot[1] if reduction == "mean" else tot[0].clone()

    @staticmethod
    def backward(ctx, g):
        logits2, labels, lse, tot, weight, coef = ctx.saved_tensors
        rows, nc = logits2.shape
        ld = ctx.ld
        name, p = UpsampledLossFn._params(ctx.kind, logits2, labels, weight, lse, coef, ctx.dims, ctx.ignore_index, ld, ctx.x)
        if ctx.reduction == "none":
            grad = g.float().contiguous().view(-1)
            p.row_grad = grad.data_ptr()
        else:
            grad = g.float().reshape(1)
            if ctx.reduction == "mean":
                grad = torch.where(tot[1:2] > 0, grad / tot[1:2], torch.zeros_like(grad))      # zero denominator: zero gradient
            grad = grad.contiguous()
            p.scale_grad = grad.data_ptr()
        full = torch.empty((rows, ld), device=logits2.device, dtype=torch.float32)
        p.dlogits = full.data_ptr()
        launch(f"sigma_{name}_bwd", ctypes.byref(p), device=logits2.device, what=f"{name}_bwd ({ctx.kind})")
        return (_hand_off_padded(full, nc),) + (None,) * 8


def upsampled_loss(criterion, coarse: torch.Tensor, scale: int, label: torch.Tensor):
    """criterion(upsample(coarse), label) as ``upsampled_cross_entropy`` gives it, for the criteria that function leaves to
    the expansion (``UpsampledLossFn``): an nn.CrossEntropyLoss with ``criterion_route(...) == "options"`` (class weights,
    label smoothing, 'sum' / 'none'), a ``FocalLoss2d`` with exponent 0 or >= 1 and a ``ProbOhemCrossEntropy2d`` (thresh in
    (0, 1]), each with the weight ``_class_weight`` takes.  None where this route does not apply: the plain criterion
    (it belongs to ``upsampled_cross_entropy``), any other criterion, exponent or weight, and every shape, pitch, alignment,
    class count, scale and label that function declines.  'none' returns (B, h scale, w scale)."""
    from .utils.loss_opr import FocalLoss2d, ProbOhemCrossEntropy2d
    if coarse.dim() != 4:
        return None
    nc = coarse.shape[3]
    if type(criterion) is FocalLoss2d:
        crit = criterion.loss
        gamma = float(criterion.exponent)
        if not (gamma == 0.0 or 1.0 <= gamma < float("inf")):
            return None
        kind, x, weight, reduction, ignore = "focal", gamma, crit.weight, crit.reduction, crit.ignore_index
    elif type(criterion) is ProbOhemCrossEntropy2d:
        if not 0.0 < criterion.thresh <= 1.0:
            return None
        kind, x, weight = "ohem", (criterion.thresh, criterion.min_kept), criterion.criterion.weight
        reduction, ignore = criterion.reduction, criterion.ignore_label
    elif criterion_route(criterion, coarse.device, nc) == "options":
        kind, x, weight = "options", float(criterion.label_smoothing), criterion.weight
        reduction, ignore = criterion.reduction, criterion.ignore_index
    else:
        return None
    if reduction not in CE_REDUCTIONS:
        return None
    args = _upsampled_rows(coarse, scale, label)
    if args is None:
        return None
    ok, w = _class_weight(weight, nc, coarse.device)
    if not ok:
        return None
    logits2, labels, ld, dims = args
    return UpsampledLossFn.apply(logits2, labels, w, int(ignore), ld, dims, kind, x, reduction)


CE_REDUCTIONS = ("mean", "sum", "none")


def _channels_last_rows(logits, label):
    """(nhwc, classes, ld) when `logits` (B, classes, H, W) is the view of fp32 channels-last rows on the GPU that the loss
    kernels take -- contiguous (B, H, W, classes) with classes % 4 == 0, or the first `classes` columns of a (B, H, W, ld)
    buffer with ld % 4 == 0 -- and `label` is a GPU tensor of its (B, H, W); else None"""
    if not (logits.is_cuda and logits.dtype == torch.float32 and label.is_cuda):
        return None
    nhwc = logits.permute(0, 2, 3, 1)
    nc = nhwc.shape[-1]
    if nhwc.data_ptr() % 16 != 0 or tuple(label.shape) != tuple(nhwc.shape[:3]):
        return None
    ld = nc if nhwc.is_contiguous() else _row_pitch(nhwc)
    if ld is None or ld % 4 != 0 or ld < nc:
        return None
    return nhwc, nc, ld


def _class_weight(weight, nc, device):
    """(True, w) with w None or the detached, contiguous weight the kernels read, or (False, None) for a weight they do
    not take: anything but a 1-D fp32 tensor of `nc` elements on `device`, 4-byte aligned"""
    if weight is None:
        return True, None
    if not (torch.is_tensor(weight) and weight.dtype == torch.float32 and weight.dim() == 1 and weight.numel() == nc
            and weight.device == device):
        return False, None
    w = weight.detach().contiguous()
    return (True, w) if w.data_ptr() % 4 == 0 else (False, None)


def _loss_rows(logits, label, weight):
    """What the three front-ends below hand to their Function: (logits2, labels, w, ld) -- the (rows, classes) view of
    ``_channels_last_rows`` at its pitch, the int64 labels of its rows, the weight of ``_class_weight`` -- or None when
    `logits` (B, classes, H, W), `label` (B, H, W) or `weight` is not what the loss kernels take"""
    if not (logits.dim() == 4 and label.dim() == 3):
        return None
    rows_view = _channels_last_rows(logits, label)
    if rows_view is None:
        return None
    nhwc, nc, ld = rows_view
    ok, w = _class_weight(weight, nc, logits.device)
    if not ok:
        return None
    return nhwc.reshape(-1, nc), label.long().contiguous().view(-1), w, ld      # reshape: a view at either pitch


def criterion_route(criterion, device, classes, any_float_weight=False):
    """Which Function takes `criterion` for logits of `classes` classes on `device`: "plain" (``SoftmaxCEFn``: mean, no
    weight, no smoothing), "options" (``SoftmaxCEOptFn``: anything else an nn.CrossEntropyLoss can be told, with the weight
    None or a 1-D fp32 tensor of `classes` elements on `device`), or None: a subclass or another criterion, a weight of
    another dtype (unless `any_float_weight`: the element-wise formulation casts it), size or device."""
    if type(criterion) is not nn.CrossEntropyLoss or criterion.reduction not in CE_REDUCTIONS:
        return None
    eps = float(getattr(criterion, "label_smoothing", 0.0))
    w = criterion.weight
    if criterion.reduction == "mean" and w is None and eps == 0.0:
        return "plain"
    if not 0.0 <= eps <= 1.0:
        return None
    if w is not None:
        dtype_ok = w.is_floating_point() if any_float_weight else w.dtype == torch.float32
        if not (dtype_ok and w.dim() == 1 and w.numel() == classes and w.device == torch.device(device)):
            return None
    return "options"


def cross_entropy(criterion, logits: torch.Tensor, label: torch.Tensor):
    """criterion(logits, label) for an nn.CrossEntropyLoss on channels-last logits -- logits is the (B, classes, H, W) VIEW
    of a contiguous (B, H, W, classes) tensor with classes % 4 == 0, or of the first `classes` columns of a (B, H, W, ld)
    buffer with ld % 4 == 0 (any class count: the padded classifier output of MambaDecoder.up_x4) -- or None when this
    path does not apply.  The plain criterion (mean, no weight, no smoothing) takes ``SoftmaxCEFn`` as it always has;
    ``weight`` (1-D fp32, on the logits' device), ``label_smoothing`` and ``reduction`` 'sum' / 'none' take
    ``SoftmaxCEOptFn`` ('none' returns (B, H, W)); see ``criterion_route`` for what is declined.  One combination keeps
    the answer it always had here, None: ``reduction='none'`` with neither a weight nor smoothing
    (tests/test_pointwise_gpu.py pins it).  The caller then runs the criterion itself or, under the deterministic flag,
    ``cross_entropy_deterministic``; the kernels take it (a NULL weight, eps = 0, a row loss), only this router does not.
    Labels outside [0, classes) that are not ``ignore_index`` are treated as ignored (csrc/pointwise.hip), where
    torch's kernel device-asserts: the reference's datasets map every unlabeled pixel to 255 = ignore_index
    (dataloader/RGBXDataset.py), so such labels do not occur on this path."""
    if logits.dim() != 4:
        return None
    route = criterion_route(criterion, logits.device, logits.shape[1])
    if route is None:
        return None
    if criterion.reduction == "none" and criterion.weight is None and float(getattr(criterion, "label_smoothing", 0.0)) == 0.0:
        return None                                        # declined before the option kernels existed, and still (see above)
    args = _loss_rows(logits, label, criterion.weight)
    if args is None:
        return None
    logits2, lab, w, ld = args
    if route == "plain":
        return SoftmaxCEFn.apply(logits2, lab, criterion.ignore_index, ld)
    return SoftmaxCEOptFn.apply(logits2, lab, w, criterion.ignore_index, ld, float(criterion.label_smoothing), criterion.reduction,
                                tuple(label.shape))


def ohem_cross_entropy(logits: torch.Tensor, label: torch.Tensor, ignore_index, thresh, min_kept, weight=None, reduction="mean"):
    """ProbOhemCrossEntropy2d(ignore_index, reduction, thresh, min_kept) with optional class weights on the channels-last
    logits ``cross_entropy`` takes (same layouts, same treatment of labels outside [0, classes)), or None when this path
    does not apply: another layout, dtype or device, a weight that is not a 1-D fp32 tensor of `classes` elements on the
    logits' device, a thresh outside (0, 1].  The hard pixels are selected on the device (sigma_ohem_select): no host
    synchronisation, so the step can be captured into a graph whichever branch the data take.  'none' returns (B, H, W)
    with zeros at dropped pixels; 'mean' divides by the summed weights of the KEPT pixels."""
    if reduction not in CE_REDUCTIONS or not 0.0 < float(thresh) <= 1.0:
        return None
    args = _loss_rows(logits, label, weight)
    if args is None:
        return None
    logits2, lab, w, ld = args
    return OhemCEFn.apply(logits2, lab, w, int(ignore_index), ld, float(thresh), int(min_kept), reduction, tuple(label.shape))


def focal_cross_entropy(logits: torch.Tensor, label: torch.Tensor, ignore_index, gamma, weight=None, reduction="mean"):
    """FocalLoss2d (utils/loss_opr.py:12-23) with the exponent `gamma` -- nn.NLLLoss(weight, reduction, ignore_index) of
    (1 - softmax)^gamma * log_softmax, i.e. w_y (1 - p_y)^gamma (lse - x_y) per pixel -- on the channels-last logits
    ``cross_entropy`` takes (same layouts, same treatment of labels outside [0, classes)), or None when this path does not
    apply: another layout, dtype or device, a weight the OHEM route would decline, or an exponent the kernels do not
    take: 0 < gamma < 1 (q^(gamma - 1) is unbounded as p_y -> 1; see include/sigma_ops.h), negative, NaN or infinite.
    'mean' divides by the summed weights of the labelled pixels on the device; 'none' returns (B, H, W)."""
    gamma = float(gamma)
    if reduction not in CE_REDUCTIONS or not (gamma == 0.0 or 1.0 <= gamma < float("inf")):
        return None
    args = _loss_rows(logits, label, weight)
    if args is None:
        return None
    logits2, lab, w, ld = args
    return SoftmaxFocalFn.apply(logits2, lab, w, int(ignore_index), ld, gamma, reduction, tuple(label.shape))


def _det_labels(logits, label, ignore_index, weight):
    """For the two element-wise losses below: (onehot, validf, wv, wy) -- the one-hot labels (B, classes, H, W), all zero
    at ignored pixels (labels outside [0, classes) count as ignored); 1 / 0 per pixel for labelled / ignored; the weight as
    (1, classes, 1, 1) or None; w_y per pixel, zero at ignored pixels"""
    nc = logits.shape[1]
    lab = label.long()
    valid = (lab != ignore_index) & (lab >= 0) & (lab < nc)
    onehot = F.one_hot(torch.where(valid, lab, torch.zeros_like(lab)), nc).permute(0, 3, 1, 2).to(logits.dtype)
    validf = valid.to(logits.dtype)
    wv = None if weight is None else weight.detach().to(logits.dtype).view(1, nc, 1, 1)
    wy = validf if wv is None else (onehot * wv).sum(dim=1) * validf
    return onehot, validf, wv, wy


def _det_reduce(per_pixel, wy, reduction):
    """'mean' divides the sum by the sum of w_y over the labelled pixels (0 / 0 = NaN when there is none)"""
    if reduction == "none":
        return per_pixel
    return per_pixel.sum() / wy.sum() if reduction == "mean" else per_pixel.sum()


def focal_deterministic(logits: torch.Tensor, label: torch.Tensor, ignore_index, gamma, weight=None, reduction="mean"):
    """The focal loss where ``focal_cross_entropy`` declines and torch's nll_loss2d may not run (the deterministic flag
    on GPU tensors): element-wise ops and fixed-order reductions only, as ``cross_entropy_deterministic`` below.  Per
    pixel -w_y (1 - p_y)^gamma log p_y, zero at ignored pixels (labels outside [0, classes) count as ignored); 'mean'
    divides the sum by the sum of w_y over the labelled pixels (0 / 0 = NaN when there is none).  Any gamma >= 0."""
    onehot, _, _, wy = _det_labels(logits, label, ignore_index, weight)
    lsm = F.log_softmax(logits, dim=1)
    focal = lsm if float(gamma) == 0.0 else (1.0 - F.softmax(logits, dim=1)) ** float(gamma) * lsm
    return _det_reduce(-(focal * onehot).sum(dim=1) * wy, wy, reduction)


def cross_entropy_deterministic(criterion, logits: torch.Tensor, label: torch.Tensor):
    """Deterministic mode only (sigma_amd/deterministic.py): criterion(logits, label) for an nn.CrossEntropyLoss -- class
    weights, label smoothing and any reduction included -- where ``cross_entropy`` above declines on LAYOUT: contiguous
    (B, classes, H, W) logits with classes % 4 != 0, i.e. SIGMA_GEMM=fp32 and the small test models; or None.  torch's
    nll_loss2d raises under the deterministic flag; this formulation uses only element-wise ops and fixed-order
    reductions: per pixel -(1 - eps) w_y log_softmax[y] - (eps / classes) sum_c w_c log_softmax[c], zero at ignored
    pixels (labels outside [0, classes) count as ignored, as on the kernels); 'mean' divides the sum by the sum of w_y
    over the labelled pixels (0 / 0 = NaN when there is none)."""
    if not (logits.dim() == 4 and label.dim() == 3):
        return None
    nc = logits.shape[1]
    route = criterion_route(criterion, logits.device, nc, any_float_weight=True)
    if route is None:
        return None
    onehot, validf, wv, wy = _det_labels(logits, label, criterion.ignore_index, criterion.weight)
    lsm = F.log_softmax(logits, dim=1)
    if route == "plain":
        return _det_reduce(-(lsm * onehot).sum(dim=1) * validf, validf, "mean")
    eps = float(criterion.label_smoothing)
    lsm_w = lsm if wv is None else lsm * wv
    per_pixel = -(lsm_w * onehot).sum(dim=1)
    if eps > 0.0:
        per_pixel = (1.0 - eps) * per_pixel - (eps / nc) * lsm_w.sum(dim=1)
    return _det_reduce(per_pixel * validf, wy, criterion.reduction)


REGION_KINDS = {"dice": (0.5, 0.5), "jaccard": (1.0, 1.0)}      # (a, b) of the Tversky index; "tversky" takes its own
REGION_MAX_CLASSES = 64      # include/sigma_region.h


class RegionLossFn(torch.autograd.Function):
    """The soft region-overlap loss of include/sigma_region.h on the rows of ``SoftmaxCEFn`` (csrc/region.hip):
    region_weight * (1 - mean over the labelled classes of the Tversky index (a, b) with smoothing s) + ce_weight * the mean
    cross entropy, the sums taken over the valid rows of this call.  Forward: sigma_region_loss_fwd -- the sums and the
    coefficient table on the device, nothing read back; backward: sigma_region_loss_bwd, one pass, the upstream gradient as a
    device scalar.  Returns (loss, terms, sums): the 0-dim loss, (region, cross entropy) and (3, classes) = I, P, Y; only the
    loss carries a gradient.  No labelled pixel at all: loss 0 and a zero gradient."""

    @staticmethod
    def _params(logits2, labels, lse, coef, ignore_index, ld, a, b, s, rw, cw):
        from ._capi_region import RegionParams
        p = RegionParams()
        p.rows, p.classes, p.ld, p.ignore_index = logits2.shape[0], logits2.shape[1], ld, int(ignore_index)
        p.alpha, p.beta, p.smooth, p.region_weight, p.ce_weight = float(a), float(b), float(s), float(rw), float(cw)
        p.logits, p.labels, p.lse, p.coef = logits2.data_ptr(), labels.data_ptr(), lse.data_ptr(), coef.data_ptr()
        return p

    @staticmethod
    def forward(ctx, logits2, labels, ignore_index, ld, a, b, s, rw, cw):
        from . import _capi_region
        lib = _capi_region.load()
        rows, nc = logits2.shape
        dev = logits2.device
        f32 = dict(device=dev, dtype=torch.float32)
        lse, coef = torch.empty(rows, **f32), torch.empty(2 * nc + 1, **f32)
        out = torch.empty(3 + 3 * nc, **f32)                  # loss, the two terms, the sums
        p = RegionLossFn._params(logits2, labels, lse, coef, ignore_index, ld, a, b, s, rw, cw)
        ws = _workspace(int(lib.sigma_region_loss_workspace_bytes(ctypes.byref(p))), dev, "region_loss_workspace_bytes")
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        p.loss, p.terms, p.sums = out.data_ptr(), out[1:].data_ptr(), out[3:].data_ptr()
        launch("sigma_region_loss_fwd", ctypes.byref(p), device=dev, what="region_loss_fwd")
        ctx.save_for_backward(logits2, labels, lse, coef)
        ctx.args = (int(ignore_index), ld, a, b, s, rw, cw)
        terms, sums = out[1:3], out[3:].view(3, nc)
        ctx.mark_non_differentiable(terms, sums)
        return out[0], terms, sums

    @staticmethod
    def backward(ctx, g, _gt, _gs):
        logits2, labels, lse, coef = ctx.saved_tensors
        rows, nc = logits2.shape
        ld = ctx.args[1]
        scale = g.float().reshape(1).contiguous()
        full = torch.empty((rows, ld), device=logits2.device, dtype=torch.float32)
        p = RegionLossFn._params(logits2, labels, lse, coef, ctx.args[0], ld, *ctx.args[2:])
        p.scale, p.dlogits = scale.data_ptr(), full.data_ptr()
        launch("sigma_region_loss_bwd", ctypes.byref(p), device=logits2.device, what="region_loss_bwd")
        return (_hand_off_padded(full, nc),) + (None,) * 8


def region_loss(logits: torch.Tensor, label: torch.Tensor, ignore_index=255, alpha=0.5, beta=0.5, smooth=0.0, region_weight=1.0,
                ce_weight=0.0, with_terms=False):
    """The region-overlap loss (``RegionLossFn``: Tversky index (alpha, beta); Dice = (0.5, 0.5), Jaccard = (1, 1)) on the
    channels-last logits ``cross_entropy`` takes (same layouts, same treatment of labels outside [0, classes)), or None
    when this path does not apply: another layout, dtype or device, more than 64 classes, beta <= 0, or a negative alpha,
    smooth or weight.  `with_terms`: (loss, terms, sums) instead of the loss."""
    a, b, s, rw, cw = float(alpha), float(beta), float(smooth), float(region_weight), float(ce_weight)
    if logits.dim() != 4 or not 1 <= logits.shape[1] <= REGION_MAX_CLASSES or not (b > 0.0 and a >= 0.0 and s >= 0.0 and rw >= 0.0 and cw >= 0.0):
        return None
    args = _loss_rows(logits, label, None)
    if args is None:
        return None
    logits2, lab, _, ld = args
    out = RegionLossFn.apply(logits2, lab, int(ignore_index), ld, a, b, s, rw, cw)
    return out if with_terms else out[0]


DISTILL_MAX_CLASSES = 64      # include/sigma_distill.h


class DistillLossFn(torch.autograd.Function):
    """The distillation loss of include/sigma_distill.h on the rows of ``SoftmaxCEFn`` (csrc/distill.hip), student rows
    logits2 at the pitch `ld` and teacher rows teacher2 at `ld_t`: kd_weight * T^2 * mean over the set S of
    KL(softmax(t / T) || softmax(x / T)) + ce_weight * the mean cross entropy; S = the valid rows, or every row with `kd_all`.
    Forward: sigma_distill_loss_fwd -- the sums and both scale factors on the device, nothing read back; backward:
    sigma_distill_loss_bwd, one pass, the upstream gradient as a device scalar.  Returns (loss, terms): the 0-dim loss and
    (kd, cross entropy), both unweighted; only the loss carries a gradient, and only to the student's logits.  An empty S:
    KD term 0; no valid row: CE term 0; both: a zero gradient."""

    @staticmethod
    def _params(logits2, teacher2, labels, lse, coef, ignore_index, ld, ld_t, T, kw, cw, kd_all):
        from ._capi_distill import DistillParams
        p = DistillParams()
        p.rows, p.classes, p.ld, p.ld_t = logits2.shape[0], logits2.shape[1], ld, ld_t
        p.kd_all, p.ignore_index = int(bool(kd_all)), int(ignore_index)
        p.temperature, p.kd_weight, p.ce_weight = float(T), float(kw), float(cw)
        p.logits, p.teacher, p.labels = logits2.data_ptr(), teacher2.data_ptr(), labels.data_ptr()
        p.lse, p.coef = lse.data_ptr(), coef.data_ptr()
        return p

    @staticmethod
    def forward(ctx, logits2, teacher2, labels, ignore_index, ld, ld_t, T, kw, cw, kd_all):
        from . import _capi_distill
        lib = _capi_distill.load()
        rows, nc = logits2.shape
        dev = logits2.device
        f32 = dict(device=dev, dtype=torch.float32)
        lse, coef = torch.empty(rows, 3, **f32), torch.empty(2, **f32)
        out = torch.empty(3, **f32)                           # loss, the two terms
        p = DistillLossFn._params(logits2, teacher2, labels, lse, coef, ignore_index, ld, ld_t, T, kw, cw, kd_all)
        ws = _workspace(int(lib.sigma_distill_loss_workspace_bytes(ctypes.byref(p))), dev, "distill_loss_workspace_bytes")
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        p.loss, p.terms = out.data_ptr(), out[1:].data_ptr()
        launch("sigma_distill_loss_fwd", ctypes.byref(p), device=dev, what="distill_loss_fwd")
        ctx.save_for_backward(logits2, teacher2, labels, lse, coef)
        ctx.args = (int(ignore_index), ld, ld_t, T, kw, cw, kd_all)
        terms = out[1:3]
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, g, _gt):
        logits2, teacher2, labels, lse, coef = ctx.saved_tensors
        rows, nc = logits2.shape
        ld = ctx.args[1]
        scale = g.float().reshape(1).contiguous()
        full = torch.empty((rows, ld), device=logits2.device, dtype=torch.float32)
        p = DistillLossFn._params(logits2, teacher2, labels, lse, coef, *ctx.args)
        p.scale, p.dlogits = scale.data_ptr(), full.data_ptr()
        launch("sigma_distill_loss_bwd", ctypes.byref(p), device=logits2.device, what="distill_loss_bwd")
        return (_hand_off_padded(full, nc),) + (None,) * 9


def distill_loss(logits: torch.Tensor, teacher_logits: torch.Tensor, label: torch.Tensor, ignore_index=255, temperature=1.0,
                 kd_weight=1.0, ce_weight=0.0, kd_all=False, with_terms=False):
    """The distillation loss (``DistillLossFn``) on the channels-last logits ``cross_entropy`` takes, student and teacher each
    at its own pitch (same layouts, same treatment of labels outside [0, classes)), or None when this path does not apply:
    either tensor of another layout, dtype or device, shapes that disagree, more than 64 classes, a temperature that is not
    positive or a negative weight.  The teacher's logits are read as they are and get no gradient.  `with_terms`: (loss,
    terms) instead of the loss."""
    T, kw, cw = float(temperature), float(kd_weight), float(ce_weight)
    if logits.dim() != 4 or tuple(teacher_logits.shape) != tuple(logits.shape) or not 1 <= logits.shape[1] <= DISTILL_MAX_CLASSES:
        return None
    if not (T > 0.0 and kw >= 0.0 and cw >= 0.0):
        return None
    args = _loss_rows(logits, label, None)
    if args is None or teacher_logits.device != logits.device:
        return None
    teacher = _channels_last_rows(teacher_logits.detach(), label)
    if teacher is None:
        return None
    logits2, lab, _, ld = args
    nhwc_t, nc, ld_t = teacher
    out = DistillLossFn.apply(logits2, nhwc_t.reshape(-1, nc), lab, int(ignore_index), ld, ld_t, T, kw, cw, bool(kd_all))
    return out if with_terms else out[0]
