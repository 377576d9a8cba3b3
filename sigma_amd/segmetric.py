"""The evaluator's per-image bookkeeping on the HIP kernels of csrc/segmetric.hip (C ABI: include/sigma_ops.h).

``accumulate_scores``   acc (+)= score for one scale: (C, H, W) float32 into (C, H, W) float64, the first scale writes
                        (engine/evaluator.py:437-448 adds into np.zeros of float64 in scale order; same IEEE adds)
``argmax_confusion``    ONE pass: numpy's argmax over the classes, and utils/metric.py:8-15 hist_info of that prediction
                        against the labels -> pred on the device, (hist, labeled, correct) on the host
``confusion``           hist_info of a given prediction

Device tensors only (host inputs are copied to the device by the callers); there is no host fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi
from ._launch import call, launch


def _labels(t: torch.Tensor, what: str) -> torch.Tensor:
    """uint8 and int64 are read as they are; other integer types are widened to int64 (exact)"""
    if t.dtype in (torch.uint8, torch.int64):
        return t.contiguous()
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{what} must hold integers, got {t.dtype}")
    return t.to(torch.int64).contiguous()


def accumulate_scores(acc: torch.Tensor, score: torch.Tensor, first: bool) -> None:
    """acc = 0.0 + score (first) or acc += score, elementwise in float64; acc (C, H, W) float64, score (C, H, W) float32,
    both on the same GPU (score made contiguous if it is not)."""
    if acc.dtype != torch.float64 or score.dtype != torch.float32 or not acc.is_cuda or acc.device != score.device:
        raise TypeError(f"accumulate_scores: float64 acc and float32 score on one GPU, got {acc.dtype} {acc.device} / "
                        f"{score.dtype} {score.device}")
    if acc.dim() != 3 or tuple(acc.shape) != tuple(score.shape) or not acc.is_contiguous():
        raise ValueError(f"accumulate_scores: contiguous (C, H, W) acc of the score's shape, got {tuple(acc.shape)} / {tuple(score.shape)}")
    score = score.contiguous()
    p = _capi.SegAccumulateParams()
    p.pixels = acc.shape[1] * acc.shape[2]
    p.classes, p.first = acc.shape[0], int(bool(first))
    p.score, p.acc = score.data_ptr(), acc.data_ptr()
    p.score_plane_stride = p.acc_plane_stride = p.pixels
    launch("sigma_seg_accumulate", ctypes.byref(p), device=acc.device)


def _launch(p, dev) -> None:
    rc = call("sigma_seg_argmax_confusion", ctypes.byref(p), device=dev)
    if rc != 0:
        raise RuntimeError(f"sigma_seg_argmax_confusion: status {rc}")


def _counts(p, gt: torch.Tensor, n_cl: int, dev):
    """points p at a zero-filled int64 buffer [hist (n_cl * n_cl) | labeled | correct | invalid] and the labels"""
    if not 1 <= n_cl <= 256:
        raise ValueError(f"n_cl must be in 1..256, got {n_cl}")
    buf = torch.zeros(n_cl * n_cl + 3, dtype=torch.int64, device=dev)
    p.n_cl = n_cl
    p.gt, p.gt_elem_size = gt.data_ptr(), gt.element_size()
    p.hist, p.counts = buf.data_ptr(), buf[n_cl * n_cl:].data_ptr()
    return buf


def _host_result(buf: torch.Tensor, n_cl: int):
    host = buf.cpu().numpy()
    labeled, correct, invalid = (int(v) for v in host[n_cl * n_cl:])
    if invalid:
        raise ValueError(f"{invalid} labeled pixels have a prediction outside [0, {n_cl})")
    return host[:n_cl * n_cl].reshape(n_cl, n_cl).copy(), labeled, correct


def argmax(acc: torch.Tensor, pred_dtype: torch.dtype = torch.int64) -> torch.Tensor:
    """numpy's acc.argmax(0) of a contiguous (C, H, W) float64 device tensor (first maximum, first NaN) -> (H, W)"""
    pred, _ = _argmax_confusion(acc, None, 0, pred_dtype, True)
    return pred


def argmax_confusion(acc: torch.Tensor, gt, n_cl: int, pred_dtype: torch.dtype = torch.int64, want_pred: bool = True):
    """(pred or None, (hist, labeled, correct)): pred = acc.argmax(0) on the device, and hist_info(n_cl, pred, gt)
    computed in the same pass.  gt: (H, W) labels, a tensor or numpy array (copied to acc's device)."""
    return _argmax_confusion(acc, gt, n_cl, pred_dtype, want_pred)


def _argmax_confusion(acc, gt, n_cl, pred_dtype, want_pred):
    if acc.dtype != torch.float64 or not acc.is_cuda or acc.dim() != 3 or not acc.is_contiguous():
        raise TypeError(f"argmax_confusion: contiguous (C, H, W) float64 device scores, got {acc.dtype} {tuple(acc.shape)} {acc.device}")
    if pred_dtype not in (torch.int64, torch.uint8):
        raise TypeError(f"pred_dtype must be torch.int64 or torch.uint8, got {pred_dtype}")
    dev = acc.device
    C, H, W = acc.shape
    p = _capi.SegConfusionParams()
    p.pixels, p.classes = H * W, C
    p.acc, p.acc_plane_stride = acc.data_ptr(), H * W
    p.pred_elem_size = 1 if pred_dtype == torch.uint8 else 8
    pred = torch.empty((H, W), dtype=pred_dtype, device=dev) if want_pred else None
    p.pred = pred.data_ptr() if want_pred else None
    if gt is None:
        p.n_cl, p.gt_elem_size = 1, 1               # arg-max only: no labels, no counts (the checks still see valid sizes)
        _launch(p, dev)
        return pred, None
    gt = _labels(torch.as_tensor(gt).to(dev), "gt")
    if tuple(gt.shape) != (H, W):
        raise ValueError(f"gt of shape {tuple(gt.shape)} for scores of {H} x {W} pixels")
    buf = _counts(p, gt, n_cl, dev)
    _launch(p, dev)
    return pred, _host_result(buf, n_cl)


def confusion(pred, gt, n_cl: int, device=None):
    """utils/metric.py:8-15 hist_info(n_cl, pred, gt) on the device: (hist int64 (n_cl, n_cl), labeled, correct).
    pred / gt: tensors or numpy arrays of one shape; host data goes to `device` (default: the device of a GPU
    argument, else the current one)."""
    if device is None:
        on = [t.device for t in (pred, gt) if isinstance(t, torch.Tensor) and t.is_cuda]
        device = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    pred = _labels(torch.as_tensor(pred).to(dev), "pred")
    gt = _labels(torch.as_tensor(gt).to(dev), "gt")
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    p = _capi.SegConfusionParams()
    p.pixels, p.classes = pred.numel(), 0
    p.acc, p.acc_plane_stride = None, 0
    p.pred, p.pred_elem_size = pred.data_ptr(), pred.element_size()
    buf = _counts(p, gt, n_cl, dev)
    if p.pixels:
        _launch(p, dev)
    return _host_result(buf, n_cl)
