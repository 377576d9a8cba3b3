"""Explicit hand-off of a gradient buffer between two autograd nodes (no dynamic attributes on tensors)."""
from __future__ import annotations
# ---- hand-off of the in_proj gradient buffer between two autograd nodes -------------------------------------------------
# The gated LayerNorm's backward (layernorm.py) allocates ONE (..., 2C) buffer for the gradient of the in_proj output and
# writes dz into its z half; SplitXZFn.backward (ss2d_fused.py) completes the x half of the SAME buffer in place.  The
# buffer is handed over explicitly: registered here under the address of its z half, claimed (and removed) by the one
# consumer that presents a gradient living at that address with that geometry.  A gradient that took any other route
# (summed with a second consumer's, cloned by a hook) does not match and takes the copying path; stale entries are dropped
# after a few registrations.
_XZ_GRAD_BUFFERS = {}          # address of the z half -> weak reference to the full buffer
_XZ_GRAD_KEEP = 8


def offer_xz_grad_buffer(full, C: int) -> None:
    """`full`: contiguous (..., 2C) fp32 buffer whose z half [..., C:] is about to be written by the caller.

    Held WEAKLY: the gradient the caller returns is a view of `full` and keeps it alive (``view._base``) exactly as long
    as autograd holds that gradient; a buffer nobody claims (another consumer, a cloning hook) is released with its
    gradient instead of staying resident between steps or inside a graph-private pool (~100 MB each)."""
    import weakref
    for k in [k for k, r in _XZ_GRAD_BUFFERS.items() if r() is None]:
        _XZ_GRAD_BUFFERS.pop(k, None)
    while len(_XZ_GRAD_BUFFERS) >= _XZ_GRAD_KEEP:
        _XZ_GRAD_BUFFERS.pop(next(iter(_XZ_GRAD_BUFFERS)))
    _XZ_GRAD_BUFFERS[full.data_ptr() + 4 * C] = weakref.ref(full)


def claim_xz_grad_buffer(dz, shape2):
    """the registered buffer of shape `shape2` = (..., 2C) whose z half IS `dz` (same address, strides, dtype, device), or None"""
    if dz is None:
        return None
    ref = _XZ_GRAD_BUFFERS.pop(dz.data_ptr(), None)
    full = ref() if ref is not None else None
    if full is None:
        return None
    C = shape2[-1] // 2
    ok = (tuple(full.shape) == tuple(shape2) and full.is_contiguous() and full.dtype == dz.dtype and full.device == dz.device
          and tuple(dz.shape) == (*shape2[:-1], C) and dz.stride() == full[..., C:].stride())
    return full if ok else None


# ---- hand-off of the padded logits gradient between the loss and the classifier ---------------------------------------------
# A classifier of nc classes with nc % 4 != 0 writes its logits into (rows, ld) buffers, ld = 4 ceil(nc / 4)
# (gemm.ClassifierPadFn); the loss backward (pointwise.SoftmaxCEFn) writes the gradient into a buffer of the same pitch with
# exact zeros in the pad columns and returns its [:, :nc] view.  The classifier's backward may hand the WHOLE buffer to its
# GEMMs only when it knows the pad is zero: the buffer is registered here under its address and claimed by the consumer
# that presents a gradient at that address with that geometry.  Same rules as above: held weakly, anything else copies.
_PAD_GRAD_BUFFERS = {}         # address of the buffer -> weak reference to it
_PAD_GRAD_KEEP = 8


def offer_padded_grad_buffer(full) -> None:
    """`full`: contiguous (rows, ld) fp32 buffer whose columns [nc, ld) the caller has just written with zeros"""
    import weakref
    for k in [k for k, r in _PAD_GRAD_BUFFERS.items() if r() is None]:
        _PAD_GRAD_BUFFERS.pop(k, None)
    while len(_PAD_GRAD_BUFFERS) >= _PAD_GRAD_KEEP:
        _PAD_GRAD_BUFFERS.pop(next(iter(_PAD_GRAD_BUFFERS)))
    _PAD_GRAD_BUFFERS[full.data_ptr()] = weakref.ref(full)


def claim_padded_grad_buffer(dy, ld: int):
    """the registered (rows, ld) buffer whose first nc columns ARE the 2-D gradient `dy` (same address, pitch, dtype,
    device), or None"""
    if dy is None:
        return None
    ref = _PAD_GRAD_BUFFERS.pop(dy.data_ptr(), None)
    full = ref() if ref is not None else None
    if full is None:
        return None
    ok = (dy.dim() == 2 and tuple(full.shape) == (dy.shape[0], ld) and full.is_contiguous() and full.dtype == dy.dtype
          and full.device == dy.device and dy.shape[1] <= ld and dy.stride() == (ld, 1))
    return full if ok else None
