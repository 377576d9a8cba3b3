"""The torch side of a call into libsigma_hip.so: the one place where tensors, devices and streams meet the C ABI that
``_capi`` mirrors.  An operator module fills a parameter struct (or lists plain arguments) and names the entry point:

    launch("sigma_transpose2d", ctypes.byref(p), device=src.device, what="transpose2d")

Arguments are converted by the entry point's row in ``_capi.SIGNATURES``: ``ctypes.byref(p)`` for a ``const struct *``
parameter, ``ptr(t)`` for a device pointer, ``None`` for NULL.  The stream is never written out by a caller.
"""
from __future__ import annotations

import ctypes

import torch

from . import _capi


def ptr(t):
    """the device pointer of `t` (storage offset included) for a ``void *`` / ``float *`` parameter; None (NULL) for None"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(name, *args, device):
    """``name(*args, stream)`` with `device` current and its current stream as the last argument; returns the status"""
    fn = getattr(_capi.load(), name)
    with torch.cuda.device(device):
        return fn(*args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))


def launch(name, *args, device, what=None):
    """``call`` that raises ``RuntimeError("{what}: {last error} (sigma_status {rc})")`` on a non-zero status"""
    _capi.check(call(name, *args, device=device), what or name)


def workspace(nbytes, device, what):
    """The scratch buffer a ``*_workspace_bytes`` query asked for: a uint8 tensor of `nbytes` on `device`, None for zero.
    A negative answer is the query refusing the parameters: RuntimeError with the library's reason.  The caller stores
    pointer and size in its params and keeps the tensor referenced until its launch is enqueued."""
    if nbytes < 0:
        raise RuntimeError(f"{what}: {_capi.last_error()}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes > 0 else None


def first_use(done, device, in_capture_message, run):
    """Once per process and device (`done`: the caller's set of device indices): ``run()``, a self test that allocates
    and synchronises -- so never inside a stream capture, where `in_capture_message` is raised instead.  ``run`` raises
    its own error on failure, and the device is then not marked."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key in done:
        return
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(in_capture_message)
    run()
    done.add(key)
