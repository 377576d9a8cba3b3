"""ctypes binding of include/sigma_distill.h, the fifth header of libsigma_hip.so: the distillation loss of
csrc/distill.hip.  Kept apart from ``_capi.SIGNATURES`` / ``_capi.STRUCTS``, which list the three older headers exactly, as
``_capi_region`` is; the rows here are bound on top of ``_capi.load()``, so ``_launch.launch`` calls these entry points like
any other."""
from __future__ import annotations

import ctypes

from . import _capi

SIGMA_DISTILL_MAX_CLASSES = 64      # include/sigma_distill.h


class DistillParams(ctypes.Structure):
    """mirror of sigma_distill_params (include/sigma_distill.h)"""
    _fields_ = [
        ("rows", ctypes.c_int64), ("classes", ctypes.c_int32), ("ld", ctypes.c_int32), ("ld_t", ctypes.c_int32),
        ("kd_all", ctypes.c_int32), ("ignore_index", ctypes.c_int64),
        ("temperature", ctypes.c_double), ("kd_weight", ctypes.c_double), ("ce_weight", ctypes.c_double),
        ("logits", ctypes.c_void_p), ("teacher", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("loss", ctypes.c_void_p), ("terms", ctypes.c_void_p), ("coef", ctypes.c_void_p),
        ("scale", ctypes.c_void_p), ("dlogits", ctypes.c_void_p),
    ]


STRUCTS = {"sigma_distill_params": DistillParams}

# the prototypes of include/sigma_distill.h: name -> (restype, [argtypes]), as the rows of _capi.SIGNATURES
SIGNATURES = {
    **_capi._params_stream(DistillParams, "sigma_distill_loss_fwd", "sigma_distill_loss_bwd"),
    "sigma_distill_loss_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(DistillParams)]),
}
DISTILL_SYMBOLS = tuple(SIGNATURES)

_bound = None


def load() -> ctypes.CDLL:
    """``_capi.load()`` with the rows above bound as well; raises ``SigmaHipUnavailable`` for a library without them"""
    global _bound
    lib = _capi.load()
    if _bound is not lib:
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise _capi.SigmaHipUnavailable(f"{_capi.LIB_PATH} does not export {name}; rebuild") from e
            fn.restype, fn.argtypes = restype, argtypes
        _bound = lib
    return lib
