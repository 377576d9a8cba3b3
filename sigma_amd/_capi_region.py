"""ctypes binding of include/sigma_region.h, the fourth header of libsigma_hip.so: the region-overlap losses of
csrc/region.hip.  Kept apart from ``_capi.SIGNATURES`` / ``_capi.STRUCTS``, which list the three older headers exactly;
the rows here are bound on top of ``_capi.load()``, so ``_launch.launch`` calls these entry points like any other."""
from __future__ import annotations

import ctypes

from . import _capi

SIGMA_REGION_MAX_CLASSES = 64      # include/sigma_region.h


class RegionParams(ctypes.Structure):
    """mirror of sigma_region_params (include/sigma_region.h)"""
    _fields_ = [
        ("rows", ctypes.c_int64), ("classes", ctypes.c_int32), ("ld", ctypes.c_int32), ("ignore_index", ctypes.c_int64),
        ("alpha", ctypes.c_double), ("beta", ctypes.c_double), ("smooth", ctypes.c_double),
        ("region_weight", ctypes.c_double), ("ce_weight", ctypes.c_double),
        ("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("loss", ctypes.c_void_p), ("terms", ctypes.c_void_p), ("coef", ctypes.c_void_p), ("sums", ctypes.c_void_p),
        ("scale", ctypes.c_void_p), ("dlogits", ctypes.c_void_p),
    ]


STRUCTS = {"sigma_region_params": RegionParams}

# the prototypes of include/sigma_region.h: name -> (restype, [argtypes]), as the rows of _capi.SIGNATURES
SIGNATURES = {
    **_capi._params_stream(RegionParams, "sigma_region_loss_fwd", "sigma_region_loss_bwd"),
    "sigma_region_loss_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(RegionParams)]),
}
REGION_SYMBOLS = tuple(SIGNATURES)

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
