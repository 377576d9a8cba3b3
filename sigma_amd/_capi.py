"""ctypes binding of libsigma_hip.so (C ABI declared in include/sigma_scan.h).

The library is REQUIRED: importing the operator modules without it raises
``SigmaHipUnavailable`` -- there is no CPU or eager fallback anywhere in the product
path (the CPU oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# SIGMA_HIP_LIB lets a benchmark A/B an experimental build of the same ABI; default is the in-tree library
LIB_PATH = os.environ.get("SIGMA_HIP_LIB") or os.path.join(_HERE, "lib", "libsigma_hip.so")

SIGMA_SCAN_ABI_VERSION = 13
SIGMA_SCAN_CHUNK = 2048
SIGMA_SCAN_CKPT_PITCH = 1280
SIGMA_SCAN_CKPT_PITCH_FINE = 640
SIGMA_SCAN_CKPT_PITCH_320 = 320
SIGMA_SCAN_CKPT_PITCH_160 = 160
SIGMA_SCAN_CKPT_PITCH_16 = 16
SIGMA_SCAN_MAX_DSTATE = 256
SIGMA_SCAN_BWD_DETERMINISTIC = 1    # sigma_scan_bwd_params.flags
SIGMA_DWCONV_DETERMINISTIC = 1      # sigma_dwconv_params.flags (include/sigma_ops.h)

DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2


class SigmaHipUnavailable(RuntimeError):
    pass


class FwdParams(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32), ("dim", ctypes.c_int32), ("seqlen", ctypes.c_int32),
        ("dstate", ctypes.c_int32), ("n_groups", ctypes.c_int32), ("n_chunks", ctypes.c_int32),
        ("io_dtype", ctypes.c_int32), ("delta_softplus", ctypes.c_int32),
        ("rev_group_mask", ctypes.c_uint32), ("u_group_shift", ctypes.c_int32),
        ("ckpt_pitch", ctypes.c_int32), ("param_group_swap", ctypes.c_int32), ("x_row_stride", ctypes.c_int64),
        ("u", ctypes.c_void_p), ("delta", ctypes.c_void_p), ("A", ctypes.c_void_p),
        ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("D", ctypes.c_void_p),
        ("delta_bias", ctypes.c_void_p),
        ("out", ctypes.c_void_p), ("x", ctypes.c_void_p),
        ("u_batch_stride", ctypes.c_int64), ("u_d_stride", ctypes.c_int64),
        ("delta_batch_stride", ctypes.c_int64), ("delta_d_stride", ctypes.c_int64),
        ("A_d_stride", ctypes.c_int64), ("A_dstate_stride", ctypes.c_int64),
        ("B_batch_stride", ctypes.c_int64), ("B_group_stride", ctypes.c_int64), ("B_dstate_stride", ctypes.c_int64),
        ("C_batch_stride", ctypes.c_int64), ("C_group_stride", ctypes.c_int64), ("C_dstate_stride", ctypes.c_int64),
        ("out_batch_stride", ctypes.c_int64), ("out_d_stride", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]


class BwdParams(ctypes.Structure):
    _fields_ = [
        ("fwd", FwdParams),
        ("dout", ctypes.c_void_p), ("du", ctypes.c_void_p), ("ddelta", ctypes.c_void_p),
        ("dA", ctypes.c_void_p), ("dB", ctypes.c_void_p), ("dC", ctypes.c_void_p),
        ("dD", ctypes.c_void_p), ("ddelta_bias", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("dout_group_shift", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("dout_batch_stride", ctypes.c_int64), ("dout_d_stride", ctypes.c_int64),
        ("du_batch_stride", ctypes.c_int64), ("du_d_stride", ctypes.c_int64),
        ("ddelta_batch_stride", ctypes.c_int64), ("ddelta_d_stride", ctypes.c_int64),
        ("dA_d_stride", ctypes.c_int64), ("dA_dstate_stride", ctypes.c_int64),
        ("dB_batch_stride", ctypes.c_int64), ("dB_group_stride", ctypes.c_int64), ("dB_dstate_stride", ctypes.c_int64),
        ("dC_batch_stride", ctypes.c_int64), ("dC_group_stride", ctypes.c_int64), ("dC_dstate_stride", ctypes.c_int64),
    ]


class DwConvParams(ctypes.Structure):
    """mirror of sigma_dwconv_params (include/sigma_ops.h)"""
    _fields_ = [
        ("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
        ("n_orders", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p),
        ("out2", ctypes.c_void_p),
        ("g2", ctypes.c_void_p), ("gpre", ctypes.c_void_p), ("dweight", ctypes.c_void_p), ("dbias", ctypes.c_void_p),
        ("dx", ctypes.c_void_p),
        ("x_batch_stride", ctypes.c_int64), ("x_channel_stride", ctypes.c_int64),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]


class MergeParams(ctypes.Structure):
    """mirror of sigma_merge_params (include/sigma_ops.h)"""
    _fields_ = [
        ("batch", ctypes.c_int32), ("channels", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
        ("planes4", ctypes.c_void_p), ("planes2", ctypes.c_void_p), ("nhwc", ctypes.c_void_p),
    ]


class TransposeParams(ctypes.Structure):
    """mirror of sigma_transpose_params (include/sigma_ops.h)"""
    _fields_ = [
        ("batch", ctypes.c_int32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("reserved_", ctypes.c_int32),
        ("src", ctypes.c_void_p), ("dst", ctypes.c_void_p),
        ("src_batch_stride", ctypes.c_int64), ("src_row_stride", ctypes.c_int64),
        ("dst_batch_stride", ctypes.c_int64), ("dst_row_stride", ctypes.c_int64),
    ]


class LayerNormParams(ctypes.Structure):
    """mirror of sigma_layernorm_params (include/sigma_ops.h)"""
    _fields_ = [
        ("rows", ctypes.c_int64), ("channels", ctypes.c_int32), ("eps", ctypes.c_float),
        ("x", ctypes.c_void_p), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
        ("y", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("rstd", ctypes.c_void_p),
        ("dy", ctypes.c_void_p), ("dx", ctypes.c_void_p), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p),
        ("gate", ctypes.c_void_p), ("gate_row_stride", ctypes.c_int64), ("dgate", ctypes.c_void_p),
        ("dgate_row_stride", ctypes.c_int64),
        ("row_scale", ctypes.c_void_p), ("rows_per_scale", ctypes.c_int64),
        ("dx_add", ctypes.c_void_p),
    ]


class GemmParams(ctypes.Structure):
    """mirror of sigma_gemm_params (include/sigma_gemm.h)"""
    _fields_ = [
        ("M", ctypes.c_int64), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("A", ctypes.c_void_p), ("Bt", ctypes.c_void_p), ("C", ctypes.c_void_p), ("bias", ctypes.c_void_p),
        ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
        ("accumulate", ctypes.c_int32), ("batch", ctypes.c_int32),
        ("strideA", ctypes.c_int64), ("strideB", ctypes.c_int64), ("strideC", ctypes.c_int64),
        ("a_mod", ctypes.c_int32), ("pieces", ctypes.c_int32),
        ("c_mod", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("residual", ctypes.c_void_p), ("residual2", ctypes.c_void_p), ("ldr", ctypes.c_int64), ("strideR", ctypes.c_int64),
        ("Ct", ctypes.c_void_p), ("ldct", ctypes.c_int64), ("t_cols", ctypes.c_int32), ("k_slices", ctypes.c_int32),
        ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
    ]


class GateBwdParams(ctypes.Structure):
    """mirror of sigma_gate_bwd_params (include/sigma_ops.h)"""
    _fields_ = [
        ("planes", ctypes.c_int64), ("hw", ctypes.c_int64),
        ("g", ctypes.c_void_p), ("x", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("dmean", ctypes.c_void_p),
        ("dmax", ctypes.c_void_p), ("max", ctypes.c_void_p), ("count", ctypes.c_void_p), ("dx", ctypes.c_void_p),
    ]


class SegAccumulateParams(ctypes.Structure):
    """mirror of sigma_seg_accumulate_params (include/sigma_ops.h)"""
    _fields_ = [
        ("pixels", ctypes.c_int64), ("classes", ctypes.c_int32), ("first", ctypes.c_int32),
        ("score", ctypes.c_void_p), ("acc", ctypes.c_void_p),
        ("score_plane_stride", ctypes.c_int64), ("acc_plane_stride", ctypes.c_int64),
    ]


class SegConfusionParams(ctypes.Structure):
    """mirror of sigma_seg_confusion_params (include/sigma_ops.h)"""
    _fields_ = [
        ("pixels", ctypes.c_int64), ("classes", ctypes.c_int32), ("n_cl", ctypes.c_int32),
        ("gt_elem_size", ctypes.c_int32), ("pred_elem_size", ctypes.c_int32),
        ("acc", ctypes.c_void_p), ("acc_plane_stride", ctypes.c_int64),
        ("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("hist", ctypes.c_void_p), ("counts", ctypes.c_void_p),
    ]


class CeOptParams(ctypes.Structure):
    """mirror of sigma_ce_opt_params (include/sigma_ops.h)"""
    _fields_ = [
        ("rows", ctypes.c_int64), ("classes", ctypes.c_int32), ("ld", ctypes.c_int32), ("ignore_index", ctypes.c_int64),
        ("label_smoothing", ctypes.c_float), ("reserved_", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("weight", ctypes.c_void_p),
        ("lse", ctypes.c_void_p), ("row_loss", ctypes.c_void_p), ("partial", ctypes.c_void_p),
        ("scale", ctypes.c_void_p), ("row_grad", ctypes.c_void_p), ("dlogits", ctypes.c_void_p),
    ]


class OhemParams(ctypes.Structure):
    """mirror of sigma_ohem_params (include/sigma_ops.h)"""
    _fields_ = [
        ("rows", ctypes.c_int64), ("ignore_index", ctypes.c_int64), ("classes", ctypes.c_int32), ("thresh", ctypes.c_float),
        ("min_kept", ctypes.c_int64),
        ("nll", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("mined", ctypes.c_void_p), ("tau", ctypes.c_void_p),
        ("counts", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_int64),
        ("weight", ctypes.c_void_p), ("row_loss", ctypes.c_void_p), ("partial", ctypes.c_void_p),
    ]


class UpsampleCeParams(ctypes.Structure):
    """mirror of sigma_upsample_ce_params (include/sigma_ops.h)"""
    _fields_ = [
        ("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("scale", ctypes.c_int32),
        ("classes", ctypes.c_int32), ("ld", ctypes.c_int32), ("ignore_index", ctypes.c_int64),
        ("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("lse", ctypes.c_void_p), ("partial", ctypes.c_void_p),
        ("scale_grad", ctypes.c_void_p), ("dlogits", ctypes.c_void_p),
    ]


class UpsampleLossParams(ctypes.Structure):
    """mirror of sigma_upsample_loss_params (include/sigma_ops.h)"""
    _fields_ = [
        ("batch", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("scale", ctypes.c_int32),
        ("classes", ctypes.c_int32), ("ld", ctypes.c_int32), ("ignore_index", ctypes.c_int64),
        ("kind", ctypes.c_int32), ("label_smoothing", ctypes.c_float), ("gamma", ctypes.c_float), ("reserved_", ctypes.c_int32),
        ("logits", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("lse", ctypes.c_void_p),
        ("row_loss", ctypes.c_void_p), ("coef", ctypes.c_void_p), ("partial", ctypes.c_void_p),
        ("scale_grad", ctypes.c_void_p), ("row_grad", ctypes.c_void_p), ("dlogits", ctypes.c_void_p),
    ]


SIGMA_CE_BLOCKS = 1024      # include/sigma_ops.h
SIGMA_UPSAMPLE_LOSS_OPTIONS, SIGMA_UPSAMPLE_LOSS_FOCAL = 0, 1      # include/sigma_ops.h: sigma_upsample_loss_params.kind
SIGMA_OHEM_HIST_BLOCKS = 512        # include/sigma_ops.h
SIGMA_SEG_LDS_HIST_BYTES = 32768    # include/sigma_ops.h

GEMM_FORMS = {"nt": 0, "nn": 1, "tn": 2}
GEMM_EPILOGUES = ("rows", "direct", "transposed")      # sigma_gemm_plan out[7] bits 0-1
GEMM_RES_LOADS = ("none", "vector", "scalar")          # bits 2-3
GEMM_STORES = ("store", "accumulate", "atomic")        # bits 6-7

# C struct name -> ctypes mirror, every struct of the three headers (tests compare each layout with the compiler's)
STRUCTS = {
    "sigma_scan_fwd_params": FwdParams, "sigma_scan_bwd_params": BwdParams,
    "sigma_dwconv_params": DwConvParams, "sigma_merge_params": MergeParams, "sigma_transpose_params": TransposeParams,
    "sigma_layernorm_params": LayerNormParams, "sigma_gate_bwd_params": GateBwdParams,
    "sigma_seg_accumulate_params": SegAccumulateParams, "sigma_seg_confusion_params": SegConfusionParams,
    "sigma_ce_opt_params": CeOptParams, "sigma_ohem_params": OhemParams, "sigma_upsample_ce_params": UpsampleCeParams,
    "sigma_upsample_loss_params": UpsampleLossParams,
    "sigma_gemm_params": GemmParams,
}

# The prototypes of the three headers, one row per entry point: name -> (restype, [argtypes]).  ``load`` binds exactly
# these rows -- an entry point without a row cannot be called through the binding -- and tests/test_capi_cpu.py holds
# every row against its prototype.  A new entry point is declared HERE, once; the public tuples below follow.
_I32, _I64, _INT, _F32, _VP, _STR = (ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                     ctypes.c_char_p)
_P = ctypes.POINTER


def _params_stream(struct, *names):
    """rows of the commonest prototype, int f(const struct *params, void *stream)"""
    return {n: (_INT, [_P(struct), _VP]) for n in names}


# include/sigma_scan.h
_SCAN_SIGNATURES = {
    **_params_stream(FwdParams, "sigma_selective_scan_fwd"),
    **_params_stream(BwdParams, "sigma_selective_scan_bwd"),
    "sigma_scan_bwd_workspace_bytes": (_I64, [_P(BwdParams)]),
    "sigma_scan_fwd_workspace_bytes": (_I64, [_P(FwdParams)]),
    "sigma_scan_last_error": (_STR, []),
    "sigma_scan_abi_version": (_INT, []),
    "sigma_scan_set_option": (_INT, [_STR, _INT]),
    "sigma_scan_get_option": (_INT, [_STR]),
    "sigma_scan_fwd_plan": (_INT, [_P(FwdParams), _P(_I32 * 6)]),
    "sigma_scan_bwd_plan": (_INT, [_P(BwdParams), _P(_I32 * 6)]),
    "sigma_scan_selftest": (_INT, [_VP]),
    "sigma_scan_rowlane_selftest": (_INT, [_VP]),
}
# include/sigma_ops.h: the launches and the host-side row count of the LayerNorm backward (int results) ...
_OPS_SIGNATURES = {
    **_params_stream(DwConvParams, "sigma_dwconv3x3_silu_fwd", "sigma_dwconv3x3_silu_bwd"),
    **_params_stream(MergeParams, "sigma_cross_merge_nhwc", "sigma_cross_split_nhwc"),
    **_params_stream(LayerNormParams, "sigma_layernorm_fwd", "sigma_layernorm_bwd"),
    "sigma_layernorm_bwd_partial_rows": (_INT, [_I64, _I32]),
    **_params_stream(TransposeParams, "sigma_transpose2d"),
    "sigma_pair_sum_add": (_INT, [_VP, _VP, _I64, _I64, _VP]),
    "sigma_upsample2x_nhwc": (_INT, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "sigma_plane_pool": (_INT, [_VP, _I64, _I64, _VP, _VP, _VP, _VP]),
    "sigma_plane_scale": (_INT, [_VP, _VP, _VP, _I64, _I64, _VP]),
    "sigma_plane_dot": (_INT, [_VP, _VP, _VP, _I64, _I64, _VP]),
    **_params_stream(GateBwdParams, "sigma_plane_gate_bwd"),
    "sigma_softmax_ce_fwd": (_INT, [_VP, _VP, _I64, _I32, _I64, _VP, _VP, _VP]),
    "sigma_softmax_ce_bwd": (_INT, [_VP, _VP, _VP, _VP, _I64, _I32, _I64, _VP, _VP]),
    "sigma_softmax_ce_fwd_ld": (_INT, [_VP, _VP, _I64, _I32, _I32, _I64, _VP, _VP, _VP]),
    "sigma_softmax_ce_bwd_ld": (_INT, [_VP, _VP, _VP, _VP, _I64, _I32, _I32, _I64, _VP, _VP]),
    **_params_stream(CeOptParams, "sigma_softmax_ce_opt_fwd", "sigma_softmax_ce_opt_bwd"),
    "sigma_colscale_bwd": (_INT, [_VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP]),
    "sigma_colscale_bwd_ws": (_INT, [_VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _I64, _VP]),
    **_params_stream(SegAccumulateParams, "sigma_seg_accumulate"),
    **_params_stream(SegConfusionParams, "sigma_seg_argmax_confusion"),
    **_params_stream(OhemParams, "sigma_ohem_select"),
    "sigma_softmax_focal_fwd": (_INT, [_P(CeOptParams), _F32, _VP]),
    "sigma_softmax_focal_bwd": (_INT, [_P(CeOptParams), _F32, _VP]),
    **_params_stream(UpsampleCeParams, "sigma_upsample_ce_fwd", "sigma_upsample_ce_bwd"),
    **_params_stream(UpsampleLossParams, "sigma_upsample_loss_fwd", "sigma_upsample_loss_bwd"),
}
# ... and its size queries (int64_t results)
_OPS_AUX_SIGNATURES = {
    "sigma_dwconv3x3_silu_bwd_workspace_bytes": (_I64, [_P(DwConvParams)]),
    "sigma_colscale_bwd_workspace_bytes": (_I64, [_I64, _I32]),
    "sigma_ohem_workspace_bytes": (_I64, [_I64]),
}
# include/sigma_gemm.h: the three launches, then the host-side entry points and the self test
_GEMM_SIGNATURES = _params_stream(GemmParams, "sigma_gemm_nt_split3", "sigma_gemm_nn_split3", "sigma_gemm_tn_split3")
_GEMM_AUX_SIGNATURES = {
    "sigma_gemm_selftest": (_INT, [_VP]),
    "sigma_gemm_workspace_bytes": (_I64, [_P(GemmParams), _INT]),
    "sigma_gemm_plan": (_INT, [_P(GemmParams), _INT, _P(_I32 * 8)]),
}

# every symbol each header declares, in the table's order; tests check the library exports all of them
EXPORTED_SYMBOLS = tuple(_SCAN_SIGNATURES)
OPS_SYMBOLS = tuple(_OPS_SIGNATURES)
OPS_AUX_SYMBOLS = tuple(_OPS_AUX_SIGNATURES)
GEMM_SYMBOLS = tuple(_GEMM_SIGNATURES)
GEMM_AUX_SYMBOLS = tuple(_GEMM_AUX_SIGNATURES)
SIGNATURES = {**_SCAN_SIGNATURES, **_OPS_SIGNATURES, **_OPS_AUX_SIGNATURES, **_GEMM_SIGNATURES, **_GEMM_AUX_SIGNATURES}

_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Load the HIP library or raise loudly.  Never falls back to anything."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SigmaHipUnavailable(
            f"{LIB_PATH} is missing: build it with `python -m sigma_amd.build` "
            "(hipcc --offload-arch=gfx950).  sigma_amd has no CPU/eager fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 not found
        raise SigmaHipUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise SigmaHipUnavailable(f"{LIB_PATH} does not export {name}; rebuild") from e
        fn.restype, fn.argtypes = restype, argtypes
    if lib.sigma_scan_abi_version() != SIGMA_SCAN_ABI_VERSION:
        raise SigmaHipUnavailable(
            f"ABI mismatch: library {lib.sigma_scan_abi_version()} vs binding {SIGMA_SCAN_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def gemm_plan(p: GemmParams, form, lib=None) -> Optional[dict]:
    """sigma_gemm_plan decoded (include/sigma_gemm.h; host only): the kernel variant and regime of the launch `p`
    describes, None where the launch would be refused.  form: 'nt' / 'nn' / 'tn' or 0 / 1 / 2."""
    out = (ctypes.c_int32 * 8)()
    f = GEMM_FORMS[form] if isinstance(form, str) else int(form)
    if (lib or load()).sigma_gemm_plan(ctypes.byref(p), f, ctypes.byref(out)) != 0:
        return None
    bits = out[7]
    return dict(form=("nt", "nn", "tn")[f], bn=out[0], ntm=out[1], ntn=out[2], slices=out[3], slice_k=out[4], items=out[5],
                pieces=out[6] & 15, res=bool(out[6] & 16), epilogue=GEMM_EPILOGUES[bits & 3], res_load=GEMM_RES_LOADS[(bits >> 2) & 3],
                summed=bool(bits & 16), two_stage=bool(bits & 32), store=GEMM_STORES[(bits >> 6) & 3], reduce_vec=bool(bits & 256))


def last_error() -> str:
    """The library's error text: the reason of the non-zero status (or negative size) that an entry point of any of the
    three headers -- sigma_scan.h, sigma_ops.h, sigma_gemm.h -- just returned ON THIS THREAD.  Every refusal and every
    failed launch writes it and no success does, so read it right after the call it belongs to: after a success it
    still holds the text of an earlier failure."""
    return load().sigma_scan_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    """raise ``RuntimeError("{what}: {last_error()} (sigma_status {rc})")`` for the non-zero status `rc` that an entry
    point of any of the three headers just returned on this thread"""
    if rc != 0:
        raise RuntimeError(f"{what}: {last_error()} (sigma_status {rc})")


def set_option(name: str, value: int) -> None:
    check(load().sigma_scan_set_option(name.encode(), int(value)), f"sigma_scan_set_option({name})")


def get_option(name: str) -> int:
    return int(load().sigma_scan_get_option(name.encode()))
