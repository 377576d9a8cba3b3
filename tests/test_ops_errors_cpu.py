"""Every refusal of include/sigma_ops.h and include/sigma_gemm.h says why, in the library's one error text.

Three parts: a table with at least one refused call per entry point of the two headers (a new entry point cannot arrive
without one), the source rule that no csrc/*.hip returns a bare SIGMA_OPS_ERR_* code, and the regression itself: an
operator's refusal after a scan's refusal no longer reports the scan's reason.  No test here touches a device: every
refusal happens on the host before any launch, on addresses that are never dereferenced.
"""
import ctypes
import glob
import os
import re

import pytest

from sigma_amd import _capi
from tests.capi_refusals import assert_refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A, B, C, D, E = (ctypes.c_void_p(0x10000 * i) for i in range(1, 6))      # 16-byte aligned, non-NULL
ODD = ctypes.c_void_p(0x10004)                                             # 4-byte aligned only
NULL = None


def _struct(cls, **kw):
    p = cls()
    for k, v in kw.items():
        setattr(p, k, v)
    return ctypes.byref(p)


def _dw(**kw):
    return _struct(_capi.DwConvParams, **dict(dict(batch=1, channels=4, height=4, width=4, n_orders=2), **kw))


def _merge(**kw):
    return _struct(_capi.MergeParams, **dict(dict(batch=1, channels=4, height=4, width=4), **kw))


def _ln(**kw):
    return _struct(_capi.LayerNormParams, **dict(dict(rows=8, channels=8, eps=1e-5), **kw))


def _ce(**kw):
    good = dict(rows=8, classes=9, ld=12, ignore_index=255, logits=0x10000, labels=0x20000, lse=0x30000, partial=0x40000,
                scale=0x50000, dlogits=0x60000)
    return _struct(_capi.CeOptParams, **dict(good, **kw))


def _up(cls, **kw):
    good = dict(batch=2, height=3, width=5, scale=8, classes=9, ld=12, ignore_index=255, logits=0x10000, labels=0x20000,
                lse=0x30000, partial=0x40000, scale_grad=0x50000, dlogits=0x60000)
    return _struct(cls, **dict(good, **kw))


def _gemm(**kw):
    good = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, A=0x10000, Bt=0x20000, C=0x30000, batch=1, pieces=2)
    return _struct(_capi.GemmParams, **dict(good, **kw))


# entry point -> [(arguments without the stream where the last parameter is one, refused with, the text names)]
S = (NULL,)      # the stream argument
CASES = {
    "sigma_dwconv3x3_silu_fwd": [((NULL,) + S, 1, "NULL"), ((_dw(n_orders=3),) + S, 1, "n_orders"), ((_dw(),) + S, 1, "weight")],
    "sigma_dwconv3x3_silu_bwd": [((NULL,) + S, 1, "NULL"), ((_dw(flags=2),) + S, 1, "flags"),
                                 ((_dw(batch=0, flags=1),) + S, 1, "dweight")],
    "sigma_cross_merge_nhwc": [((NULL,) + S, 1, "NULL"), ((_merge(channels=0),) + S, 1, "channels"), ((_merge(),) + S, 1, "planes4")],
    "sigma_cross_split_nhwc": [((NULL,) + S, 1, "NULL"), ((_merge(width=-1),) + S, 1, "width"), ((_merge(),) + S, 1, "planes2")],
    "sigma_layernorm_fwd": [((NULL,) + S, 1, "NULL"), ((_ln(channels=6),) + S, 1, "channels"), ((_ln(rows=-1),) + S, 1, "rows"),
                            ((_ln(x=0x10000, gamma=0x20000, y=0x30000, gate=0x40000, gate_row_stride=6),) + S, 1, "gate_row_stride")],
    "sigma_layernorm_bwd": [((NULL,) + S, 1, "NULL"), ((_ln(channels=2052),) + S, 1, "channels"), ((_ln(),) + S, 1, "dgamma"),
                            ((_ln(dgamma=0x10000),) + S, 1, "workspace")],
    "sigma_transpose2d": [((NULL,) + S, 1, "NULL"), ((_struct(_capi.TransposeParams, batch=1, rows=0, cols=4),) + S, 1, "rows"),
                          ((_struct(_capi.TransposeParams, batch=1, rows=4, cols=4),) + S, 1, "src")],
    "sigma_pair_sum_add": [((A, B, -1, 4) + S, 1, "n_outer"), ((NULL, B, 1, 4) + S, 1, "src")],
    "sigma_upsample2x_nhwc": [((A, B, 1, 4, 4, 6, 0) + S, 1, "channels"), ((ODD, B, 1, 4, 4, 8, 0) + S, 1, "align")],
    "sigma_plane_pool": [((A, 1, 0, B, C, D) + S, 1, "hw"), ((A, 1, 4, NULL, C, D) + S, 1, "mean")],
    "sigma_plane_scale": [((A, B, C, -1, 4) + S, 1, "planes"), ((NULL, B, C, 1, 4) + S, 1, "x")],
    "sigma_plane_dot": [((A, B, C, 2 ** 31, 4) + S, 1, "planes"), ((A, B, NULL, 1, 4) + S, 1, "out")],
    "sigma_plane_gate_bwd": [((NULL,) + S, 1, "NULL"), ((_struct(_capi.GateBwdParams, planes=1, hw=0),) + S, 1, "hw"),
                             ((_struct(_capi.GateBwdParams, planes=1, hw=4),) + S, 1, "dmean")],
    "sigma_softmax_ce_fwd": [((A, B, 8, 9, 255, C, D) + S, 1, "classes")],
    "sigma_softmax_ce_bwd": [((A, B, C, D, 8, 9, 255, E) + S, 1, "classes")],
    "sigma_softmax_ce_fwd_ld": [((A, B, 8, 9, 8, 255, C, D) + S, 1, "ld"), ((ODD, B, 8, 9, 12, 255, C, D) + S, 1, "align"),
                                ((A, B, 8, 9, 12, 255, C, NULL) + S, 1, "partial")],
    "sigma_softmax_ce_bwd_ld": [((A, B, C, D, 8, 9, 10, 255, E) + S, 1, "ld"), ((A, B, C, D, 8, 9, 12, 255, ODD) + S, 1, "align")],
    "sigma_softmax_ce_opt_fwd": [((NULL,) + S, 1, "NULL"), ((_ce(label_smoothing=1.5),) + S, 1, "label_smoothing"),
                                 ((_ce(weight=0x70002),) + S, 1, "align"), ((_ce(ld=8),) + S, 1, "ld")],
    "sigma_softmax_ce_opt_bwd": [((NULL,) + S, 1, "NULL"), ((_ce(row_grad=0x70000),) + S, 1, "row_grad"),
                                 ((_ce(dlogits=0x60004),) + S, 1, "align")],
    "sigma_colscale_bwd": [((A, B, C, D, E, 8, 6) + S, 1, "channels"), ((A, B, C, D, NULL, 8, 8) + S, 1, "dscale"),
                           ((A, ODD, C, D, E, 8, 8) + S, 1, "align")],
    "sigma_colscale_bwd_ws": [((A, B, C, D, E, -1, 8, A, 1 << 20) + S, 1, "rows"), ((A, B, C, D, NULL, 8, 8, A, 1 << 20) + S, 1, "dscale"),
                              ((A, B, C, D, E, 8, 8, NULL, 0) + S, 1, "workspace"), ((A, B, C, D, E, 8, 8, A, 8) + S, 1, "workspace")],
    "sigma_seg_accumulate": [((NULL,) + S, 1, "NULL"),
                             ((_struct(_capi.SegAccumulateParams, pixels=12, classes=3, first=2),) + S, 1, "first")],
    "sigma_seg_argmax_confusion": [((NULL,) + S, 1, "NULL"),
                                   ((_struct(_capi.SegConfusionParams, pixels=64, classes=9, n_cl=0),) + S, 1, "n_cl")],
    "sigma_ohem_select": [((NULL,) + S, 1, "NULL"), ((_struct(_capi.OhemParams, rows=100, classes=5, thresh=0.0),) + S, 1, "thresh"),
                          ((_struct(_capi.OhemParams, rows=100, classes=5, thresh=0.7),) + S, 1, "workspace")],
    "sigma_softmax_focal_fwd": [((NULL, 2.0) + S, 1, "NULL"), ((_ce(), 0.5) + S, 1, "gamma"),
                                ((_ce(label_smoothing=0.1), 2.0) + S, 1, "label_smoothing")],
    "sigma_softmax_focal_bwd": [((NULL, 2.0) + S, 1, "NULL"), ((_ce(), float("nan")) + S, 1, "gamma")],
    "sigma_upsample_ce_fwd": [((NULL,) + S, 1, "NULL"), ((_up(_capi.UpsampleCeParams, scale=0),) + S, 1, "scale"),
                              ((_up(_capi.UpsampleCeParams, partial=None),) + S, 1, "partial")],
    "sigma_upsample_ce_bwd": [((NULL,) + S, 1, "NULL"), ((_up(_capi.UpsampleCeParams, classes=65, ld=68),) + S, 1, "classes"),
                              ((_up(_capi.UpsampleCeParams, dlogits=0x60008),) + S, 1, "align")],
    "sigma_upsample_loss_fwd": [((NULL,) + S, 1, "NULL"), ((_up(_capi.UpsampleLossParams, kind=2),) + S, 1, "kind"),
                                ((_up(_capi.UpsampleLossParams, kind=1, gamma=2.0),) + S, 1, "coef")],
    "sigma_upsample_loss_bwd": [((NULL,) + S, 1, "NULL"), ((_up(_capi.UpsampleLossParams, label_smoothing=-0.1),) + S, 1, "label_smoothing"),
                                ((_up(_capi.UpsampleLossParams, row_grad=0x70000),) + S, 1, "row_grad")],
    # the size queries answer -1
    "sigma_dwconv3x3_silu_bwd_workspace_bytes": [((NULL,), -1, "NULL"), ((_dw(height=0),), -1, "height")],
    "sigma_colscale_bwd_workspace_bytes": [((-1, 8), -1, "rows"), ((8, 1028), -1, "channels")],
    "sigma_ohem_workspace_bytes": [((-1,), -1, "rows"), ((2 ** 31,), -1, "rows")],
    # include/sigma_gemm.h
    "sigma_gemm_nt_split3": [((NULL,) + S, 1, "NULL"), ((_gemm(K=6),) + S, 1, "K"), ((_gemm(A=0x10004),) + S, 1, "align"),
                             ((_gemm(pieces=4),) + S, 1, "pieces"), ((_gemm(residual=0x40000, ldr=64, pieces=3),) + S, 1, "residual")],
    "sigma_gemm_nn_split3": [((NULL,) + S, 1, "NULL"), ((_gemm(N=6),) + S, 1, "N"), ((_gemm(lda=0),) + S, 1, "lda")],
    "sigma_gemm_tn_split3": [((NULL,) + S, 1, "NULL"), ((_gemm(bias=0x40000),) + S, 1, "bias"), ((_gemm(C=None),) + S, 1, "C")],
    "sigma_gemm_workspace_bytes": [((_gemm(), 7), -1, "form"), ((NULL, 0), -1, "NULL"), ((_gemm(K=6), 1), -1, "K")],
    "sigma_gemm_plan": [((_gemm(), 0, NULL), 1, "out"), ((_gemm(reserved=1), 0, ctypes.byref((ctypes.c_int32 * 8)())), 1, "reserved"),
                        ((_gemm(), 3, ctypes.byref((ctypes.c_int32 * 8)())), 1, "form")],
}
# no argument of these can be refused: a self test that takes a stream, and a host-side count that clamps its inputs
UNREFUSABLE = {"sigma_gemm_selftest", "sigma_layernorm_bwd_partial_rows"}
ENTRY_POINTS = _capi.OPS_SYMBOLS + _capi.OPS_AUX_SYMBOLS + _capi.GEMM_SYMBOLS + _capi.GEMM_AUX_SYMBOLS


def test_the_table_covers_the_two_headers():
    assert UNREFUSABLE <= set(ENTRY_POINTS)
    assert set(CASES) == set(ENTRY_POINTS) - UNREFUSABLE
    assert all(len(cases) >= 1 for cases in CASES.values())


@pytest.mark.parametrize("name", [n for n in ENTRY_POINTS if n not in UNREFUSABLE])
def test_every_refusal_names_the_offending_field(name):
    assert name in CASES, f"{name}: a new entry point needs a refusal case here"
    fn = getattr(_capi.load(), name)
    for args, code, says in CASES[name]:
        text = assert_refused(fn, *args, code=code, says=says, msg=(name, says))
        assert name not in text and name[len("sigma_"):] not in text, f"the caller's label names the entry point, not the reason: {text}"


def test_no_bare_ops_status_is_returned():
    """every non-zero return of csrc/*.hip goes through sigma::fail (capi_error.h) or sigma::launched (ops_host.h)"""
    sources = sorted(glob.glob(os.path.join(ROOT, "sigma_amd", "csrc", "*.hip")))
    assert len(sources) >= 19
    bare = [f"{os.path.basename(src)}:{i}: {line.strip()}" for src in sources
            for i, line in enumerate(open(src), 1) if re.search(r"return SIGMA_OPS_ERR_", line)]
    assert not bare, "\n".join(bare)


def test_an_operators_refusal_does_not_report_an_earlier_scan_refusal():
    """the sequence of the issue: a refused scan query, then two refused operator calls, raised as the launch layer does"""
    lib = _capi.load()
    scan = _capi.FwdParams()
    scan.batch, scan.dim, scan.seqlen, scan.dstate, scan.n_groups, scan.n_chunks = 1, 6, 100, 4, 4, 1
    assert lib.sigma_scan_fwd_workspace_bytes(ctypes.byref(scan)) < 0 and "n_groups" in _capi.last_error()
    with pytest.raises(RuntimeError) as e:
        _capi.check(lib.sigma_ohem_select(_struct(_capi.OhemParams, rows=100, classes=5, thresh=0.0), None), "ohem_select")
    assert str(e.value).startswith("ohem_select: ") and "thresh" in str(e.value) and "n_groups" not in str(e.value)
    assert str(e.value).endswith("(sigma_status 1)")
    with pytest.raises(RuntimeError) as e:
        _capi.check(lib.sigma_layernorm_fwd(_ln(channels=6), None), "layernorm_fwd")
    assert "channels 6" in str(e.value) and "n_groups" not in str(e.value) and str(e.value).endswith("(sigma_status 1)")
    # a success writes nothing: the text is still the LayerNorm reason
    assert lib.sigma_layernorm_fwd(_ln(rows=0), None) == 0 and "channels 6" in _capi.last_error()
