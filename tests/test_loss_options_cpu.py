"""Host side of the criterion options (class weights, label smoothing, reduction 'sum' / 'none') of the segmentation loss:
the element-wise formulation ``pointwise.cross_entropy_deterministic`` against torch in fp64, the layout of
sigma_ce_opt_params against gcc, the argument checks of sigma_softmax_ce_opt_fwd / _bwd and the routing of a criterion --
no GPU, no launch is reached."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from sigma_amd import _capi
from tests.capi_refusals import assert_refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255
NC = 9
OPTIONS = [(w, eps, red) for w, eps, red in itertools.product((True, False), (0.0, 0.1), ("mean", "sum", "none"))
           if (w, eps, red) != (False, 0.0, "mean")]


def _inputs():
    g = torch.Generator().manual_seed(31)
    logits = torch.randn(2, NC, 9, 11, generator=g, dtype=torch.float64) * 3.0
    label = torch.randint(0, NC, (2, 9, 11), generator=g)
    label[torch.rand(2, 9, 11, generator=g) < 0.1] = IGNORE
    weight = torch.rand(NC, generator=g, dtype=torch.float64) * 2.0 + 0.1
    weight[4] = 0.0
    return logits, label, weight


@pytest.mark.parametrize("opt", OPTIONS, ids=[f"{'w' if w else 'now'}-eps{e}-{r}" for w, e, r in OPTIONS])
def test_elementwise_formulation_against_torch_in_fp64(opt):
    """(2, 9, 9, 11) fp64 logits, ~10 % ignored pixels, class 4 with weight 0: loss and gradient of
    cross_entropy_deterministic against F.cross_entropy, assert_close at the fp64 defaults"""
    from sigma_amd.pointwise import cross_entropy_deterministic
    has_w, eps, red = opt
    logits, label, weight = _inputs()
    assert bool((label == 4).any()) and bool((label == IGNORE).any())
    crit = nn.CrossEntropyLoss(weight=weight if has_w else None, ignore_index=IGNORE, reduction=red, label_smoothing=eps)
    a = logits.clone().requires_grad_()
    got = cross_entropy_deterministic(crit, a, label)
    assert got is not None
    b = logits.clone().requires_grad_()
    want = F.cross_entropy(b, label, weight=weight if has_w else None, ignore_index=IGNORE, reduction=red, label_smoothing=eps)
    assert got.shape == want.shape and got.dtype == torch.float64
    torch.testing.assert_close(got, want)
    up = torch.randn(want.shape, generator=torch.Generator().manual_seed(32), dtype=torch.float64)
    (got * up).sum().backward()
    (want * up).sum().backward()
    torch.testing.assert_close(a.grad, b.grad)
    if red == "none":
        assert bool((got.detach()[label == IGNORE] == 0).all())


def test_elementwise_formulation_keeps_the_plain_case_and_its_refusals():
    from sigma_amd.pointwise import cross_entropy_deterministic
    logits, label, weight = _inputs()
    plain = nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    torch.testing.assert_close(cross_entropy_deterministic(plain, logits, label), F.cross_entropy(logits, label, ignore_index=IGNORE))

    class Mine(nn.CrossEntropyLoss):
        pass

    assert cross_entropy_deterministic(Mine(ignore_index=IGNORE), logits, label) is None
    assert cross_entropy_deterministic(nn.CrossEntropyLoss(weight=weight[:5]), logits, label) is None
    assert cross_entropy_deterministic(nn.NLLLoss(), logits, label) is None


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of sigma_ce_opt_params by gcc against the ctypes mirror"""
    cname, cls = "sigma_ce_opt_params", _capi.CeOptParams
    lines = [f'printf("%s %zu\\n", "{cname}", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("%s.%s %zu\\n", "{cname}", "{fname}", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_ops.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    assert len(got) == 1 + len(cls._fields_)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    body = header[header.index("typedef struct sigma_ce_opt_params {"):header.index("} sigma_ce_opt_params;")]
    assert body.count(";") == len(cls._fields_) - 1                 # `classes, ld` share a declaration: no field is missing
    assert {"sigma_softmax_ce_opt_fwd", "sigma_softmax_ce_opt_bwd"} <= set(_capi.OPS_SYMBOLS)
    assert _capi.SIGMA_SCAN_ABI_VERSION == 13 and _capi.load().sigma_scan_abi_version() == 13


OK, ODD16, ODD4 = 0x10000, 0x10004, 0x10002      # never dereferenced: every call below is refused, or has no rows


def _params(**kw):
    p = _capi.CeOptParams()
    p.rows, p.classes, p.ld, p.ignore_index, p.label_smoothing = 8, 9, 12, IGNORE, 0.1
    for f in ("logits", "labels", "weight", "lse", "row_loss", "partial", "scale", "dlogits"):
        setattr(p, f, OK)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _capi.load()
    ERR = 1                                                      # SIGMA_OPS_ERR_ARG
    # fwd / bwd: the status of a call that must be refused -- with a reason of its own in the error text (assert_refused)
    fwd = lambda **kw: assert_refused(lib.sigma_softmax_ce_opt_fwd, ctypes.byref(_params(**kw)), None, code=ERR, msg=kw) and ERR
    bwd = lambda **kw: assert_refused(lib.sigma_softmax_ce_opt_bwd, ctypes.byref(_params(**kw)), None, code=ERR, msg=kw) and ERR
    bwd_status = lambda **kw: lib.sigma_softmax_ce_opt_bwd(ctypes.byref(_params(**kw)), None)
    assert_refused(lib.sigma_softmax_ce_opt_fwd, None, None, says="NULL")
    assert_refused(lib.sigma_softmax_ce_opt_bwd, None, None, says="NULL")
    for f in (fwd, bwd):
        assert f(classes=0) == ERR and f(classes=-3) == ERR                      # classes < 1
        assert f(ld=10) == ERR and f(ld=9) == ERR and f(ld=13) == ERR            # ld % 4 != 0
        assert f(ld=8) == ERR and f(classes=13) == ERR                           # ld < classes
        assert f(rows=-1) == ERR
        for eps in (-0.01, 1.5, float("nan"), float("inf")):                     # eps outside [0, 1]
            assert f(label_smoothing=eps) == ERR, eps
        assert f(logits=ODD16) == ERR and f(weight=ODD4) == ERR and f(lse=ODD4) == ERR and f(labels=ODD16) == ERR
        assert f(logits=None) == ERR and f(labels=None) == ERR and f(lse=None) == ERR
    assert fwd(partial=None) == ERR and fwd(rows=0, partial=None) == ERR and fwd(row_loss=ODD4) == ERR and fwd(partial=ODD4) == ERR
    assert bwd(dlogits=None) == ERR and bwd(dlogits=ODD16) == ERR
    # exactly one of scale and row_grad -- checked even when there is nothing to write
    for rows in (8, 0):
        assert bwd(rows=rows, scale=OK, row_grad=OK) == ERR and bwd(rows=rows, scale=None, row_grad=None) == ERR
    assert bwd(row_grad=ODD4, scale=None) == ERR and bwd(scale=ODD4) == ERR
    # nothing to write: success without a launch, with either gradient and with the optional pointers absent
    assert bwd_status(rows=0, logits=None, dlogits=None, weight=None) == 0
    assert bwd_status(rows=0, logits=None, dlogits=None, scale=None, row_grad=OK, label_smoothing=0.0) == 0
    assert bwd_status(rows=0, label_smoothing=1.0) == 0


class _Sub(nn.CrossEntropyLoss):
    pass


def test_routing_of_a_criterion():
    """plain -> SoftmaxCEFn, options -> SoftmaxCEOptFn, declined: a subclass, another loss, a weight on another device, of
    another dtype or size"""
    from sigma_amd.pointwise import criterion_route, cross_entropy
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    CE = nn.CrossEntropyLoss
    for dev in (cpu, gpu):
        assert criterion_route(CE(reduction="mean", ignore_index=IGNORE), dev, 9) == "plain"
        assert criterion_route(CE(), dev, 9) == "plain"
        for kw in (dict(reduction="sum"), dict(reduction="none"), dict(label_smoothing=0.1), dict(label_smoothing=1.0),
                   dict(reduction="sum", label_smoothing=0.1)):
            assert criterion_route(CE(ignore_index=IGNORE, **kw), dev, 9) == "options", kw
        assert criterion_route(_Sub(), dev, 9) is None and criterion_route(_Sub(reduction="sum"), dev, 9) is None
        assert criterion_route(nn.NLLLoss(), dev, 9) is None
    w = torch.rand(9)
    assert criterion_route(CE(weight=w), cpu, 9) == "options"
    assert criterion_route(CE(weight=w, label_smoothing=0.1, reduction="none"), cpu, 9) == "options"
    assert criterion_route(CE(weight=w), gpu, 9) is None                     # a CPU weight for GPU logits
    assert criterion_route(CE(weight=w), cpu, 12) is None and criterion_route(CE(weight=w.view(3, 3)), cpu, 9) is None
    assert criterion_route(CE(weight=w.double()), cpu, 9) is None and criterion_route(CE(weight=w.half()), cpu, 9) is None
    assert criterion_route(CE(weight=w.double()), cpu, 9, any_float_weight=True) == "options"
    # cross_entropy itself still declines CPU logits, whatever the criterion
    buf = torch.randn(2, 3, 5, 12)
    label = torch.zeros(2, 3, 5, dtype=torch.long)
    for crit in (CE(), CE(weight=w), CE(reduction="none", label_smoothing=0.1)):
        assert cross_entropy(crit, buf[..., :9].permute(0, 3, 1, 2), label) is None
