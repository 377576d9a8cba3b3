"""FocalLoss2d without a GPU: the fp64 twin (tests/focal_fp64_twin.py) against the reference's own output
(tests/golden/loss_focal.npz, made by tests/golden/make_golden_focal.py), the class on CPU tensors against the same
fixture, the host side of sigma_softmax_focal_fwd / _bwd (include/sigma_ops.h), and the bounds and inputs of
tests/test_focal_gpu.py against an fp32 emulation of the kernels' formulas (tests/focal_bounds.py).

Formula identities are held to rtol 1e-12 (atol 1e-12 for the gradient's elements), as the project's other formula-identity
checks (tests/test_loss_options_gpu.py, tests/test_ohem_cpu.py).
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sigma_amd import _capi
from tests.capi_refusals import assert_refused
from tests import focal_bounds as fb
from tests.focal_fp64_twin import VARIANTS, twin
from tests.test_stream_fp64_gpu import check, rejects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255
NAMES = ("mean", "sum", "none", "gamma_0_passed", "gamma_3p5_passed", "weighted_mean", "no_valid")
FAMILY = "focal loss (fp32 emulation)"


def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "loss_focal.npz"))
    cases = {}
    for name in [str(n) for n in z["cases"]]:
        w = z[f"{name}.weight"]
        cases[name] = dict(x=torch.from_numpy(z[f"{name}.x"]), target=torch.from_numpy(z[f"{name}.target"]),
                           gamma=float(z[f"{name}.gamma"]), reduction=str(z[f"{name}.reduction"]),
                           weight=torch.from_numpy(w) if w.size else None, loss=torch.from_numpy(z[f"{name}.loss"]),
                           grad=torch.from_numpy(z[f"{name}.grad"]))
    return cases


FIXTURE = _fixture()


def _rows(c):
    x = c["x"]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]), c["target"].reshape(-1)


def _same(got, want, atol=0.0):
    if bool(torch.isnan(want).any()):
        assert bool(torch.isnan(want).all()) and bool(torch.isnan(got).all())
    else:
        torch.testing.assert_close(got, want, rtol=1e-12, atol=atol)


def test_fixture_holds_the_cases():
    assert set(FIXTURE) == set(NAMES)
    assert FIXTURE["weighted_mean"]["weight"] is not None and FIXTURE["sum"]["reduction"] == "sum"
    assert tuple(FIXTURE["none"]["loss"].shape) == tuple(FIXTURE["none"]["target"].shape)
    assert bool((FIXTURE["no_valid"]["target"] == IGNORE).all())
    ignored = float((FIXTURE["mean"]["target"] == IGNORE).double().mean())
    assert 0.05 < ignored < 0.25


def test_the_reference_ignores_its_gamma():
    """gamma passed as 0 and as 3.5 on the inputs of 'mean': the reference's loss and gradient do not move by a bit"""
    base = FIXTURE["mean"]
    for other in ("gamma_0_passed", "gamma_3p5_passed"):
        c = FIXTURE[other]
        assert c["gamma"] != 2 and torch.equal(c["x"], base["x"]) and torch.equal(c["target"], base["target"])
        assert torch.equal(c["loss"], base["loss"]) and torch.equal(c["grad"], base["grad"])


@pytest.mark.parametrize("name", NAMES)
def test_twin_reproduces_the_reference(name):
    """exponent 2 whatever gamma the case passed; 'none' stores the gradient of the summed map"""
    c = FIXTURE[name]
    x, lab = _rows(c)
    t = twin(x, lab, IGNORE, 2.0, weight=c["weight"], reduction=c["reduction"])
    _same(t["loss"].reshape(c["loss"].shape), c["loss"])
    _same(t["dl"], c["grad"].permute(0, 2, 3, 1).reshape(-1, x.shape[1]), atol=1e-12)
    if name == "no_valid":
        assert bool(torch.isnan(c["loss"])) and bool((t["dl"] == 0).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_twins_fail_the_fixture(variant):
    """'detached' fails every gradient, 'den_count' the weighted mean; 'square' IS the reference (its exponent is 2), so it
    is held against the twin at gamma = 3.5 instead"""
    c = FIXTURE["weighted_mean"]
    x, lab = _rows(c)
    wrong = twin(x, lab, IGNORE, 3.5 if variant == "square" else 2.0, weight=c["weight"], reduction="mean", variant=variant)
    want = twin(x, lab, IGNORE, 3.5, weight=c["weight"], reduction="mean") if variant == "square" else None
    loss, grad = (want["loss"], want["dl"]) if want else (c["loss"], c["grad"].permute(0, 2, 3, 1).reshape(-1, x.shape[1]))
    if variant == "square":
        _same(wrong["loss"], c["loss"])                       # exponent 2 on gamma = 3.5: the reference's number
    if variant != "detached":
        assert abs(float(wrong["loss"] - loss)) > 1e-3 * abs(float(loss))
    assert float((wrong["dl"] - grad).abs().max()) > 1e-3 * float(grad.abs().max())


def test_gamma_zero_is_the_cross_entropy():
    for name in ("mean", "sum", "none", "weighted_mean"):
        c = FIXTURE[name]
        x, lab = _rows(c)
        z = x.clone().requires_grad_()
        want = F.cross_entropy(z, lab, weight=c["weight"], ignore_index=IGNORE, reduction=c["reduction"])
        want.sum().backward()
        t = twin(x, lab, IGNORE, 0.0, weight=c["weight"], reduction=c["reduction"])
        _same(t["loss"], want.detach())
        _same(t["dl"], z.grad, atol=1e-12)


@pytest.mark.parametrize("gamma", [1.0, 3.5])
def test_twin_gradient_is_autograd_of_its_loss(gamma):
    """the dlogits formula against autograd of the torch formulation at the exponents the fixture cannot reach"""
    c = FIXTURE["weighted_mean"]
    x, lab = _rows(c)
    z = x.clone().requires_grad_()
    loss = F.nll_loss((1 - F.softmax(z, 1)) ** gamma * F.log_softmax(z, 1), lab, weight=c["weight"], ignore_index=IGNORE)
    loss.backward()
    t = twin(x, lab, IGNORE, gamma, weight=c["weight"], reduction="mean")
    _same(t["loss"], loss.detach())
    _same(t["dl"], z.grad, atol=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_class_on_the_cpu_matches_the_reference(name):
    """exponent=None, the case's gamma passed through; the weighted case in fp64 needs .double() on the module (the fp32
    weight of nn.NLLLoss refuses fp64 inputs, in the reference too), which rounds the fixture's fp64 weights to fp32: that
    case is held against the twin with the rounded weights, and the twin against the fixture by the test above"""
    from sigma_amd.utils.loss_opr import FocalLoss2d
    c = FIXTURE[name]
    crit = FocalLoss2d(gamma=c["gamma"], weight=None if c["weight"] is None else c["weight"].tolist(), reduction=c["reduction"],
                       ignore_index=IGNORE)
    want_loss, want_grad = c["loss"], c["grad"]
    if c["weight"] is not None:
        assert crit.loss.weight.dtype == torch.float32 and list(crit.state_dict()) == ["loss.weight"]
        with pytest.raises(RuntimeError):
            crit(c["x"], c["target"])
        w32 = crit.loss.weight.clone()
        crit = crit.double()
        x, lab = _rows(c)
        t = twin(x, lab, IGNORE, 2.0, weight=w32.double(), reduction=c["reduction"])
        want_loss, want_grad = t["loss"], t["dl"].view(2, 8, 8, -1).permute(0, 3, 1, 2)
    z = c["x"].clone().requires_grad_()
    loss = crit(z, c["target"])
    loss.sum().backward()
    _same(loss.detach(), want_loss)
    _same(z.grad, want_grad, atol=1e-12)


def test_class_signature_exponent_and_weight_forms():
    from sigma_amd.utils.loss_opr import FocalLoss2d
    names = list(inspect.signature(FocalLoss2d.__init__).parameters)
    assert names == ["self", "gamma", "weight", "reduction", "ignore_index", "exponent"]
    assert FocalLoss2d().exponent == 2.0 and FocalLoss2d(gamma=3.5).exponent == 2.0 and FocalLoss2d(gamma=3.5).gamma == 3.5
    assert FocalLoss2d(exponent=0.5).exponent == 0.5
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            FocalLoss2d(exponent=bad)
    c = FIXTURE["mean"]
    x, lab = _rows(c)
    w = [0.5, 1.0, 2.0, 0.25, 1.5]
    for form in (w, np.array(w), torch.tensor(w, dtype=torch.float64)):
        crit = FocalLoss2d(weight=form)
        assert isinstance(crit.loss, torch.nn.NLLLoss) and crit.loss.weight.dtype == torch.float32
        assert torch.equal(crit.loss.weight, torch.tensor(w))
    for e in (0.0, 0.5, 1.0, 3.5):                            # 0.5: declined by the kernels, the torch formulation takes it
        got = FocalLoss2d(exponent=e, weight=w).double()(c["x"], c["target"])
        if e == 0.5:                                          # outside the twin's (and the kernels') range: the torch formulation itself
            want = F.nll_loss((1 - F.softmax(c["x"], 1)) ** e * F.log_softmax(c["x"], 1), c["target"], weight=torch.tensor(w).double(),
                              ignore_index=IGNORE)
        else:
            want = twin(x, lab, IGNORE, e, weight=torch.tensor(w), reduction="mean")["loss"]
        _same(got, want)


def test_class_raises_nothing_under_the_deterministic_flag_on_cpu_tensors():
    from sigma_amd.utils.loss_opr import FocalLoss2d
    c = FIXTURE["mean"]
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        z = c["x"].clone().requires_grad_()
        loss = FocalLoss2d(ignore_index=IGNORE)(z, c["target"])
        loss.backward()
    finally:
        torch.use_deterministic_algorithms(was)
    _same(loss.detach(), c["loss"])
    _same(z.grad, c["grad"], atol=1e-12)


def test_deterministic_formulation_equals_the_twin():
    """pointwise.focal_deterministic (what the class uses on GPU tensors under the flag where the kernels decline), on CPU"""
    from sigma_amd.pointwise import focal_deterministic
    for name in ("mean", "sum", "none", "weighted_mean", "no_valid"):
        c = FIXTURE[name]
        x, lab = _rows(c)
        for gamma in (0.0, 2.0, 3.5):
            z = c["x"].clone().requires_grad_()
            loss = focal_deterministic(z, c["target"], IGNORE, gamma, weight=c["weight"], reduction=c["reduction"])
            loss.sum().backward()
            t = twin(x, lab, IGNORE, gamma, weight=c["weight"], reduction=c["reduction"])
            _same(loss.detach().reshape(-1) if c["reduction"] == "none" else loss.detach(), t["loss"])
            if t["den"] != 0:                                 # 0 / 0: the element-wise form differentiates to NaN, the kernels write zeros
                _same(z.grad.permute(0, 2, 3, 1).reshape(-1, x.shape[1]), t["dl"], atol=1e-12)


def _params(**kw):
    p = _capi.CeOptParams()
    p.rows, p.classes, p.ld, p.ignore_index, p.label_smoothing = 100, 5, 8, IGNORE, 0.0
    # never dereferenced: every call below is refused before any launch (aligned non-null addresses)
    p.logits, p.labels, p.lse, p.partial, p.scale, p.dlogits = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _capi.load()
    # every refusal is SIGMA_OPS_ERR_ARG (1) with a reason of its own in the error text
    fwd = lambda p, gamma=2.0, **kw: assert_refused(lib.sigma_softmax_focal_fwd, ctypes.byref(p), gamma, None, **kw)
    bwd = lambda p, gamma=2.0, **kw: assert_refused(lib.sigma_softmax_focal_bwd, ctypes.byref(p), gamma, None, **kw)
    assert_refused(lib.sigma_softmax_focal_fwd, None, 2.0, None, says="NULL")
    assert_refused(lib.sigma_softmax_focal_bwd, None, 2.0, None, says="NULL")
    for call in (fwd, bwd):
        for gamma in (float("nan"), -1.0, -0.0001, 0.5, 0.999, 1e-30, float("inf")):
            call(_params(), gamma, says="gamma", msg=gamma)
        call(_params(label_smoothing=0.1), says="label_smoothing")
        # everything the option entry points refuse
        for kw in (dict(rows=-1), dict(classes=0), dict(ld=6), dict(ld=4), dict(logits=None), dict(labels=None), dict(lse=None),
                   dict(logits=0x10004), dict(labels=0x20004), dict(lse=0x30002), dict(weight=0x70002), dict(row_loss=0x80002),
                   dict(partial=0x40002), dict(scale=0x50002), dict(row_grad=0x90002)):
            call(_params(**kw), msg=kw)
    fwd(_params(partial=None), says="partial")
    bwd(_params(dlogits=None), says="dlogits")
    bwd(_params(dlogits=0x60004), says="dlogits")
    bwd(_params(scale=None), says="row_grad")                 # neither scale nor row_grad
    bwd(_params(row_grad=0x90000), says="row_grad")           # both
    assert lib.sigma_softmax_focal_bwd(ctypes.byref(_params(rows=0)), 2.0, None) == 0      # nothing to do is a success without a launch
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    for name in ("sigma_softmax_focal_fwd", "sigma_softmax_focal_bwd"):
        assert name in _capi.OPS_SYMBOLS and f"int {name}(const sigma_ce_opt_params *params, float gamma, void *stream);" in header
    assert _capi.SIGMA_SCAN_ABI_VERSION == 13


def test_router_declines_what_the_kernels_do_not_take():
    """on CPU tensors everything is declined; the exponent is looked at before the layout"""
    from sigma_amd.pointwise import focal_cross_entropy
    c = FIXTURE["mean"]
    for gamma in (0.0, 0.5, 2.0, -1.0, float("nan")):
        assert focal_cross_entropy(c["x"].float(), c["target"], IGNORE, gamma) is None


@pytest.mark.parametrize("has_w", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("gamma", fb.GAMMAS)
@pytest.mark.parametrize("case", fb.CASES, ids=fb.CASE_IDS)
def test_bounds_hold_for_an_fp32_emulation_and_reject_the_wrong_kernels(case, gamma, has_w):
    """The inputs and bounds of the GPU kernel test on tests/focal_bounds.emulate_fp32: it passes ``check`` for lse,
    row_loss, both sums and dlogits (scalar and per-row upstream), and the three wrong kernels fail it -- the modulating
    factor detached (gamma > 0; where a row has q < 1, i.e. more than one class), the exponent 2 at gamma = 3.5, the pixel
    count as the mean's denominator (weighted)."""
    rows, nc, ld = case
    buf, lab, sat = fb.focal_inputs(rows, nc, ld, seed=401)
    w = fb.focal_weights(nc, seed=403) if has_w else None
    x32 = buf[:, :nc].contiguous()
    x64 = x32.double()
    assert bool(torch.isnan(buf[:, nc:]).all())
    r0 = fb.bounds(x64, lab, nc, w, gamma, 0.0)
    den = float(r0["wy"].sum())
    assert den > 0
    if rows >= 257 and nc > 1:
        assert sat.numel() == 8 and bool((r0["nll"][sat] < 1e-40).all())
    row_grad = torch.randn(rows, generator=torch.Generator().manual_seed(404))
    K = r0["K"]
    for g, what in ((0.7 / den, "scale"), (row_grad, "row gradient")):
        r = fb.bounds(x64, lab, nc, w, gamma, g)
        e = fb.emulate_fp32(x32, lab, nc, w, gamma, g)
        check(FAMILY, e["lse"], r["lse"], r["S_lse"], r["K_lse"], "lse")
        check(FAMILY, e["row"], r["row"], r["S_row"], K, "row_loss")
        check(FAMILY, e["row"].double().sum().view(1), r["row"].sum().view(1), r["S_row"].sum().view(1), fb.k_sum(rows) + K, "loss sum")
        check(FAMILY, e["wy"].double().sum().view(1), r["wy"].sum().view(1), r["wy"].sum().view(1), fb.k_sum(rows), "sum of w_y")
        check(FAMILY, e["dl"], r["dl"], r["S_dl"], K, f"dlogits ({what})")
        assert bool((e["row"][sat] == 0).all())
        if gamma > 0:
            assert bool((e["dl"][sat] == 0).all())
        if gamma > 0 and nc > 1:
            bad = fb.emulate_fp32(x32, lab, nc, w, gamma, g, variant="detached")
            rejects(bad["dl"], r["dl"], r["S_dl"], K, f"detached modulating factor ({what})")
            wrong = twin(x64, lab, IGNORE, gamma, weight=w, reduction="none", upstream=g, variant="detached")
            rejects(e["dl"], wrong["dl"], r["S_dl"], K, f"detached modulating factor, twin ({what})")
        if gamma == 3.5 and nc > 1:
            bad = fb.emulate_fp32(x32, lab, nc, w, gamma, g, variant="square")
            rejects(bad["row"], r["row"], r["S_row"], K, "exponent 2 at gamma 3.5 (row_loss)")
            rejects(bad["dl"], r["dl"], r["S_dl"], K, f"exponent 2 at gamma 3.5 ({what})")
    if has_w:
        count = r0["valid"].double().sum().view(1)
        got_den = fb.emulate_fp32(x32, lab, nc, w, gamma, 0.0)["wy"].double().sum().view(1)
        rejects(got_den, count, r0["wy"].sum().view(1), fb.k_sum(rows), "mean denominator = pixel count")
