"""The loss kernels on saturated, shifted, swept, sorted, tied, masked and non-finite logits -- run with -m gpu.  The regimes,
the fp64 references, the bounds (the existing ones plus the two additions derived there) and the fp32 emulation that
tests/test_loss_regimes_cpu.py holds under the same bounds on the same inputs are in tests/loss_regimes.py.

Every entry point of the family through the C ABI, all outputs inside NaN guard bands: sigma_softmax_ce_fwd_ld / _bwd_ld,
sigma_softmax_ce_opt_fwd / _bwd (weights, smoothing, both; device scalar and row gradient; ``masked`` without smoothing,
where torch itself returns inf or NaN), sigma_softmax_focal_fwd / _bwd at four exponents with and without weights, at the
register cases (up to 64 classes) and the walking cases (65 to 130).  Then ``pointwise.cross_entropy`` and
``focal_cross_entropy`` with 'mean', ProbOhemCrossEntropy2d on its threshold branch and the fused upsample + cross-entropy
kernels on coarse logits of the regimes.

Through the front ends 300 rows are two workgroups: torch adds two non-zero partial pairs, one rounding more than the
256-row tests of tests/test_loss_options_gpu.py have (nb - 1 = 1, as tests/test_ohem_gpu.py derives): K_den = _k_sum + 1,
loss K = (K of the sum + 1) + K_den + 1 on S / den, gradient K = (K of dlogits) + K_den + 2.

Before the fix of softmax_ce_fwd_kernel the walking ``masked`` cases fail here with NaN lse -- exp(-inf - (-inf)) on a
first chunk that is masked whole -- and nothing else does.
Worst error / bound seen on an MI355X (``test_zz_report_worst_ratios`` prints the table, DESIGN.md 4.4 holds it): 0.40 under
the existing bounds (the walk on the sorted rows), 0.81 under the sharper lse bound of ``offset``, whose first term is the
half ulp of the final add alone; 0.23 through the front ends, 0.03 through OHEM, 0.10 on the fused upsample kernels.
"""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn as nn

from tests import deepsup_bounds as db
from tests import loss_regimes as lr
from tests.ohem_fp64_twin import twin as ohem_twin
from tests.test_stream_fp64_gpu import WORST, _guarded, _intact, check

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGNORE = lr.IGNORE
PREFIX = "loss regimes"
_IN: dict = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _family(nc, regime):
    return f"{PREFIX} {lr.form_of(nc)} {regime}"


def _inputs(regime, case, seed=701):
    """the case's inputs on the device, made once per (regime, case): buf, lab, the fp64 logits and the class weights"""
    key = (regime, case, seed)
    if key not in _IN:
        rows, nc, ld = case
        buf, lab = lr.regime_inputs(regime, rows, nc, ld, seed)[:2]
        _IN[key] = (buf.to(DEV), lab.to(DEV), buf[:, :nc].double().to(DEV), lr.weights(nc, seed=703).to(DEV))
    return _IN[key]


def _k_sum(rows):
    from sigma_amd import _capi
    return -(-rows // (256 * _capi.SIGMA_CE_BLOCKS)) + 10


def _row_grad(rows):
    return torch.randn(rows, generator=torch.Generator().manual_seed(704)).to(DEV)


def _run(kind, param, buf, lab, w, nc, ld, scale, row_grad):
    """One kind of the family through the C ABI on (rows, ld) logits.  kind "plain": sigma_softmax_ce_fwd_ld / _bwd_ld;
    "opt" (param = eps) and "focal" (param = gamma): the option entry points, forward with a row loss, backward with the
    device scalar and with the row gradient.  Returns the guarded outputs: lse, row_loss (None for plain), partial, dlogits
    (scalar), dlogits (row gradient; None for plain)."""
    from sigma_amd import _capi
    lib = _capi.load()
    rows = buf.shape[0]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    glse, part, gdl_s = _guarded((rows,), 64), _guarded((_capi.SIGMA_CE_BLOCKS, 2), 2), _guarded((rows, ld), ld)
    if kind == "plain":
        _capi.check(lib.sigma_softmax_ce_fwd_ld(vp(buf), vp(lab), rows, nc, ld, IGNORE, vp(glse[1]), vp(part[1]), _stream()), "ce fwd ld")
        _capi.check(lib.sigma_softmax_ce_bwd_ld(vp(buf), vp(lab), vp(glse[1]), vp(scale), rows, nc, ld, IGNORE, vp(gdl_s[1]), _stream()),
                    "ce bwd ld")
        torch.cuda.synchronize()
        outs = (glse, None, part, gdl_s, None)
    else:
        grow, gdl_r = _guarded((rows,), 64), _guarded((rows, ld), ld)
        p = _capi.CeOptParams()
        p.rows, p.classes, p.ld, p.ignore_index = rows, nc, ld, IGNORE
        p.label_smoothing = param if kind == "opt" else 0.0
        p.logits, p.labels, p.lse = buf.data_ptr(), lab.data_ptr(), glse[1].data_ptr()
        p.weight = w.data_ptr() if w is not None else None
        p.row_loss, p.partial = grow[1].data_ptr(), part[1].data_ptr()
        extra = () if kind == "opt" else (param,)
        fwd, bwd = (lib.sigma_softmax_ce_opt_fwd, lib.sigma_softmax_ce_opt_bwd) if kind == "opt" else (lib.sigma_softmax_focal_fwd,
                                                                                                      lib.sigma_softmax_focal_bwd)
        _capi.check(fwd(ctypes.byref(p), *extra, _stream()), f"{kind} fwd")
        p.scale, p.row_grad, p.dlogits = scale.data_ptr(), None, gdl_s[1].data_ptr()
        _capi.check(bwd(ctypes.byref(p), *extra, _stream()), f"{kind} bwd (scale)")
        p.scale, p.row_grad, p.dlogits = None, row_grad.data_ptr(), gdl_r[1].data_ptr()
        _capi.check(bwd(ctypes.byref(p), *extra, _stream()), f"{kind} bwd (row gradient)")
        torch.cuda.synchronize()
        outs = (glse, grow, part, gdl_s, gdl_r)
    for gg, what in zip(outs, ("lse", "row_loss", "partial", "dlogits", "dlogits (row gradient)")):
        if gg is not None:
            _intact(gg, what)
    return outs


def _reference(kind, param, x, lab, nc, w, g):
    """the fp64 reference of a kind with its S and K: (dict, K_row, K_dl, K of the rows inside the loss sum)"""
    if kind == "plain":
        return lr.plain_ref(x, lab, nc, g), None, nc + 16, 8 + nc + 8 - 10
    if kind == "opt":
        return lr.opt_ref(x, lab, nc, w, param, g), 2 * nc + 16, 2 * nc + 24, 2 * nc + 16
    r = lr.focal_ref(x, lab, nc, w, param, g)
    return r, r["K"], r["K"], r["K"]


def _check_kind(regime, case, kind, param, has_w):
    """lse, row_loss, both columns of the summed partials and dlogits under the bounds; the pad and the ignored rows of
    dlogits exact zeros; on ``offset`` lse under the sharper bound; on ``masked`` everything finite (``check`` asserts it)
    and dlogits exactly zero at masked columns.  Returns the ratios."""
    rows, nc, ld = case
    fam = _family(nc, regime)
    buf, lab, x, w_all = _inputs(regime, case)
    w = w_all if has_w else None
    r0, K_row, K_dl, K_in_sum = _reference(kind, param, x, lab, nc, w, 0.0)
    den = float(r0["wy"].sum())
    assert den > 0
    scale = torch.tensor([0.7 / den], device=DEV)
    row_grad = _row_grad(rows)
    glse, grow, part, gdl_s, gdl_r = _run(kind, param, buf, lab, w, nc, ld, scale, row_grad)
    valid, masked = r0["valid"], torch.isinf(buf[:, :nc])
    ratios = {"lse": check(fam, glse[1], r0["lse"], r0["S_lse"], nc + 8, "lse")}
    if regime == "offset":
        ratios["lse sharp"] = check(fam + " sharp", glse[1], r0["lse"], lr.lse_offset_bound(r0["lse"], nc) / lr.U, 1, "lse (sharper bound)")
    if grow is not None:
        ratios["row_loss"] = check(fam, grow[1], r0["row"], r0["S_row"], K_row, "row_loss")
        assert bool((grow[1][~valid] == 0).all()), "row_loss of an ignored row is not zero"
    assert torch.isfinite(part[1]).all(), "non-finite partial sums"
    got_sum, got_den = part[1][:, 0].double().sum().view(1), part[1][:, 1].double().sum().view(1)
    ratios["loss sum"] = check(fam, got_sum, r0["row"].sum().view(1), r0["S_row"].sum().view(1), _k_sum(rows) + K_in_sum, "loss sum")
    if kind == "plain":
        assert float(got_den) == den, "the plain kernels count the valid rows exactly"
    else:
        ratios["den"] = check(fam, got_den, r0["wy"].sum().view(1), r0["wy"].sum().view(1), _k_sum(rows), "sum of w_y")
    for gdl, g, what in ((gdl_s, float(scale), "scale"), (gdl_r, row_grad, "row gradient")):
        if gdl is None:
            continue
        r = _reference(kind, param, x, lab, nc, w, g)[0]
        S = r["S_dl"]
        if kind != "focal" and regime in lr.SUBNORMAL_REGIMES:
            S = S + lr.underflow_S(r["f"], K_dl)
        ratios["dlogits " + what] = check(fam, gdl[1][:, :nc], r["dl"], S, K_dl, f"dlogits ({what})")
        pad = gdl[1][:, nc:]
        assert pad.numel() == rows * (ld - nc) and bool((pad == 0).all()), "pad columns of dlogits are not exact zeros"
        assert bool((gdl[1][~valid] == 0).all()), "dlogits of an ignored row are not exact zeros"
        assert bool((gdl[1][:, :nc][masked] == 0).all()), "dlogits of a masked class are not exact zeros"
    return ratios


def _show(tag, ratios):
    print(f"\n{tag}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + " of the bound")


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
@pytest.mark.parametrize("regime", lr.FINITE_REGIMES)
def test_plain_kernels_on_the_regime(regime, case):
    _show(f"{regime} {case} plain", _check_kind(regime, case, "plain", None, False))


# ``masked`` runs without smoothing alone: with it torch itself returns inf or NaN on -inf logits, there is no reference
OPT_RUNS = [(regime, opt, oid) for regime in lr.FINITE_REGIMES for opt, oid in zip(lr.OPTS, lr.OPT_IDS) if not (regime == "masked" and opt[1] > 0)]


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
@pytest.mark.parametrize("regime,opt", [(r, o) for r, o, _ in OPT_RUNS], ids=[f"{r}-{i}" for r, _, i in OPT_RUNS])
def test_option_kernels_on_the_regime(regime, opt, case):
    has_w, eps = opt
    _show(f"{regime} {case} {opt}", _check_kind(regime, case, "opt", eps, has_w))


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
@pytest.mark.parametrize("regime", lr.FINITE_REGIMES)
def test_focal_kernels_on_the_regime(regime, case):
    """gamma 0, 1, 2, 3.5, with and without weights"""
    worst = {}
    for gamma in lr.GAMMAS:
        for has_w in (False, True):
            for k, v in _check_kind(regime, case, "focal", gamma, has_w).items():
                worst[k] = max(worst.get(k, 0.0), v)
    _show(f"{regime} {case} focal", worst)


@pytest.mark.parametrize("case", [(300, 9, 12), (300, 68, 68)], ids=["300x9@12", "300x68@68"])
def test_restated_references_are_the_existing_ones(case):
    """``plain_ref`` / ``opt_ref`` of tests/loss_regimes.py against ``_ce_ref`` of tests/test_head_classes_gpu.py and ``_ref``
    of tests/test_loss_options_gpu.py on finite logits: the same formulas and the same S (rtol 1e-12, atol 1e-12 for an element
    of the gradient that cancels, as the project's other formula-identity checks)"""
    from tests.test_head_classes_gpu import _ce_ref
    from tests.test_loss_options_gpu import _ref
    rows, nc, ld = case
    same = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    for regime in ("confident", "offset"):
        buf, lab, x, w = _inputs(regime, case)
        valid, lse, xl, dl, S_dl = _ce_ref(x, lab, nc, 0.01)
        r = lr.plain_ref(x, lab, nc, 0.01)
        for a, b in ((r["lse"], lse), (r["dl"], dl), (r["S_dl"], S_dl), (r["row"], torch.where(valid, lse - xl, torch.zeros_like(lse)))):
            same(a, b)
        for (has_w, eps), g in zip(lr.OPTS, (0.01, _row_grad(rows), 0.02)):
            want = _ref(x, lab, nc, w if has_w else None, eps, g)
            got = lr.opt_ref(x, lab, nc, w if has_w else None, eps, g)
            for k in ("lse", "row", "S_row", "wy", "dl", "S_dl"):
                same(got[k], want[k])


KINDS = [("plain", None, False), ("opt", 0.0, True), ("opt", 0.1, False), ("opt", 0.1, True), ("focal", 0.0, True), ("focal", 2.0, False),
         ("focal", 3.5, True)]


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
def test_a_non_finite_row_touches_only_its_own_outputs(case):
    """Three calls per kind: the poisoned rows (six with a valid label, six ignored, all in workgroup 0), the base rows, and
    the ignored set alone poisoned.  Every clean row's lse, row_loss and dlogits and the partial pair of workgroup 1 have
    the base call's bits; with only ignored rows poisoned every partial pair has, and those rows' row_loss is exactly 0.
    lse of a poisoned row is non-finite exactly where fp64 logsumexp is; the row with -inf at its label has a finite lse and
    row_loss +inf; with a valid row poisoned the loss sum of workgroup 0 is non-finite; the pad of dlogits is exact zeros
    throughout.  The gradient inside a poisoned row is not specified."""
    rows, nc, ld = case
    buf, lab, base, poisoned = lr.regime_inputs("nonfinite", rows, nc, ld, seed=701)
    only = lr.regime_inputs("nonfinite", rows, nc, ld, seed=701, poison=("ignored",))[0]
    hit = torch.cat([poisoned["valid"], poisoned["ignored"]])
    clean = torch.ones(rows, dtype=torch.bool)
    clean[hit] = False
    clean = clean.to(DEV)
    ref_lse = torch.logsumexp(buf[:, :nc].double(), 1)
    lab_d, w_all = lab.to(DEV), lr.weights(nc, seed=703).to(DEV)
    scale, row_grad = torch.tensor([0.01], device=DEV), _row_grad(rows)
    for kind, param, has_w in KINDS:
        w = w_all if has_w else None
        outs = {name: _run(kind, param, b.to(DEV), lab_d, w, nc, ld, scale, row_grad)
                for name, b in (("poisoned", buf), ("base", base), ("ignored", only))}
        tag = f"{kind} {param} {'w' if has_w else ''}"
        (lse_p, row_p, part_p, dls_p, dlr_p), (lse_b, row_b, part_b, dls_b, dlr_b) = outs["poisoned"], outs["base"]
        for got, want, what in ((lse_p, lse_b, "lse"), (row_p, row_b, "row_loss"), (dls_p, dls_b, "dlogits"), (dlr_p, dlr_b, "dlogits (rows)")):
            if got is not None:
                assert torch.isfinite(want[1][:, :nc] if want[1].dim() == 2 else want[1]).all()
                assert torch.equal(got[1][clean], want[1][clean]), f"{tag}: {what} of a clean row moved"
        assert torch.equal(part_p[1][1], part_b[1][1]), f"{tag}: the partial pair of workgroup 1 moved"
        assert bool((part_b[1][2:] == 0).all()) and torch.isfinite(part_b[1]).all()
        assert not bool(torch.isfinite(part_p[1][0, 0])), f"{tag}: a poisoned labelled row did not reach the loss sum"
        assert torch.equal(part_p[1][0, 1], part_b[1][0, 1]), f"{tag}: the denominator moved"
        assert torch.equal(torch.isfinite(lse_p[1]).cpu(), torch.isfinite(ref_lse)), f"{tag}: lse is non-finite elsewhere than fp64 logsumexp"
        at_label = int(poisoned["valid"][lr.NONFINITE_KINDS.index("neg_inf_label")])
        assert bool(torch.isfinite(lse_p[1][at_label]))
        if row_p is not None:
            assert float(row_p[1][at_label]) == float("inf"), f"{tag}: -inf at the label: row_loss {float(row_p[1][at_label])}"
            assert bool((row_p[1][poisoned["ignored"].to(DEV)] == 0).all())
        lse_i, row_i, part_i, dls_i, dlr_i = outs["ignored"]
        assert torch.equal(part_i[1], part_b[1]), f"{tag}: an ignored non-finite row moved a partial pair"
        if row_i is not None:
            assert bool((row_i[1][poisoned["ignored"].to(DEV)] == 0).all())
            assert torch.equal(row_i[1], row_b[1])
        for gdl in (dls_p, dlr_p, dls_i, dlr_i):
            if gdl is not None:
                assert bool((gdl[1][:, nc:] == 0).all()), f"{tag}: pad columns of dlogits are not exact zeros"


# ---------------------------------------------------------------------------------------------------------------------
# front ends

def _padded_view(x_cpu, ld):
    rows, nc = x_cpu.shape
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = x_cpu
    buf = buf.to(DEV).view(1, 1, rows, ld).requires_grad_()
    return buf, buf[..., :nc].permute(0, 3, 1, 2)


FRONT_CASES = [(300, 9, 12), (300, 68, 68)]
FRONTS = ["plain", "weighted", "focal"]


def _front(front, view, label, w):
    from sigma_amd.pointwise import cross_entropy, focal_cross_entropy
    if front == "focal":
        return focal_cross_entropy(view, label, IGNORE, 2.0)
    crit = nn.CrossEntropyLoss(weight=w if front == "weighted" else None, ignore_index=IGNORE)
    return cross_entropy(crit, view, label)


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("case", FRONT_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in FRONT_CASES])
@pytest.mark.parametrize("regime", ["confident", "offset", "masked"])
def test_front_end_mean_against_the_twin(regime, case, front):
    """pointwise.cross_entropy (plain and weighted criterion) and focal_cross_entropy (gamma 2) with 'mean' on the padded
    view: loss and gradient under the bounds of the module docstring"""
    rows, nc, ld = case
    fam = _family(nc, regime) + " front end"
    buf_c, lab_c = lr.regime_inputs(regime, rows, nc, ld, seed=721)
    x = buf_c[:, :nc].double().to(DEV)
    lab = lab_c.to(DEV)
    w = lr.weights(nc, seed=703).to(DEV) if front == "weighted" else None
    kind, param = {"plain": ("plain", None), "weighted": ("opt", 0.0), "focal": ("focal", 2.0)}[front]
    buf, view = _padded_view(buf_c[:, :nc], ld)
    loss = _front(front, view, lab.view(1, 1, rows), w)
    assert loss is not None
    (loss * 1.7).backward()
    r0, _, K_dl, K_in_sum = _reference(kind, param, x, lab, nc, w, 0.0)
    den = float(r0["wy"].sum())
    K_den = 0 if kind == "plain" else _k_sum(rows) + 1
    K_loss = (_k_sum(rows) + K_in_sum + 1) + K_den + 1
    a = check(fam, loss.detach().double().view(1), (r0["row"].sum() / den).view(1), r0["S_row"].sum().view(1) / den, K_loss, "loss")
    r = _reference(kind, param, x, lab, nc, w, 1.7 / den)[0]
    S = r["S_dl"] + (lr.underflow_S(r["f"], K_dl) if kind != "focal" and regime in lr.SUBNORMAL_REGIMES else 0.0)
    g = buf.grad.view(-1, ld)
    b = check(fam, g[:, :nc], r["dl"], S, K_dl + K_den + 2, "gradient")
    assert bool((g[:, nc:] == 0).all()) and bool((g[:, :nc][torch.isinf(x)] == 0).all())
    _show(f"{regime} {case} {front}", {"loss": a, "gradient": b})


@pytest.mark.parametrize("front", FRONTS)
@pytest.mark.parametrize("case", FRONT_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in FRONT_CASES])
def test_front_end_loss_is_nan_iff_a_labelled_row_is_poisoned(case, front):
    """cross_entropy (plain and weighted): NaN with a labelled row poisoned; the bits of the base call with only ignored
    rows poisoned.  focal_cross_entropy: +inf, not NaN -- focal_row clamps d = fminf(x_y - lse, 0), and fminf drops a NaN
    operand, so a labelled row whose lse is NaN adds a loss of 0; what makes the sum non-finite is the row with -inf at its
    label (loss +inf).  Asserted as it is: non-finite."""
    rows, nc, ld = case
    buf_c, lab_c, base_c, _ = lr.regime_inputs("nonfinite", rows, nc, ld, seed=721)
    only_c = lr.regime_inputs("nonfinite", rows, nc, ld, seed=721, poison=("ignored",))[0]
    lab = lab_c.to(DEV).view(1, 1, rows)
    w = lr.weights(nc, seed=703).to(DEV) if front == "weighted" else None
    losses = {}
    for name, b in (("poisoned", buf_c), ("base", base_c), ("ignored", only_c)):
        buf, view = _padded_view(b[:, :nc], ld)
        loss = _front(front, view, lab, w)
        assert loss is not None
        loss.backward()
        assert bool((buf.grad.view(-1, ld)[:, nc:] == 0).all())
        losses[name] = loss.detach()
    assert bool(torch.isfinite(losses["base"]))
    if front == "focal":
        assert float(losses["poisoned"]) == float("inf")
    else:
        assert bool(torch.isnan(losses["poisoned"]))
    assert torch.equal(losses["ignored"], losses["base"])


# ---------------------------------------------------------------------------------------------------------------------
# OHEM, threshold branch

@pytest.mark.parametrize("regime", lr.OHEM_REGIMES)
@pytest.mark.parametrize("case", lr.OHEM_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in lr.OHEM_CASES])
def test_ohem_threshold_branch_on_the_regime(case, regime):
    """ProbOhemCrossEntropy2d on the padded view, thresh 0.7 governing (tests/test_loss_regimes_cpu.py holds the seeds to the
    gap condition: zero valid rows within delta_r of tau): the mined set and the counts are the twin's exactly, loss and
    gradient lie under the bounds of tests/test_ohem_gpu.py"""
    from sigma_amd.pointwise import OhemCEFn, ohem_stages
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    rows, nc, ld = case
    fam = _family(nc, regime) + " ohem"
    buf_c, lab_c = lr.regime_inputs(regime, rows, nc, ld, lr.OHEM_SEEDS[(regime, case)])
    x_c = buf_c[:, :nc].contiguous()
    x64, lab = x_c.double().to(DEV), lab_c.to(DEV)
    thresh, min_kept = lr.OHEM_THRESH, lr.OHEM_MIN_KEPT
    K_den = _k_sum(rows) + 1
    for has_w in (False, True):
        w = lr.weights(nc, seed=703).to(DEV) if has_w else None
        t = ohem_twin(x_c, lab_c, IGNORE, thresh, min_kept, weight=w.cpu() if has_w else None)
        assert t["mining"] and t["tau_row"] < 0 and lr.ohem_gap_violations(t, nc) == 0
        buf, view = _padded_view(x_c, ld)
        st = ohem_stages(view.detach().permute(0, 2, 3, 1).reshape(-1, nc), lab, w, IGNORE, ld, thresh, min_kept)
        torch.cuda.synchronize()
        assert torch.equal(st["mined"].cpu(), t["mined"]), "kept set differs from the twin's"
        assert tuple(int(v) for v in st["counts"].cpu()) == (int(t["valid"].sum()), int(t["keep"].sum()))
        crit = ProbOhemCrossEntropy2d(IGNORE, "mean", thresh, min_kept, weight=w)
        loss = crit(view, lab.view(1, 1, rows))
        assert type(loss.grad_fn).__name__.startswith(OhemCEFn.__name__)
        (loss * 1.7).backward()
        mined = t["mined"].to(DEV)
        r0 = lr.opt_ref(x64, mined, nc, w, 0.0, 0.0)
        den = float(r0["wy"].sum())
        K_loss = (_k_sum(rows) + 2 * nc + 16 + 1) + K_den + 1
        a = check(fam, loss.detach().double().view(1), (r0["row"].sum() / den).view(1), r0["S_row"].sum().view(1) / den, K_loss, "loss")
        r = lr.opt_ref(x64, mined, nc, w, 0.0, 1.7 / den)
        K_dl = 2 * nc + 24
        S = r["S_dl"] + (lr.underflow_S(r["f"], K_dl) if regime in lr.SUBNORMAL_REGIMES else 0.0)
        g = buf.grad.view(-1, ld)
        b = check(fam, g[:, :nc], r["dl"], S, K_dl + K_den + 2, "gradient")
        assert bool((g[:, nc:] == 0).all()) and bool((g[~t["keep"].to(DEV)] == 0).all())
        _show(f"{regime} {case} ohem {'w' if has_w else ''}", {"loss": a, "gradient": b})


# ---------------------------------------------------------------------------------------------------------------------
# deep supervision: the fused upsample + cross-entropy kernels (130 classes: the entry point ends at 64)

@pytest.mark.parametrize("regime", lr.DEEPSUP_REGIMES)
@pytest.mark.parametrize("case", lr.DEEPSUP_CASES, ids=["%dx%dx%d_x%d_%d@%d" % c for c in lr.DEEPSUP_CASES])
def test_upsample_ce_kernels_on_the_regime(case, regime):
    from tests.test_deepsup_gpu import _kernels
    B, h, w, s, nc, ld = case
    buf, lab = lr.deepsup_regime_inputs(case, regime, seed=711)
    g = 1.0 / 37.0
    b = db.bounds(buf[..., :nc].double(), lab, s, g=float(torch.tensor(g, dtype=torch.float32)))
    lse, partial, dl = _kernels(buf, lab, s, nc, g)
    assert torch.isfinite(lse).all() and torch.isfinite(partial).all() and torch.isfinite(dl).all()
    e_lse = (lse.cpu().double() - b["lse"]).abs()
    e_p0 = (partial[:, 0].cpu().double() - b["partial"][:, 0]).abs()
    e_dl = (dl[..., :nc].cpu().double() - b["dl"]).abs()
    ratios = {"lse": float((e_lse / b["E_lse"]).max()), "partial": float((e_p0 / b["E_partial"].clamp_min(1e-300)).max()),
              "dlogits": float((e_dl / b["E_dl"]).max())}
    fam = f"{PREFIX} upsample+ce {regime}"
    WORST[fam] = max(WORST.get(fam, 0.0), *ratios.values())
    _show(f"{regime} {case} upsample+ce", ratios)
    assert bool((e_lse <= b["E_lse"]).all())
    assert bool((e_p0 <= b["E_partial"]).all())
    assert torch.equal(partial[:, 1].cpu().double(), b["partial"][:, 1])
    assert bool((e_dl <= b["E_dl"]).all())
    assert bool((dl[..., nc:] == 0).all())


def test_upsample_ce_declines_130_classes():
    """the fused entry point ends at 64 classes: (1, 3, 3, 4, 130, 132) is refused by the front end, not run"""
    from sigma_amd.pointwise import upsampled_cross_entropy
    buf, _ = lr.regime_inputs("sweep", 9, 130, 132, seed=711)
    lab = torch.zeros(1, 12, 12, dtype=torch.long, device=DEV)
    crit = nn.CrossEntropyLoss(ignore_index=IGNORE)
    assert upsampled_cross_entropy(crit, buf.view(1, 3, 3, 132).to(DEV)[..., :130], 4, lab) is None


def test_zz_report_worst_ratios():
    print("\nworst error / bound seen, per kernel form and regime:")
    for fam in sorted(k for k in WORST if k.startswith(PREFIX)):
        print(f"  {fam:50s} {WORST[fam]:.3f}")
