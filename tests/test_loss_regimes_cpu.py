"""The loss family's value regimes without a GPU (tests/loss_regimes.py): the fp32 emulation of every kernel kind in both
forms -- the row maximum first, and the walk with the online rescale as the fixed kernel does it -- under the bounds that
tests/test_loss_regimes_gpu.py applies to the kernels, on the same inputs; the three wrong variants rejected on the regimes
named for them; the fp64 twins finite on every regime but ``nonfinite``; the deep-supervision emulation under its bounds
on the regimes' coarse logits; and the OHEM seeds' gap condition."""
import pytest
import torch

from tests import deepsup_bounds as db
from tests import focal_bounds as fb
from tests import loss_regimes as lr
from tests.ohem_fp64_twin import twin as ohem_twin
from tests.test_stream_fp64_gpu import WORST, check, rejects

FORMS = ("reg", "walk")


def _family(form, regime):
    return f"loss regimes (fp32 emulation) {form} {regime}"


def _inputs(regime, case, seed=701):
    rows, nc, ld = case
    buf, lab = lr.regime_inputs(regime, rows, nc, ld, seed)[:2]
    return buf[:, :nc].contiguous(), lab


def _grads(rows, den):
    return 0.7 / den, torch.randn(rows, generator=torch.Generator().manual_seed(704))


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
@pytest.mark.parametrize("regime", lr.FINITE_REGIMES)
def test_emulation_stays_under_the_bounds(regime, case):
    """every kind (plain; option with weights, smoothing and both -- ``masked`` without smoothing; focal at four exponents
    with and without weights) in both forms, device-scalar and per-row gradient: lse, row_loss and dlogits under the
    bounds; on ``offset`` lse under the sharper bound as well; on ``masked`` everything finite and the gradient exactly
    zero at masked columns"""
    rows, nc, ld = case
    x32, lab = _inputs(regime, case)
    x64 = x32.double()
    masked = torch.isinf(x32)
    sub = regime in lr.SUBNORMAL_REGIMES
    w = lr.weights(nc, seed=703)
    valid = lr.is_valid(lab, nc)
    assert 0 < int(valid.sum()) < rows
    for form in FORMS:
        fam = _family(form, regime)
        sc, row_grad = _grads(rows, float(valid.sum()))
        r = lr.plain_ref(x64, lab, nc, sc)
        e = lr.emulate_ce_fp32(x32, lab, nc, None, 0.0, sc, form, kind="plain")
        check(fam, e["lse"], r["lse"], r["S_lse"], nc + 8, "lse")
        if regime == "offset":
            check(fam + " sharp", e["lse"], r["lse"], lr.lse_offset_bound(r["lse"], nc) / lr.U, 1, "lse (sharper bound)")
        S = r["S_dl"] + (lr.underflow_S(r["f"], nc + 16) if sub else 0.0)
        check(fam, e["dl"], r["dl"], S, nc + 16, "plain dlogits")
        assert bool((e["dl"][masked] == 0).all()) and bool((e["dl"][~valid] == 0).all())
        for has_w, eps in lr.OPTS:
            if regime == "masked" and eps > 0:
                continue
            wo = w if has_w else None
            den = float(lr.opt_ref(x64, lab, nc, wo, eps, 0.0)["wy"].sum())
            for g in _grads(rows, den):
                r = lr.opt_ref(x64, lab, nc, wo, eps, g)
                e = lr.emulate_ce_fp32(x32, lab, nc, wo, eps, g, form)
                check(fam, e["lse"], r["lse"], r["S_lse"], nc + 8, "lse")
                check(fam, e["row"], r["row"], r["S_row"], 2 * nc + 16, "option row_loss")
                S = r["S_dl"] + (lr.underflow_S(r["f"], 2 * nc + 24) if sub else 0.0)
                check(fam, e["dl"], r["dl"], S, 2 * nc + 24, "option dlogits")
                assert bool((e["dl"][masked] == 0).all()) and bool((e["dl"][~valid] == 0).all())
        for gamma in lr.GAMMAS:
            for wo in (None, w):
                den = float(lr.focal_ref(x64, lab, nc, wo, gamma, 0.0)["wy"].sum())
                for g in _grads(rows, den):
                    r = lr.focal_ref(x64, lab, nc, wo, gamma, g)
                    e = fb.emulate_fp32(x32, lab, nc, wo, gamma, g, form=form)
                    check(fam, e["lse"], r["lse"], r["S_lse"], r["K_lse"], "focal lse")
                    check(fam, e["row"], r["row"], r["S_row"], r["K"], "focal row_loss")
                    check(fam, e["dl"], r["dl"], r["S_dl"], r["K"], "focal dlogits")
                    assert bool((e["dl"][masked] == 0).all()) and bool((e["dl"][~valid] == 0).all())


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
def test_no_max_is_rejected_on_offset(case):
    rows, nc, ld = case
    x32, lab = _inputs("offset", case)
    r = lr.plain_ref(x32.double(), lab, nc, 1.0)
    for form in FORMS:
        wrong = lr.lse_fp32(x32, form, "no_max")
        assert not bool(torch.isfinite(wrong).all())                  # exp(1e2) overflows, exp(-1e2) sums to 0
        bad = ~torch.isfinite(wrong)
        rejects(torch.where(bad, torch.full_like(wrong, 3e38), wrong), r["lse"], r["S_lse"], nc + 8, "exp without the max")


@pytest.mark.parametrize("regime", ["ascending", "sweep"])
@pytest.mark.parametrize("case", [c for c in lr.CASES if c[1] > 4], ids=[i for c, i in zip(lr.CASES, lr.CASE_IDS) if c[1] > 4])
def test_no_rescale_is_rejected_where_the_maximum_rises(regime, case):
    """more than one chunk: the walk without s *= exp(m - vm) keeps sums taken against an earlier, smaller maximum"""
    rows, nc, ld = case
    x32, lab = _inputs(regime, case)
    r = lr.plain_ref(x32.double(), lab, nc, 1.0)
    wrong = lr.lse_fp32(x32, "walk", "no_rescale")
    bad = ~torch.isfinite(wrong)
    rejects(torch.where(bad, torch.full_like(wrong, 3e38), wrong), r["lse"], r["S_lse"], nc + 8, "walk without the rescale")
    check(_family("walk", regime), lr.lse_fp32(x32, "walk"), r["lse"], r["S_lse"], nc + 8, "the walk itself")


@pytest.mark.parametrize("case", [c for c in lr.CASES if c[1] >= 5], ids=[i for c, i in zip(lr.CASES, lr.CASE_IDS) if c[1] >= 5])
def test_the_walk_before_the_fix_gives_nan_on_a_masked_first_chunk(case):
    """exp(-inf - (-inf)): NaN in exactly the rows whose first chunk is masked whole (kind (a), and rows of (c) and (d) that
    happen to be), where fp64 logsumexp and the fixed walk are finite"""
    rows, nc, ld = case
    x32, lab = _inputs("masked", case)
    first = torch.isinf(x32[:, :4]).all(1)
    assert int(first.sum()) >= rows // 8
    old = lr.lse_fp32(x32, "walk", "first_chunk")
    assert torch.equal(torch.isnan(old), first)
    ref = torch.logsumexp(x32.double(), 1)
    assert bool(torch.isfinite(ref).all())
    new = lr.lse_fp32(x32, "walk")
    check(_family("walk", "masked"), new, ref, ref.abs() + 1.0, nc + 8, "the fixed walk")
    assert torch.equal(old[~first], new[~first])                      # the same bits wherever the old walk had an answer


def test_the_fixed_walk_keeps_the_bits_on_finite_rows():
    """the guard reads m alone: on every finite regime the fixed walk and the walk before it agree bit for bit"""
    for regime in lr.FINITE_REGIMES[:-1]:
        for case in lr.CASES:
            x32, _ = _inputs(regime, case)
            assert torch.equal(lr.lse_fp32(x32, "walk"), lr.lse_fp32(x32, "walk", "first_chunk")), (regime, case)


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
def test_twins_are_finite_on_every_finite_regime(case):
    rows, nc, ld = case
    w = lr.weights(nc, seed=703)
    for regime in lr.FINITE_REGIMES:
        x32, lab = _inputs(regime, case)
        x64 = x32.double()
        outs = [lr.plain_ref(x64, lab, nc, 0.01), lr.opt_ref(x64, lab, nc, w, 0.0, 0.01), lr.focal_ref(x64, lab, nc, w, 3.5, 0.01),
                ohem_twin(x64, lab, lr.IGNORE, lr.OHEM_THRESH, lr.OHEM_MIN_KEPT, weight=w)]
        if regime != "masked":
            outs.append(lr.opt_ref(x64, lab, nc, w, 0.1, 0.01))
        for t in outs:
            for k in ("lse", "row", "dl", "S_row", "S_dl", "loss"):
                if k in t and torch.is_tensor(t[k]):
                    assert bool(torch.isfinite(t[k]).all()), (regime, k)


def test_nonfinite_inputs_are_what_the_docstring_says():
    for rows, nc, ld in lr.CASES:
        buf, lab, base, poisoned = lr.regime_inputs("nonfinite", rows, nc, ld, seed=701)
        hit = torch.cat([poisoned["valid"], poisoned["ignored"]])
        assert hit.numel() == 12 and int(hit.max()) < 256
        clean = torch.ones(rows, dtype=torch.bool)
        clean[hit] = False
        assert torch.equal(buf[clean][:, :nc], base[clean][:, :nc]) and bool(torch.isfinite(base[:, :nc]).all())
        assert bool(lr.is_valid(lab[poisoned["valid"]], nc).all()) and bool((lab[poisoned["ignored"]] == lr.IGNORE).all())
        assert not bool(torch.isfinite(buf[hit][:, :nc]).all(1).any())
        ref = torch.logsumexp(buf[:, :nc].double(), 1)
        last = poisoned["valid"][5]                                    # -inf at the label: lse finite, the loss +inf
        assert bool(torch.isfinite(ref[last])) and float(ref[last] - buf[last, lab[last]].double()) == float("inf")
        only, lab2, _, p2 = lr.regime_inputs("nonfinite", rows, nc, ld, seed=701, poison=("ignored",))
        assert torch.equal(lab2, lab) and p2["valid"].numel() == 0 and torch.equal(only[poisoned["valid"]][:, :nc], base[poisoned["valid"]][:, :nc])
        for form in FORMS:                                             # non-finite exactly where fp64 logsumexp is
            assert torch.equal(torch.isfinite(lr.lse_fp32(buf[:, :nc].contiguous(), form)), torch.isfinite(ref)), (nc, form)


@pytest.mark.parametrize("regime", lr.DEEPSUP_REGIMES)
@pytest.mark.parametrize("case", lr.DEEPSUP_CASES, ids=["%dx%dx%d_x%d_%d@%d" % c for c in lr.DEEPSUP_CASES])
def test_deepsup_emulation_stays_under_its_bounds(case, regime):
    B, h, w, s, nc, ld = case
    buf, lab = lr.deepsup_regime_inputs(case, regime, seed=711)
    g = 1.0 / 37.0
    b = db.bounds(buf[..., :nc].double(), lab, s, g=g)
    for k in ("lse", "row", "dl"):
        assert bool(torch.isfinite(b[k]).all())
    e = db.emulate_fp32(buf, lab, s, nc, g)
    assert bool(((e["lse"].double() - b["lse"]).abs() <= b["E_lse"]).all())
    assert bool(((e["row"].double() - b["row"]).abs() <= b["E_row"]).all())
    assert bool(((e["partial"][:, 0].double() - b["partial"][:, 0]).abs() <= b["E_partial"]).all())
    assert torch.equal(e["partial"][:, 1].double(), b["partial"][:, 1])
    assert bool(((e["dl"][..., :nc].double() - b["dl"]).abs() <= b["E_dl"]).all())


@pytest.mark.parametrize("regime", lr.OHEM_REGIMES)
@pytest.mark.parametrize("case", lr.OHEM_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in lr.OHEM_CASES])
def test_ohem_seeds_keep_every_valid_row_away_from_tau(case, regime):
    """the threshold branch governs (the min_kept-th smallest p is below thresh), more rows are kept than min_kept, tau does
    not fall into the cluster of rows with p_y = 1, and no valid row lies within delta_r of tau"""
    rows, nc, ld = case
    x32, lab = _inputs(regime, case, seed=lr.OHEM_SEEDS[(regime, case)])
    for w in (None, lr.weights(nc, seed=703)):
        t = ohem_twin(x32, lab, lr.IGNORE, lr.OHEM_THRESH, lr.OHEM_MIN_KEPT, weight=w)
        assert t["mining"] and t["threshold"] == lr.OHEM_THRESH and t["tau_row"] < 0
        assert lr.OHEM_MIN_KEPT < int(t["keep"].sum()) < int(t["valid"].sum())
        assert lr.ohem_gap_violations(t, nc) == 0


def test_zz_report_worst_ratios():
    print("\nworst error / bound of the fp32 emulation, per form and regime:")
    for fam in sorted(k for k in WORST if k.startswith("loss regimes (fp32 emulation)")):
        print(f"  {fam:60s} {WORST[fam]:.3f}")
