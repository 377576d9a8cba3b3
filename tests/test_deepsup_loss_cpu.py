"""The fused upsample + loss route for the criteria with options, without a GPU: the fp64 twin against torch's own criteria,
the fp32 emulation of the kernels inside the bounds the GPU test uses (tests/deepsup_loss_bounds.py) on every case and kind,
the wrong variants of the twin outside them, the conditions on the committed OHEM inputs, the C ABI's argument checks
(no launch is reached) and what the front end declines."""
import ctypes

import pytest
import torch
import torch.nn as nn

from sigma_amd import _capi
from tests.capi_refusals import assert_refused
from tests.deepsup_fp64_twin import upsample
from tests.deepsup_loss_bounds import (CASE_IDS, CASES, G1_CASE, G1_KIND, IGNORE, KIND_IDS, KINDS, OHEM_IDS, OHEM_PAIRS, bounds,
                                       class_weights, deepsup_inputs, emulate_fp32, ohem_gap, upstream_of)
from tests.deepsup_loss_twin import VARIANTS, adjoint, twin
from tests.deepsup_loss_twin import upsample as upsample_by_axis

OHEM_SPEC = dict(kind="ohem", weighted=True, eps=0.0, gamma=0.0, reduction="mean")


def _ratios(e, b, nc, spec):
    """the emulation's (or any candidate's) errors as fractions of the bounds"""
    r = {"lse": float(((e["lse"].double() - b["lse"]).abs() / b["E_lse"]).max()),
         "row": float(((e["row"].double() - b["row"]).abs() / b["E_row"].clamp_min(1e-300)).max()),
         "partial0": float(((e["partial"][:, 0].double() - b["partial"][:, 0]).abs() / b["E_partial"][:, 0].clamp_min(1e-300)).max()),
         "partial1": float(((e["partial"][:, 1].double() - b["partial"][:, 1]).abs() / b["E_partial"][:, 1].clamp_min(1e-300)).max()),
         "dl": float(((e["dl"][..., :nc].double() - b["dl"]).abs() / b["E_front"]).max())}
    if spec["reduction"] != "none":
        r["loss"] = abs(float(e["loss"]) - float(b["loss"])) / b["E_loss"]
    return r


def _run(case, spec, variant=None, seed=0, **kw):
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case, seed)
    w = class_weights(nc, spec["weighted"])
    up = upstream_of(spec, lab)
    b = bounds(buf[..., :nc].double(), lab, s, spec, w, up, variant=variant, **kw)
    e = emulate_fp32(buf, lab, s, nc, spec, w, up, **kw)
    return e, b, _ratios(e, b, nc, spec)


def test_twin_is_torchs_criterion_on_the_upsampled_logits():
    """options: nn.CrossEntropyLoss with its own reduction, forward and gradient; ohem: the criterion on the mined labels"""
    case = (2, 5, 4, 4, 37, 40)
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    x64 = buf[..., :nc].double()
    ok = torch.where((lab >= 0) & (lab < nc), lab, torch.full_like(lab, IGNORE))
    w = class_weights(nc)
    for red, eps in (("mean", 0.0), ("mean", 0.1), ("sum", 0.1)):
        t = twin(x64, lab, s, IGNORE, "options", weight=w, eps=eps, reduction=red)
        xr = x64.clone().requires_grad_(True)
        ref = nn.CrossEntropyLoss(weight=w.double(), ignore_index=IGNORE, reduction=red, label_smoothing=eps)(
            upsample(xr, s).permute(0, 3, 1, 2), ok)
        ref.backward()
        assert abs(float(t["loss"]) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
        assert float((t["dl"] - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max())
    t = twin(x64, lab, s, IGNORE, "ohem", weight=w, thresh=0.05, min_kept=16)
    xr = x64.clone().requires_grad_(True)
    ref = nn.CrossEntropyLoss(weight=w.double(), ignore_index=IGNORE)(upsample(xr, s).permute(0, 3, 1, 2), t["mined"])
    ref.backward()
    assert abs(float(t["loss"]) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    assert float((t["dl"] - xr.grad).abs().max()) <= 1e-12 * float(xr.grad.abs().max())
    assert 0 < t["counts"][1] < t["counts"][0]


@pytest.mark.parametrize("case", CASES[:8], ids=CASE_IDS[:8])
def test_twin_interpolates_as_the_deep_supervision_twin(case):
    from tests import deepsup_fp64_twin
    B, h, wd, s, nc, ld = case
    z = torch.randn(B, h, wd, nc, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    up = deepsup_fp64_twin.upsample(z, s)
    assert float((upsample_by_axis(z, s) - up).abs().max()) <= 1e-12
    assert float((adjoint(up, h, wd, s) - deepsup_fp64_twin.adjoint(up, h, wd, s)).abs().max()) <= 1e-12 * (2 * s) ** 2


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emulation_stays_inside_the_bounds(case, kind):
    e, b, r = _run(case, KINDS[kind])
    print({k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    assert bool((e["dl"][..., case[4]:] == 0).all())
    if not KINDS[kind]["weighted"]:
        assert torch.equal(e["partial"][:, 1].double(), b["partial"][:, 1])      # whole numbers: exact


def test_emulation_stays_inside_the_bounds_with_one_lane_per_item():
    e, b, r = _run(G1_CASE, KINDS[G1_KIND])
    print({k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("pair", OHEM_PAIRS, ids=OHEM_IDS)
def test_ohem_inputs_meet_their_conditions_and_the_emulation_the_bounds(pair):
    """no valid pixel within 2 E_row of tau; the named rule decides; in the mining pairs 0 < kept < num_valid.  Then the
    emulation keeps the twin's set and stays inside the bounds."""
    case, seed, thresh, min_kept, what = pair
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case, seed)
    t, near = ohem_gap(buf[..., :nc].double(), lab, s, thresh, min_kept)
    sel, (num_valid, kept) = t["sel"], t["counts"]
    assert near == 0
    if what == "all":
        assert min_kept > num_valid and not sel["mining"] and kept == num_valid
        assert bool((sel["valid"] & (sel["p"] > thresh)).any())        # thresh, wrongly applied, would drop pixels
    else:
        assert sel["mining"] and 0 < kept < num_valid
        assert (sel["tau_row"] >= 0) == (what == "kth")
    e, b, r = _run(case, OHEM_SPEC, seed=seed, thresh=thresh, min_kept=min_kept)
    assert torch.equal(e["keep"], b["keep"]) and e["counts"] == b["counts"]
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("variant,kind,kw", [
    ("wy_wrong_class", "w", {}), ("wy_wrong_class", "focal2w", {}), ("smooth_no_W", "w+eps", {}),
    ("focal_m_one_term", "focal2w", {}), ("focal_m_one_term", "focal3.5", {}), ("mean_pixels", "w", {}),
    ("mean_pixels", "focal1w", {}), ("ohem_thresh_always", "ohem", dict(thresh=0.7, min_kept=100000))])
def test_wrong_variants_leave_the_bounds(variant, kind, kw):
    assert variant in VARIANTS
    case = (2, 2, 3, 16, 40, 40) if kind == "ohem" else (2, 5, 4, 4, 37, 40)
    e, b, r = _run(case, OHEM_SPEC if kind == "ohem" else KINDS[kind], variant=variant, **kw)
    print(variant, kind, {k: round(v, 2) for k, v in r.items()})
    assert max(r["dl"], r.get("loss", 0.0)) > 1.0, r


def test_every_variant_is_exercised():
    used = {row[0] for mark in test_wrong_variants_leave_the_bounds.pytestmark for row in mark.args[1]}
    assert used == set(VARIANTS)


def _params(**kw):
    """a sigma_upsample_loss_params that passes every check (the pointers are aligned numbers, never dereferenced: each call
    below is refused before any launch)"""
    p = _capi.UpsampleLossParams()
    p.batch, p.height, p.width, p.scale, p.classes, p.ld, p.ignore_index = 2, 3, 4, 8, 9, 12, 255
    p.kind, p.label_smoothing, p.gamma = _capi.SIGMA_UPSAMPLE_LOSS_OPTIONS, 0.0, 0.0
    for i, name in enumerate(("logits", "labels", "lse", "partial", "dlogits", "scale_grad")):
        setattr(p, name, 0x10000 + 0x1000 * i)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


FOCAL = dict(kind=_capi.SIGMA_UPSAMPLE_LOSS_FOCAL, coef=0x20000)
REFUSED_BOTH = [dict(classes=0), dict(classes=65, ld=68), dict(ld=10), dict(ld=8), dict(scale=0), dict(scale=33), dict(batch=0),
                dict(height=0), dict(width=-1), dict(batch=2 ** 20, height=2 ** 10, width=2 ** 10, scale=2),      # 2^31 fine pixels
                dict(logits=None), dict(labels=None), dict(lse=None), dict(logits=0x10008), dict(labels=0x11004), dict(lse=0x12002),
                dict(weight=0x30001), dict(kind=2), dict(kind=-1), dict(label_smoothing=-0.1), dict(label_smoothing=1.5),
                dict(label_smoothing=float("nan")), dict(FOCAL, label_smoothing=0.1), dict(FOCAL, gamma=0.5),
                dict(FOCAL, gamma=-1.0), dict(FOCAL, gamma=float("nan")), dict(FOCAL, gamma=float("inf")),
                dict(FOCAL, coef=None), dict(FOCAL, coef=0x20002)]
REFUSED_FWD = [dict(partial=None), dict(partial=0x13002), dict(row_loss=0x40002)]
REFUSED_BWD = [dict(scale_grad=None), dict(row_grad=0x50000), dict(dlogits=None), dict(dlogits=0x14008),
               dict(scale_grad=0x15002), dict(scale_grad=None, row_grad=0x50002)]


def test_host_validation_without_gpu():
    """every refusal of include/sigma_ops.h returns SIGMA_OPS_ERR_ARG before any launch"""
    lib = _capi.load()
    assert_refused(lib.sigma_upsample_loss_fwd, None, None, says="NULL")
    assert_refused(lib.sigma_upsample_loss_bwd, None, None, says="NULL")
    for kw in REFUSED_BOTH:
        p = _params(**kw)
        assert_refused(lib.sigma_upsample_loss_fwd, ctypes.byref(p), None, msg=kw)
        assert_refused(lib.sigma_upsample_loss_bwd, ctypes.byref(p), None, msg=kw)
    for kw in REFUSED_FWD:
        assert_refused(lib.sigma_upsample_loss_fwd, ctypes.byref(_params(**kw)), None, msg=kw)
    for kw in REFUSED_BWD:
        assert_refused(lib.sigma_upsample_loss_bwd, ctypes.byref(_params(**kw)), None, msg=kw)


def test_front_end_declines_without_a_gpu_and_by_criterion(monkeypatch):
    """CPU tensors have no route.  With the shape checks and the Function replaced (so that the criterion and weight checks
    alone decide, on CPU tensors), the criteria of the issue are taken and the others declined."""
    import sigma_amd.pointwise as pw
    from sigma_amd.utils.loss_opr import FocalLoss2d, ProbOhemCrossEntropy2d
    nc, s = 9, 4
    x = torch.randn(1, 2, 3, nc)
    lab = torch.zeros(1, 8, 12, dtype=torch.long)
    w = torch.rand(nc) + 0.5
    taken = [nn.CrossEntropyLoss(weight=w, ignore_index=255), nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(reduction="sum"),
             nn.CrossEntropyLoss(reduction="none", weight=w), FocalLoss2d(weight=w), FocalLoss2d(exponent=0.0), FocalLoss2d(exponent=3.5),
             ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=10, weight=w), ProbOhemCrossEntropy2d(255)]
    declined = [nn.CrossEntropyLoss(ignore_index=255),                                  # the plain criterion: upsampled_cross_entropy's
                nn.CrossEntropyLoss(weight=w.double()), nn.CrossEntropyLoss(weight=torch.rand(nc + 1)),
                nn.CrossEntropyLoss(weight=w.to("meta")), FocalLoss2d(exponent=0.5), nn.NLLLoss(), nn.MSELoss(),
                ProbOhemCrossEntropy2d(255, thresh=1.5), ProbOhemCrossEntropy2d(255, weight=torch.rand(nc + 2))]
    fw = FocalLoss2d(weight=w)
    fw.loss.weight = w.double()                                                         # a focal weight of the wrong dtype
    declined.append(fw)
    for crit in taken + declined:
        assert pw.upsampled_loss(crit, x, s, lab) is None                               # CPU tensors
    xc65 = torch.randn(1, 2, 3, 65)
    assert pw.upsampled_loss(taken[0], xc65, s, lab) is None
    assert pw.upsampled_loss(taken[1], x, 64, lab) is None and pw.upsampled_loss(taken[1], x, s, lab[:, :-1]) is None
    assert pw.upsampled_loss(taken[1], x[0], s, lab) is None
    calls = []
    monkeypatch.setattr(pw, "_upsampled_rows", lambda coarse, scale, label: (coarse.reshape(-1, nc), label, 12, (1, 2, 3, int(scale))))
    monkeypatch.setattr(pw.UpsampledLossFn, "apply", staticmethod(lambda *a: calls.append(a[6:]) or "ran"))
    for crit in taken:
        assert pw.upsampled_loss(crit, x, s, lab) == "ran", crit
    assert [c[0] for c in calls] == ["options"] * 4 + ["focal"] * 3 + ["ohem"] * 2
    assert calls[1][1] == pytest.approx(0.1) and calls[4][1] == 2.0 and calls[6][1] == 3.5 and calls[7][1] == (0.7, 10)
    assert [c[2] for c in calls[:4]] == ["mean", "mean", "sum", "none"]
    n = len(calls)
    for crit in declined:
        assert pw.upsampled_loss(crit, x, s, lab) is None, crit
    assert len(calls) == n


def test_the_old_front_end_answers_as_before_on_cpu_tensors():
    import sigma_amd.pointwise as pw
    x, lab = torch.randn(1, 2, 3, 8), torch.zeros(1, 8, 12, dtype=torch.long)
    assert pw.upsampled_cross_entropy(nn.CrossEntropyLoss(), x, 4, lab) is None
    assert pw.upsampled_cross_entropy(nn.CrossEntropyLoss(reduction="sum"), x, 4, lab) is None
    assert pw.upsampled_cross_entropy(nn.CrossEntropyLoss(), x[0], 4, lab) is None
