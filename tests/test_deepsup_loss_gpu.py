"""The fused upsample + loss route for the criteria with options on the GPU -- run with -m gpu: the kernels of
csrc/deepsup.hip (sigma_upsample_loss_fwd / _bwd) against the fp64 twin of tests/deepsup_loss_twin.py under the bounds of
tests/deepsup_loss_bounds.py, through the C ABI and through ``pointwise.upsampled_loss``; the OHEM selection on the
upsampled nll; determinism, no host synchronisation, memory; and the product model's routing of its auxiliary terms.

Scale 1: the issue asks for the bits of the non-upsampled Functions where attainable.  They are not: the upsampled forward
forms lse with the ONLINE maximum (chunk by chunk, rescaling the sum when the maximum rises: the loop of
upsample_loss_fwd_kernel, which cannot hold an interpolated row of up to 64 classes in registers), the row kernels up to 64
classes take the maximum of the whole row FIRST.  The rescale s *= exp(m - m') rounds, so lse differs in its last bits and
everything after it does.  Scale 1 is therefore a case of the bounds like every other ((1, 4, 4, 1, 9, 12) in CASES), and
``test_scale_one_is_the_row_functions_up_to_the_bounds`` holds the two routes to the sum of their bounds."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from tests.deepsup_loss_bounds import (CASE_IDS, CASES, G1_CASE, G1_KIND, IGNORE, KINDS, OHEM_IDS, OHEM_PAIRS, U, bounds, class_weights,
                                       deepsup_inputs, ohem_gap, upstream_of)
from tests.deepsup_utils import build_ds_model
from tests.model_utils import fill

pytestmark = pytest.mark.gpu

DEV = "cuda"
OHEM_SPEC = dict(kind="ohem", weighted=True, eps=0.0, gamma=0.0, reduction="mean")


def _criterion(spec, w, thresh=0.7, min_kept=0):
    from sigma_amd.utils.loss_opr import FocalLoss2d, ProbOhemCrossEntropy2d
    if spec["kind"] == "focal":
        return FocalLoss2d(weight=w, reduction=spec["reduction"], ignore_index=IGNORE, exponent=spec["gamma"]).to(DEV)
    if spec["kind"] == "ohem":
        return ProbOhemCrossEntropy2d(IGNORE, reduction=spec["reduction"], thresh=thresh, min_kept=min_kept, weight=w).to(DEV)
    return nn.CrossEntropyLoss(weight=w, ignore_index=IGNORE, reduction=spec["reduction"], label_smoothing=spec["eps"]).to(DEV)


def _kernels(buf, lab, s, nc, spec, w, g):
    """sigma_upsample_loss_fwd then _bwd on device copies: lse, row_loss, partial, dlogits.  g: a float (scale_grad) or a
    per-pixel tensor (row_grad).  Every output starts as NaN."""
    from sigma_amd import _capi
    B, h, wd, ld = buf.shape
    nan = float("nan")
    x, y = buf.to(DEV).contiguous(), lab.to(DEV).contiguous()
    lse, row, coef = (torch.full(lab.shape, nan, device=DEV) for _ in range(3))
    partial = torch.full((_capi.SIGMA_CE_BLOCKS, 2), nan, device=DEV)
    dl = torch.full((B, h, wd, ld), nan, device=DEV)
    wdev = w.to(DEV) if w is not None else None
    gdev = g.to(DEV).float().contiguous() if torch.is_tensor(g) else torch.tensor([g], device=DEV, dtype=torch.float32)
    p = _capi.UpsampleLossParams()
    p.batch, p.height, p.width, p.scale, p.classes, p.ld, p.ignore_index = B, h, wd, s, nc, ld, IGNORE
    focal = spec["kind"] == "focal"
    p.kind = _capi.SIGMA_UPSAMPLE_LOSS_FOCAL if focal else _capi.SIGMA_UPSAMPLE_LOSS_OPTIONS
    p.label_smoothing, p.gamma = spec["eps"], spec["gamma"]
    p.logits, p.labels, p.lse, p.row_loss, p.partial = x.data_ptr(), y.data_ptr(), lse.data_ptr(), row.data_ptr(), partial.data_ptr()
    p.weight = wdev.data_ptr() if wdev is not None else None
    p.coef = coef.data_ptr() if focal else None
    if torch.is_tensor(g):
        p.row_grad = gdev.data_ptr()
    else:
        p.scale_grad = gdev.data_ptr()
    p.dlogits = dl.data_ptr()
    lib = _capi.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(lib.sigma_upsample_loss_fwd(ctypes.byref(p), st), "upsample_loss_fwd")
    _capi.check(lib.sigma_upsample_loss_bwd(ctypes.byref(p), st), "upsample_loss_bwd")
    torch.cuda.synchronize()
    return lse, row, partial, dl


def _front_end(buf, lab, s, nc, crit, upstream=1.0):
    """loss and the gradient of the (B, h, w, nc) view of a device copy of buf through upsampled_loss"""
    from sigma_amd.pointwise import upsampled_loss
    x = buf.to(DEV).requires_grad_(True)
    loss = upsampled_loss(crit, x[..., :nc], s, lab.to(DEV))
    if loss is None:
        return None, None
    if torch.is_tensor(upstream):
        (loss * upstream.to(DEV)).sum().backward()
    else:
        loss.backward()
    return loss.detach(), x.grad


def _check_kernels(case, name, spec):
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    w = class_weights(nc, spec["weighted"])
    none = spec["reduction"] == "none"
    g = upstream_of(spec, lab) if none else float(torch.tensor(1.0 / 37.0, dtype=torch.float32))
    b = bounds(buf[..., :nc].double(), lab, s, dict(spec, reduction="none" if none else "sum"), w, g)
    lse, row, partial, dl = _kernels(buf, lab, s, nc, spec, w, g)
    e = {"lse": (lse.cpu().double() - b["lse"]).abs() / b["E_lse"],
         "row": (row.cpu().double() - b["row"]).abs() / b["E_row"].clamp_min(1e-300),
         "p0": (partial[:, 0].cpu().double() - b["partial"][:, 0]).abs() / b["E_partial"][:, 0].clamp_min(1e-300),
         "p1": (partial[:, 1].cpu().double() - b["partial"][:, 1]).abs() / b["E_partial"][:, 1].clamp_min(1e-300),
         "dl": (dl[..., :nc].cpu().double() - b["dl"]).abs() / b["E_dl"]}
    print(name, " ".join(f"{k} {float(v.max()):.3f}" for k, v in e.items()), "of the bounds")
    for k, v in e.items():
        assert bool((v <= 1.0).all()), (name, k, float(v.max()))          # NaN fails
    if not spec["weighted"]:
        assert torch.equal(partial[:, 1].cpu().double(), b["partial"][:, 1])
    assert bool((row.cpu()[~b["valid"]] == 0).all())
    assert bool((dl[..., nc:] == 0).all()) and not bool(torch.signbit(dl[..., nc:]).any())
    again = _kernels(buf, lab, s, nc, spec, w, g)
    assert all(torch.equal(a, c) for a, c in zip((lse, row, partial, dl), again)), name


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_kernels_against_the_twin(case):
    """lse, row_loss, the partial pairs and every element of dlogits under the bounds, every kind; NaN in the pad of the
    logits, exact zeros in the pad of dlogits; a negative label and one inside the pad count as ignored (the inputs hold
    both); the same bits twice"""
    for name, spec in KINDS.items():
        _check_kernels(case, name, spec)


def test_kernels_against_the_twin_with_one_lane_per_item():
    _check_kernels(G1_CASE, G1_KIND, KINDS[G1_KIND])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_front_end_loss_and_gradient_against_the_twin(case):
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    for name, spec in KINDS.items():
        w = class_weights(nc, spec["weighted"])
        up = upstream_of(spec, lab)
        b = bounds(buf[..., :nc].double(), lab, s, spec, w, up)
        crit = _criterion(spec, w)
        loss, grad = _front_end(buf, lab, s, nc, crit, up)
        assert loss is not None, name
        e_loss = (loss.cpu().double() - b["loss"]).abs()
        e_dl = (grad[..., :nc].cpu().double() - b["dl"]).abs() / b["E_front"]
        print(name, f"loss {float((e_loss / b['E_loss']).max()):.3f} dl {float(e_dl.max()):.3f} of the bounds")
        assert bool((e_loss <= b["E_loss"]).all()) and bool((e_dl <= 1.0).all()), name
        assert bool((grad[..., nc:] == 0).all())
        loss2, grad2 = _front_end(buf, lab, s, nc, crit, up)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2), name


@pytest.mark.parametrize("pair", OHEM_PAIRS, ids=OHEM_IDS)
def test_ohem_keeps_the_twins_set_and_meets_the_bounds_on_it(pair):
    from sigma_amd.pointwise import upsampled_ohem_stages
    case, seed, thresh, min_kept, what = pair
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case, seed)
    w = class_weights(nc)
    _, near = ohem_gap(buf[..., :nc].double(), lab, s, thresh, min_kept)
    assert near == 0                                                       # the condition on the inputs
    b = bounds(buf[..., :nc].double(), lab, s, OHEM_SPEC, w, thresh=thresh, min_kept=min_kept)
    x = buf.to(DEV)
    r = upsampled_ohem_stages(x.view(-1, ld)[:, :nc], lab.to(DEV), w.to(DEV), IGNORE, ld, (B, h, wd, s), thresh, min_kept)
    assert torch.equal(r["mined"].cpu(), b["mined"])
    assert tuple(r["counts"].tolist()) == b["counts"]
    crit = _criterion(OHEM_SPEC, w, thresh, min_kept)
    loss, grad = _front_end(buf, lab, s, nc, crit)
    e_dl = (grad[..., :nc].cpu().double() - b["dl"]).abs() / b["E_front"]
    print(what, f"loss {abs(float(loss) - float(b['loss'])) / b['E_loss']:.3f} dl {float(e_dl.max()):.3f} of the bounds")
    assert abs(float(loss) - float(b["loss"])) <= b["E_loss"] and bool((e_dl <= 1.0).all())
    assert bool((grad[..., nc:] == 0).all())
    loss2, grad2 = _front_end(buf, lab, s, nc, crit)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_scale_one_is_the_row_functions_up_to_the_bounds():
    """upsampled_loss at scale 1 against SoftmaxCEOptFn / SoftmaxFocalFn / OhemCEFn on the same rows (through their front
    ends): not the same bits (module docstring), so each side is within its bound of the twin and the two within the sum"""
    from sigma_amd.pointwise import cross_entropy, focal_cross_entropy, ohem_cross_entropy
    case = (1, 4, 4, 1, 9, 12)
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    w = class_weights(nc)
    runs = [("w+eps", KINDS["w+eps"], {}), ("focal2w", KINDS["focal2w"], {}), ("ohem", OHEM_SPEC, dict(thresh=0.2, min_kept=4))]
    assert ohem_gap(buf[..., :nc].double(), lab, s, 0.2, 4)[1] == 0        # the condition on the OHEM input
    for name, spec, kw in runs:
        b = bounds(buf[..., :nc].double(), lab, s, spec, w, **kw)
        crit = _criterion(spec, w, **kw)
        loss, grad = _front_end(buf, lab, s, nc, crit)
        x = buf.to(DEV).requires_grad_(True)
        view, y = x[..., :nc].permute(0, 3, 1, 2), lab.to(DEV)
        if spec["kind"] == "focal":
            ref = focal_cross_entropy(view, y, IGNORE, spec["gamma"], weight=w.to(DEV))
        elif spec["kind"] == "ohem":
            ref = ohem_cross_entropy(view, y, IGNORE, kw["thresh"], kw["min_kept"], weight=w.to(DEV))
        else:
            ref = cross_entropy(crit, view, y)
        assert ref is not None
        ref.backward()
        print(name, "same bits:", torch.equal(loss, ref.detach()), torch.equal(grad, x.grad))
        assert abs(float(loss) - float(ref.detach())) <= 2 * b["E_loss"]
        assert bool(((grad - x.grad)[..., :nc].cpu().double().abs() <= 2 * b["E_front"]).all())


def _three(case):
    """(name, criterion) for the weighted, focal and OHEM criteria at the case's class count"""
    nc = case[4]
    w = class_weights(nc)
    return [("w", _criterion(KINDS["w"], w)), ("focal2w", _criterion(KINDS["focal2w"], w)),
            ("ohem", _criterion(OHEM_SPEC, w, 0.05, 16))]


def test_deterministic_flag_changes_nothing_and_runs_repeat_bitwise():
    case = (2, 5, 4, 4, 37, 40)
    buf, lab = deepsup_inputs(case)
    for name, crit in _three(case):
        loss, grad = _front_end(buf, lab, 4, 37, crit)
        torch.use_deterministic_algorithms(True)
        try:
            loss2, grad2 = _front_end(buf, lab, 4, 37, crit)
        finally:
            torch.use_deterministic_algorithms(False)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2), name


def test_front_end_reads_nothing_back():
    from sigma_amd.pointwise import upsampled_loss
    case = (2, 5, 4, 4, 37, 40)
    buf, lab = deepsup_inputs(case)
    for name, crit in _three(case):
        _front_end(buf, lab, 4, 37, crit)                  # warm-up: library load, allocator
        x, y = buf.to(DEV).requires_grad_(True), lab.to(DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = upsampled_loss(crit, x[..., :37], 4, y)
            loss.backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert bool(torch.isfinite(loss)), name


def test_nothing_labelled_gives_nan_loss_and_zero_gradient():
    case = (2, 2, 3, 16, 40, 40)
    buf, lab = deepsup_inputs(case)
    for name, crit in _three(case):
        loss, grad = _front_end(buf, torch.full_like(lab, IGNORE), 16, 40, crit)
        assert bool(torch.isnan(loss)) and bool((grad == 0).all()), name
    w0 = torch.zeros(40)                                   # only zero-weight classes: the denominator is zero as well
    loss, grad = _front_end(buf, lab, 16, 40, _criterion(KINDS["w"], w0))
    assert bool(torch.isnan(loss)) and bool((grad == 0).all())


def test_fused_route_allocates_less_than_one_full_size_logit_buffer():
    from sigma_amd.pointwise import upsampled_loss
    case = (2, 8, 12, 16, 40, 40)
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    full = B * h * s * wd * s * ld * 4
    for name, crit in _three(case):
        _front_end(buf, lab, s, nc, crit)                  # warm-up
        x, y = buf.to(DEV).requires_grad_(True), lab.to(DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = upsampled_loss(crit, x[..., :nc], s, y)
        loss.backward()
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
        print(f"{name}: growth {growth} bytes, one full-size logit buffer {full} bytes")
        assert growth < full, name


def test_what_the_front_end_declines():
    from sigma_amd.pointwise import upsampled_cross_entropy, upsampled_loss
    from sigma_amd.utils.loss_opr import FocalLoss2d
    case = (2, 5, 4, 4, 37, 40)
    B, h, wd, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    x, y = buf.to(DEV), lab.to(DEV)
    w = class_weights(nc).to(DEV)
    crit = nn.CrossEntropyLoss(weight=w, ignore_index=IGNORE)
    assert upsampled_loss(crit, x[..., :nc], s, y) is not None                                  # the control
    assert upsampled_loss(nn.CrossEntropyLoss(ignore_index=IGNORE), x[..., :nc], s, y) is None  # plain: the other front end's
    assert upsampled_cross_entropy(nn.CrossEntropyLoss(ignore_index=IGNORE), x[..., :nc], s, y) is not None
    assert upsampled_cross_entropy(crit, x[..., :nc], s, y) is None
    assert upsampled_loss(nn.CrossEntropyLoss(weight=w.double()), x[..., :nc], s, y) is None
    assert upsampled_loss(nn.CrossEntropyLoss(weight=w[:-1]), x[..., :nc], s, y) is None
    assert upsampled_loss(nn.CrossEntropyLoss(weight=w.cpu()), x[..., :nc], s, y) is None
    assert upsampled_loss(FocalLoss2d(exponent=0.5).to(DEV), x[..., :nc], s, y) is None
    assert upsampled_loss(crit, x[..., :nc], s, lab) is None                                    # a CPU label
    assert upsampled_loss(crit, x[..., :nc], s, y[:, :-1]) is None
    assert upsampled_loss(crit, x[..., :nc], 64, y) is None and upsampled_loss(crit, x[..., :nc], 2 * s, y) is None
    assert upsampled_loss(crit, x[..., 1:nc], s, y) is None                                     # rows off the 16-byte grid
    buf65, lab65 = deepsup_inputs((1, 2, 2, 4, 65, 68))
    assert upsampled_loss(nn.CrossEntropyLoss(label_smoothing=0.1), buf65.to(DEV)[..., :65], 4, lab65.to(DEV)) is None
    one = torch.randn(1, 1, 1, 9, device=DEV)          # a packed single row: the chunks of a pitch of 12 would end past it
    assert upsampled_loss(nn.CrossEntropyLoss(label_smoothing=0.1), one, 4, torch.zeros(1, 4, 4, device=DEV, dtype=torch.long)) is None


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _model_criterion(kind, nc):
    from sigma_amd.utils.loss_opr import FocalLoss2d, ProbOhemCrossEntropy2d
    w = class_weights(nc)
    if kind == "weighted":
        return nn.CrossEntropyLoss(weight=w, ignore_index=255)
    if kind == "focal":
        return FocalLoss2d(weight=w, ignore_index=255)
    return ProbOhemCrossEntropy2d(255, thresh=1.2 / nc, min_kept=2000, weight=w)      # an untrained model has p_y ~ 1 / nc


@pytest.mark.parametrize("nc", [40, 9])
@pytest.mark.parametrize("kind", ["weighted", "focal", "ohem"])
def test_fused_route_is_the_general_route_on_the_model(kind, nc, monkeypatch):
    """loss and all gradients of the same model through the two routes of the aux terms, with the tolerances and the
    reasoning of tests/test_deepsup_gpu.py::test_fused_route_is_the_general_route_on_the_model.  OHEM: both routes must
    keep the same pixels in every term -- a condition on the input, read from the mined labels of the two runs; another
    seed is drawn where a pixel at the threshold changes sides by rounding."""
    import sigma_amd.pointwise as pw
    model = build_ds_model(nc, 64, 96, criterion=_model_criterion(kind, nc)).to(DEV).eval()
    real_loss, real_select = pw.upsampled_loss, pw._ohem_select
    answers, mined = [], []

    def spy(*a, **k):
        r = real_loss(*a, **k)
        answers.append(r is not None)
        return r

    def select_spy(*a, **k):
        r = real_select(*a, **k)
        mined.append(r["mined"].reshape(-1).clone())
        return r

    monkeypatch.setattr(pw, "_ohem_select", select_spy)
    for seed in (3, 4, 5, 6):
        rgb, x, label = (t.to(DEV) for t in fill.make_inputs(2, 64, 96, nc, seed=seed))
        del answers[:], mined[:]
        model.zero_grad(set_to_none=True)
        monkeypatch.setattr(pw, "upsampled_loss", spy)
        loss_f = model(rgb, x, label)
        loss_f.backward()
        assert answers == [True, True, True]
        fused, mined_f = _grads(model), list(mined)
        model.zero_grad(set_to_none=True)
        del mined[:]
        monkeypatch.setattr(pw, "upsampled_loss", lambda *a, **k: None)
        loss_g = model(rgb, x, label)
        loss_g.backward()
        general = _grads(model)
        if kind != "ohem":
            assert not mined_f and not mined
            break
        assert len(mined_f) == len(mined) == 4                         # the main term and the three aux terms, either route
        kept = [int((m != 255).sum()) for m in mined]
        print(f"seed {seed}: kept {kept} of {label.numel()} per term")
        if all(torch.equal(a, b) for a, b in zip(mined_f, mined)):
            break
    else:
        pytest.fail("no seed at which both routes keep the same pixels")
    assert abs(float(loss_f) - float(loss_g)) <= 1e-5 * abs(float(loss_g))
    assert fused.keys() == general.keys() and any(".output_ds." in n for n in fused)
    worst = [(n, float((fused[n] - general[n]).abs().max()), float(general[n].abs().max())) for n in fused
             if float((fused[n] - general[n]).abs().max()) > 2e-3 * (float(general[n].abs().max()) + 2e-5)]
    assert not worst, worst[:5]


def test_plain_criterion_is_never_answered_by_the_new_front_end(monkeypatch):
    import sigma_amd.pointwise as pw
    model = build_ds_model(9, 64, 96).to(DEV).eval()
    rgb, x, label = (t.to(DEV) for t in fill.make_inputs(2, 64, 96, 9, seed=3))
    old, new = [], []
    real_old, real_new = pw.upsampled_cross_entropy, pw.upsampled_loss
    monkeypatch.setattr(pw, "upsampled_cross_entropy", lambda *a, **k: old.append(1) or real_old(*a, **k))
    monkeypatch.setattr(pw, "upsampled_loss", lambda *a, **k: new.append(real_new(*a, **k)) or new[-1])
    model(rgb, x, label).backward()
    assert len(old) == 3 and not new                      # the old front end answers all three: the new one is not asked
    monkeypatch.setattr(pw, "upsampled_cross_entropy", lambda *a, **k: None)
    model(rgb, x, label).backward()
    assert new == [None, None, None]                      # asked, and declines: the expansion runs


def test_graphed_step_with_the_ohem_criterion_equals_the_eager_step():
    """as tests/test_deepsup_gpu.py::test_graphed_step_with_the_flag_equals_the_eager_step, with its tolerances: the
    selection launches every kernel unconditionally, so the captured step takes the data's branch at replay.  The two
    models drift apart by the order of their float atomics (the tolerances allow for that), and OHEM is discontinuous in
    its input: with a threshold amid the pixels' p_y (1.2 / nc, as in the routing test) a pixel changes sides between the
    two and the loss jumps (measured: 1.5e-5 relative).  So the criterion here mines with thresh 0.7 and min_kept 16 --
    the mining branch runs, tau = -log 0.7 -- on a model whose p_y stay near 1 / 9: no pixel is near the threshold."""
    import sigma_amd.pointwise as pw
    from sigma_amd import train_step as ts
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    crit = ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=16, weight=class_weights(9))
    eager = build_ds_model(9, 64, 96, criterion=crit).to(DEV).eval()
    graphed = copy.deepcopy(eager)
    batch = tuple(t.to(DEV) for t in fill.make_inputs(2, 64, 96, 9, seed=8))
    taken = []
    real = pw.upsampled_loss
    pw.upsampled_loss = lambda *a, **k: taken.append(1) or real(*a, **k)
    try:
        opt_e = ts.make_optimizer(eager, capturable=True)
        opt_g = ts.make_optimizer(graphed, capturable=True)
        step_e = ts.make_step(eager, opt_e, batch)
        for _ in range(3):
            step_e()
        step_g, static = ts.make_graphed_step(graphed, opt_g, batch, warmup=3)
    finally:
        pw.upsampled_loss = real
    assert taken
    for _ in range(2):
        le = step_e()
        lg = step_g()
        torch.cuda.synchronize()
        torch.testing.assert_close(lg, le.detach(), rtol=1e-5, atol=1e-6)
    for (n, a), (_, b) in zip(eager.named_parameters(), graphed.named_parameters()):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=6e-4, msg=lambda m, n=n: f"{n}: {m}")
