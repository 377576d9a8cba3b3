"""The distillation-loss kernels (csrc/distill.hip, include/sigma_distill.h) on the GPU against the fp64 twin
(tests/distill_loss_twin.py, run on the device) under the derived bounds of tests/distill_loss_bounds.py: every class count
and pitch pair, the row counts around a workgroup and the second grid-stride trip, every temperature, both kd_all values,
the value regimes of tests/loss_regimes.py, -inf masks, the poisoned pad, the excluded rows, the exact case, repeatability,
the Function, ``DistillLoss2d`` alone and through ``EncoderDecoder.attach_teacher``, and stream capture.
tests/test_distill_loss_cpu.py holds an fp32 emulation and the twin's wrong variants against the same bounds on the same
inputs."""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import distill_loss_bounds as db
from tests.distill_loss_twin import twin

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGNORE = db.IGNORE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(buf, tbuf, lab, nc, T, kw, cw, kd_all, G, ignore=IGNORE, backward=True):
    """sigma_distill_loss_fwd and _bwd on device tensors buf (rows, ld), tbuf (rows, ld_t) and lab (rows,): dict of device
    tensors loss, terms, coef, lse (rows, 3) and dl (rows, ld), the outputs filled with NaN before the launches"""
    from sigma_amd import _capi_distill
    from sigma_amd._launch import launch
    lib = _capi_distill.load()
    rows, ld = buf.shape
    nan = lambda *shape: torch.full(shape, float("nan"), device=buf.device)
    out = dict(loss=nan(1), terms=nan(2), coef=nan(2), lse=nan(rows, 3), dl=nan(rows, ld))
    p = _capi_distill.DistillParams()
    p.rows, p.classes, p.ld, p.ld_t, p.kd_all, p.ignore_index = rows, nc, ld, tbuf.shape[1], int(kd_all), ignore
    p.temperature, p.kd_weight, p.ce_weight = T, kw, cw
    p.logits, p.teacher, p.labels = buf.data_ptr(), tbuf.data_ptr(), lab.data_ptr()
    p.lse, p.coef = out["lse"].data_ptr(), out["coef"].data_ptr()
    nbytes = int(lib.sigma_distill_loss_workspace_bytes(ctypes.byref(p)))
    ws = torch.full((nbytes // 4 + 16,), float("nan"), device=buf.device)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
    p.loss, p.terms = out["loss"].data_ptr(), out["terms"].data_ptr()
    launch("sigma_distill_loss_fwd", ctypes.byref(p), device=buf.device)
    if backward:
        scale = torch.tensor([G], device=buf.device, dtype=torch.float32)
        p.scale, p.dlogits = scale.data_ptr(), out["dl"].data_ptr()
        launch("sigma_distill_loss_bwd", ctypes.byref(p), device=buf.device)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nbytes // 4:]).all()), "the workspace was written past the size the query answered"
    return out


@functools.lru_cache(maxsize=None)
def _inputs(rows, nc, ld, ldt):
    return db.distill_inputs(rows, nc, ld, ldt, seed=rows + nc)


def _check(buf, tbuf, lab, nc, par, what, finite_loss=True):
    """every output of the kernels on (buf, tbuf, lab) against the twin on the device: all rows, all columns"""
    T, kw, cw, kd_all, G = par
    assert bool(torch.isnan(buf[:, nc:]).all()) and bool(torch.isnan(tbuf[:, nc:]).all())          # the pad is poisoned
    x, te, y = buf.to(DEV), tbuf.to(DEV), lab.to(DEV)
    t = db.bounds(x[:, :nc].double(), te[:, :nc].double(), y, nc, T, kw, cw, kd_all, G)
    out = kernels(x, te, y, nc, *par)
    assert torch.equal(y.cpu(), lab) and torch.equal(te.view(torch.int32).cpu(), tbuf.view(torch.int32)), "an input was modified"
    rs = db.worst_ratio(dict(out, loss=out["loss"][0]), t, nc)
    if not finite_loss:
        assert float(out["loss"]) == float("inf") == float(t["loss"]) and float(out["terms"][0]) == float("inf"), (what, out["loss"])
        rs = {k: v for k, v in rs.items() if k not in ("loss", "kd")}
    print(what, {k: round(v, 4) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), (what, rs)
    dl = out["dl"]
    outside = ~(t["in_s"] | t["valid"])
    assert not dl[:, nc:].any() and not dl[outside].any(), "pad columns and rows outside both sets must be exact zeros"
    return out, t


def test_kernels_match_the_twin():
    """every class count and pitch pair, every row count around a workgroup, every parameter set -- all four temperatures,
    both kd_all values, ce_weight zero and not.  One case: the 160 launch pairs with their twins take about four seconds
    together, and the suite counts cases"""
    for nc, ld, ldt in db.CLASS_CASES:
        for rows in db.ROW_COUNTS:
            buf, tbuf, lab = _inputs(rows, nc, ld, ldt)
            for pi, par in enumerate(db.PARAM_CASES):
                _check(buf, tbuf, lab, nc, par, f"{rows}x{nc}@{ld}@{ldt} params {pi}")


def test_second_grid_stride_trip():
    """SIGMA_CE_BLOCKS * 256 + 257 rows: every thread of the forward has a row, 257 of them a second one"""
    nc, ld, ldt = db.BIG_CASE
    buf, tbuf, lab = _inputs(db.BIG_ROWS, nc, ld, ldt)
    _check(buf, tbuf, lab, nc, db.PARAM_CASES[2], f"{db.BIG_ROWS}x{nc}@{ld}@{ldt}")


def test_value_regimes():
    """the finite regimes of tests/loss_regimes.py in both tensors; the -inf regime with the same classes masked in both and
    with classes masked in the teacher only: a masked class has q = 0 and contributes exactly 0; and classes masked in the
    student only: an infinite loss, a finite gradient"""
    for rows, nc, ld, ldt in db.REGIME_CASES:
        for regime in db.UNMASKED_REGIMES + db.MASK_KINDS:
            pair = db.masked_pair if regime in db.MASK_KINDS else db.regime_pair
            buf, tbuf, lab = pair(regime, rows, nc, ld, ldt, seed=700 + nc)
            for par in db.REGIME_PARAMS:
                out, t = _check(buf, tbuf, lab, nc, par, f"{regime} {rows}x{nc} T {par[0]}")
                assert bool(torch.isfinite(out["dl"]).all())
                if regime in db.MASK_KINDS:
                    masked = torch.isinf(tbuf[:, :nc])
                    assert bool(masked.any()) and not t["q"][masked.to(DEV)].any()
    buf, tbuf, lab = db.masked_pair("student", 300, 9, 12, 12, seed=709)
    out, t = _check(buf, tbuf, lab, 9, (2.0, 1.0, 0.5, False, 1.0), "student-only mask", finite_loss=False)
    assert bool(torch.isfinite(out["dl"]).all()) and float(out["dl"].abs().max()) > 0 and bool(torch.isfinite(out["terms"][1]))


def _ignored_rows_carry_the_kd_gradient_only_with_kd_all():
    """kd_all with a cross-entropy term: the rows that are not valid get the bytes they get with ce_weight = 0 (the KD
    coefficient does not depend on it), and they are not zero; without kd_all they are exact zeros"""
    buf, tbuf, lab = _inputs(257, 9, 12, 12)
    x, te, y = buf.to(DEV), tbuf.to(DEV), lab.to(DEV)
    invalid = ~db.is_valid(y, 9, IGNORE)
    both = kernels(x, te, y, 9, 2.0, 0.7, 0.5, True, 0.37)
    kd_only = kernels(x, te, y, 9, 2.0, 0.7, 0.0, True, 0.37)
    assert int(invalid.sum()) > 20 and torch.equal(both["coef"][0], kd_only["coef"][0]) and float(both["coef"][1]) > 0
    assert torch.equal(both["dl"][invalid], kd_only["dl"][invalid]) and bool(both["dl"][invalid][:, :9].abs().sum(1).gt(0).all())
    assert not torch.equal(both["dl"][~invalid], kd_only["dl"][~invalid])
    assert not kernels(x, te, y, 9, 2.0, 0.7, 0.5, False, 0.37)["dl"][invalid].any()


def _no_valid_row_and_no_rows():
    buf, tbuf, lab = _inputs(257, 9, 12, 12)
    lab = torch.where(torch.arange(257) % 2 == 0, torch.full_like(lab, IGNORE), torch.full_like(lab, -3))
    x, te, y = buf.to(DEV), tbuf.to(DEV), lab.to(DEV)
    out = kernels(x, te, y, 9, 2.0, 1.0, 1.0, False, 1.0)
    for k in ("loss", "terms", "coef", "dl"):
        assert not out[k].any(), k                         # exact zeros, the pad included
    out = kernels(x, te, y, 9, 2.0, 1.0, 1.0, True, 1.0)   # every row is in S: the KD term alone
    t = twin(x[:, :9].double(), te[:, :9].double(), y, IGNORE, 2.0, 1.0, 1.0, True)
    assert float(out["terms"][1]) == 0.0 and float(out["coef"][1]) == 0.0 and float(out["terms"][0]) > 0
    assert abs(float(out["loss"]) - float(t["loss"])) <= 1e-5 * float(t["loss"]) and bool(out["dl"][:, :9].any())
    # rows == 0: both entry points accept it; the forward writes zeros, the backward launches nothing
    empty = kernels(x[:0], te[:0], y[:0], 9, 2.0, 1.0, 1.0, True, 1.0)
    for k in ("loss", "terms", "coef"):
        assert not empty[k].any(), k


def _exact_case(T):
    """the teacher's bits equal the student's, at another pitch: kl_r and p - q are exact zeros"""
    buf, _, lab = _inputs(257, 37, 40, 44)
    x = buf.to(DEV)
    te = torch.full((257, 44), float("nan"), device=DEV)
    te[:, :37] = x[:, :37]
    y = lab.to(DEV)
    for kd_all in (False, True):
        out = kernels(x, te, y, 37, T, 1.0, 0.0, kd_all, -2.5)
        assert float(out["terms"][0]) == 0.0 and float(out["loss"]) == 0.0 and float(out["coef"][0]) > 0
        assert bool((out["dl"] == 0).all())
        lse = out["lse"]
        assert torch.equal(lse[:, 1], lse[:, 2]) and (T != 1.0 or torch.equal(lse[:, 0], lse[:, 1]))
    out = kernels(x, te, y, 37, T, 1.0, 1.0, True, 1.0)     # with a cross-entropy term: that term alone
    t = twin(x[:, :37].double(), te[:, :37].double(), y, IGNORE, T, 0.0, 1.0)
    assert float(out["terms"][0]) == 0.0 and db.ratio(out["dl"][:, :37], t["dl"], db.bounds(
        x[:, :37].double(), te[:, :37].double(), y, 37, T, 0.0, 1.0, False, 1.0)["S_dl"]) <= 1.0


def test_edge_cases():
    """the excluded rows, no valid row and no row at all, and the exact case at T = 1 and T = 2"""
    _ignored_rows_carry_the_kd_gradient_only_with_kd_all()
    _no_valid_row_and_no_rows()
    for T in (1.0, 2.0):
        _exact_case(T)


def test_two_runs_give_identical_bytes():
    """two raw runs, and the Function without and with torch's deterministic flag: the same bytes"""
    from sigma_amd.pointwise import distill_loss
    nc, ld, ldt = db.BIG_CASE
    buf, tbuf, lab = _inputs(db.BIG_ROWS, nc, ld, ldt)
    x, te, y = buf.to(DEV), tbuf.to(DEV), lab.to(DEV)
    par = db.PARAM_CASES[1]
    first, again = kernels(x, te, y, nc, *par), kernels(x, te, y, nc, *par)
    for k in first:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k
    B, H, W = 1, 257, 40
    x4 = x[:H * W].view(B, H, W, ld)[..., :nc].permute(0, 3, 1, 2)
    t4 = te[:H * W].view(B, H, W, ldt)[..., :nc].permute(0, 3, 1, 2)
    saved = torch.are_deterministic_algorithms_enabled()
    flat = []
    try:
        for flag in (False, False, True, True):
            torch.use_deterministic_algorithms(flag)
            leaf = x4.detach().requires_grad_(True)
            loss = distill_loss(leaf, t4, y[:H * W].view(B, H, W), IGNORE, 2.0, 0.7, 0.5, True)
            (loss * 0.37).backward()
            flat.append((loss.detach().clone(), leaf.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(saved)
    assert len(flat) == 4 and all(torch.equal(flat[0][0], r[0]) and torch.equal(flat[0][1], r[1]) for r in flat[1:])
    assert float(flat[0][1].abs().max()) > 0


def _function_is_the_kernels(nc, ld, ldt):
    """``distill_loss`` on the (B, classes, H, W) views of channels-last rows, contiguous or padded, the two pitches
    different: the bytes of the raw launches; the teacher gets no gradient, nor do the labels; it runs with frozen logits
    and under no_grad"""
    from sigma_amd.pointwise import distill_loss
    B, H, W = 2, 11, 13
    buf, tbuf, lab = db.distill_inputs(B * H * W, nc, ld, ldt, seed=7)
    T, kw, cw, kd_all, G = par = db.PARAM_CASES[1]
    x, te, y = buf.to(DEV), tbuf.to(DEV), lab.to(DEV)
    raw = kernels(x, te, y, nc, *par)
    base, tbase = x.clone().requires_grad_(True), te.clone().requires_grad_(True)
    logits = base.view(B, H, W, ld)[..., :nc].permute(0, 3, 1, 2)
    teacher = tbase.view(B, H, W, ldt)[..., :nc].permute(0, 3, 1, 2)
    y3 = y.view(B, H, W)
    loss, terms = distill_loss(logits, teacher, y3, IGNORE, T, kw, cw, kd_all, with_terms=True)
    (loss * G).backward()
    assert loss.dim() == 0 and torch.equal(loss.detach(), raw["loss"][0]) and torch.equal(terms, raw["terms"]) and not terms.requires_grad
    assert torch.equal(base.grad[:, :nc], raw["dl"][:, :nc]) and not base.grad[:, nc:].any()
    assert tbase.grad is None
    with torch.no_grad():
        assert torch.equal(distill_loss(logits, teacher, y3, IGNORE, T, kw, cw, kd_all), raw["loss"][0])
    frozen = distill_loss(logits.detach(), teacher, y3, IGNORE, T, kw, cw, kd_all)
    assert not frozen.requires_grad and torch.equal(frozen, raw["loss"][0])
    # what the path does not take
    assert distill_loss(logits.contiguous(), teacher, y3, IGNORE, T, kw, cw, kd_all) is None
    assert distill_loss(logits, teacher.contiguous(), y3, IGNORE, T, kw, cw, kd_all) is None
    assert distill_loss(logits, teacher[:, :nc - 1], y3, IGNORE, T, kw, cw, kd_all) is None
    assert distill_loss(logits, teacher.cpu(), y3, IGNORE, T, kw, cw, kd_all) is None
    assert distill_loss(logits, teacher, y3, IGNORE, 0.0, kw, cw, kd_all) is None
    assert distill_loss(logits, teacher, y3, IGNORE, T, -1.0, cw, kd_all) is None


def test_function_and_class_routes():
    """``distill_loss`` at a padded and a contiguous pitch on either side, then ``DistillLoss2d`` on both of its routes"""
    for nc, ld, ldt in [(9, 12, 16), (40, 40, 44), (40, 44, 40)]:
        _function_is_the_kernels(nc, ld, ldt)
    _distill_loss2d_routes()


def _distill_loss2d_routes():
    """the class on the kernels (``last_terms``) and on its torch formulation: NCHW logits, and more than 64 classes.  The
    torch formulation is fp32 ATen sums over 286 pixels of terms of order 1: 1e-5 is 168 u, above the (pixels + classes) u / 2
    of a pairwise fp32 sum and far below what a wrong route would give"""
    from sigma_amd.utils.loss_opr import DistillLoss2d
    B, H, W, nc = 2, 11, 13, 8
    buf, tbuf, lab = db.distill_inputs(B * H * W, nc, nc, 12, seed=9)
    t = twin(buf.double(), tbuf[:, :nc].double(), lab, IGNORE, 2.0, 1.0, 0.5)
    crit = DistillLoss2d(2.0, 1.0, 0.5)
    nhwc, tnhwc, y3 = buf.to(DEV).view(B, H, W, nc), tbuf.to(DEV).view(B, H, W, 12)[..., :nc], lab.to(DEV).view(B, H, W)
    loss = crit(nhwc.permute(0, 3, 1, 2), y3, tnhwc.permute(0, 3, 1, 2))
    assert crit.last_terms is not None and crit.last_terms.is_cuda
    assert abs(float(crit.last_terms[0]) - float(t["kd"])) < 1e-5 and abs(float(crit.last_terms[1]) - float(t["ce"])) < 1e-5
    crit2 = DistillLoss2d(2.0, 1.0, 0.5)
    nchw = nhwc.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    loss2 = crit2(nchw, y3, tnhwc.permute(0, 3, 1, 2))
    loss2.backward()
    assert crit2.last_terms is None and abs(float(loss2.detach()) - float(t["loss"])) < 1e-5 and abs(float(loss) - float(t["loss"])) < 1e-5
    got = nchw.grad.permute(0, 2, 3, 1).reshape(-1, nc).cpu().double()
    assert float((got - t["dl"]).abs().max()) < 1e-6
    wide = torch.randn(1, 4, 5, 68, device=DEV).permute(0, 3, 1, 2)
    twide = torch.randn(1, 4, 5, 68, device=DEV).permute(0, 3, 1, 2)
    y = torch.randint(0, 68, (1, 4, 5), device=DEV)
    crit3 = DistillLoss2d(2.0)
    rows = lambda v: v.permute(0, 2, 3, 1).reshape(-1, 68).cpu().double()
    tw = twin(rows(wide), rows(twide), y.view(-1).cpu(), IGNORE, 2.0)
    assert abs(float(crit3(wide, y, twide)) - float(tw["loss"])) < 1e-5 * max(1.0, float(tw["loss"])) and crit3.last_terms is None


@contextlib.contextmanager
def _stochastic_depth_off():
    """Every DropPath draw keeps every sample: ``train()`` without its randomness.  And torch's deterministic flag for the
    duration: without it the split-operand GEMMs of the network may add their slices with float atomics, so
    that two forwards of the same model on the same batch differ in their last bits and nothing could be compared bit for
    bit."""
    from sigma_amd.models.encoders.vmamba import DropPath
    saved = (DropPath.draw_mask, torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory,
             os.environ.get("CUBLAS_WORKSPACE_CONFIG"))
    DropPath.draw_mask = lambda self, x, keep: x.new_ones((x.shape[0],) + (1,) * (x.dim() - 1))
    os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":4096:8")
    torch.use_deterministic_algorithms(True)
    torch.utils.deterministic.fill_uninitialized_memory = False
    try:
        yield
    finally:
        DropPath.draw_mask = saved[0]
        torch.use_deterministic_algorithms(saved[1])
        torch.utils.deterministic.fill_uninitialized_memory = saved[2]
        if saved[3] is None:
            os.environ.pop("CUBLAS_WORKSPACE_CONFIG", None)


def test_through_the_model():
    """A student and a teacher (the fixture model with perturbed parameters) in ``train()`` with stochastic depth given as
    all-keep masks, under torch's deterministic flag (``_stochastic_depth_off``).  The loss runs on the kernels (``last_terms``); loss and logits gradient are held to
    ``criterion.torch_formulation`` in fp64 on the SAME logits under the bounds of tests/distill_loss_bounds.py.  Every
    student parameter gradient is held to the backward of that fp64 gradient, rounded to fp32, through a second forward of
    the same network: the map from the logits gradient to a parameter gradient is linear and is run by the same kernels
    both times, so what differs is the logits gradient (<= u S_dl, checked element by element) and the rounding of the network's backward --
    for which the model tests of this suite (tests/model_utils.py) allow 5e-3 of the gradient's largest element + 2e-5; the
    same allowance is used here."""
    from sigma_amd.utils.loss_opr import DistillLoss2d
    from tests.model_utils import build_model, fill
    nc = 9
    student, teacher = build_model("sigma_tiny", nc, 64, 96).to(DEV), build_model("sigma_tiny", nc, 64, 96).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        for p in teacher.parameters():
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, device=DEV, generator=g))
    rgb, x, label = (t.to(DEV) for t in fill.make_inputs(2, 64, 96, nc, seed=3))
    crit = DistillLoss2d(2.0, 1.0, 0.5)
    student.train()
    seen = []
    real = crit.forward

    def spy(out, lab, t):
        out.retain_grad()
        seen.append((out, t))
        return real(out, lab, t)

    crit.forward = spy
    with _stochastic_depth_off():
        plain = student(rgb, x, label).detach().clone()
        student.attach_teacher(teacher, crit)
        assert student.training and not teacher.training
        before = [p.detach().clone() for p in teacher.parameters()]
        loss = student(rgb, x, label)
        assert crit.last_terms is not None and crit.last_terms.is_cuda, "the model's logits did not take the kernels"
        (out, t), = seen
        assert not t.requires_grad and tuple(t.shape) == tuple(out.shape) == (2, nc, 64, 96)
        loss.backward()
        got = {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}
        # the fp64 reference on the same logits
        rows = lambda v: v.detach().permute(0, 2, 3, 1).reshape(-1, nc).double()
        leaf = out.detach().double().requires_grad_(True)
        ref = crit.torch_formulation(leaf, label, t.double())
        ref.backward()
        b = db.bounds(rows(out), rows(t), label.view(-1), nc, 2.0, 1.0, 0.5, False, 1.0)
        assert abs(float(ref.detach()) - float(b["loss"])) <= 1e-12 * abs(float(b["loss"]))
        rs = dict(loss=db.ratio(loss.detach(), ref.detach(), b["S_loss"]), dl=db.ratio(rows(out.grad), rows(leaf.grad), b["S_dl"]))
        print("through the model", rs, float(loss.detach()))
        assert all(v <= 1.0 for v in rs.values()), rs
        # the reference's logits gradient through a second forward of the same network (the masks are given: same logits)
        student.zero_grad(set_to_none=True)
        again = student.encode_decode(rgb, x)
        assert torch.equal(again.detach(), out.detach())
        again.backward(leaf.grad.float())
        bad = []
        for n, p in student.named_parameters():
            assert (p.grad is None) == (n not in got), n
            if p.grad is not None and float((got[n] - p.grad).abs().max()) > 5e-3 * (float(p.grad.abs().max()) + 2e-5):
                bad.append((n, float((got[n] - p.grad).abs().max()), float(p.grad.abs().max())))
        assert not bad, bad[:5]
        assert sum(float(v.abs().max()) > 0 for v in got.values()) > 100
        # detached: the plain loss again, bit for bit
        student.detach_teacher()
        assert torch.equal(student(rgb, x, label).detach(), plain) and len(seen) == 1
        # attached again: an optimizer step moves the student alone
        student.attach_teacher(teacher, crit)
        assert all(p.grad is None for p in teacher.parameters())
        torch.optim.AdamW(student.parameters(), lr=1e-3).step()
        assert all(torch.equal(a, p) for a, p in zip(before, teacher.parameters()))
        assert not torch.equal(student(rgb, x, label).detach(), loss.detach()) and len(seen) == 2


def test_capture_replays_to_the_eager_bytes():
    r = subprocess.run([sys.executable, "-m", "tests.distill_capture_worker"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[distill_capture_worker] done" in r.stdout, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
