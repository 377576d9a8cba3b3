"""The region-overlap loss kernels (csrc/region.hip, include/sigma_region.h) on the GPU against the fp64 twin
(tests/region_loss_twin.py) under the derived bounds of tests/region_loss_bounds.py: every class count and pitch, the row
counts around a workgroup and the second grid-stride trip, the exact case, the edge cases, repeatability, the pad, the
Function, ``RegionLoss2d`` through the model (both routes) and stream capture.  tests/test_region_loss_cpu.py holds an fp32
emulation and the twin's wrong variants against the same bounds on the same inputs."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import region_loss_bounds as rb
from tests.region_loss_twin import twin

pytestmark = pytest.mark.gpu

DEV = "cuda"
IGNORE = rb.IGNORE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(buf, lab, nc, a, b, s, rw, cw, G, ignore=IGNORE):
    """sigma_region_loss_fwd and _bwd on device tensors buf (rows, ld) and lab (rows,): dict of device tensors loss, terms,
    sums (3, nc), coef, lse and dl (rows, ld), the outputs filled with NaN before the launches"""
    from sigma_amd import _capi_region
    from sigma_amd._launch import launch
    lib = _capi_region.load()
    rows, ld = buf.shape
    nan = lambda *shape: torch.full(shape, float("nan"), device=buf.device)
    out = dict(loss=nan(1), terms=nan(2), sums=nan(3, nc), coef=nan(2 * nc + 1), lse=nan(rows), dl=nan(rows, ld))
    p = _capi_region.RegionParams()
    p.rows, p.classes, p.ld, p.ignore_index = rows, nc, ld, ignore
    p.alpha, p.beta, p.smooth, p.region_weight, p.ce_weight = a, b, s, rw, cw
    p.logits, p.labels, p.lse, p.coef = buf.data_ptr(), lab.data_ptr(), out["lse"].data_ptr(), out["coef"].data_ptr()
    nbytes = int(lib.sigma_region_loss_workspace_bytes(ctypes.byref(p)))
    ws = torch.full((nbytes // 4 + 16,), float("nan"), device=buf.device)
    p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
    p.loss, p.terms, p.sums = out["loss"].data_ptr(), out["terms"].data_ptr(), out["sums"].data_ptr()
    launch("sigma_region_loss_fwd", ctypes.byref(p), device=buf.device)
    scale = torch.tensor([G], device=buf.device, dtype=torch.float32)
    p.scale, p.dlogits = scale.data_ptr(), out["dl"].data_ptr()
    launch("sigma_region_loss_bwd", ctypes.byref(p), device=buf.device)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nbytes // 4:]).all()), "the workspace was written past the size the query answered"
    return out


@functools.lru_cache(maxsize=None)
def _inputs(rows, nc, ld):
    return rb.region_inputs(rows, nc, ld, seed=rows + nc)


def _params(pi):
    kind, s, rw, cw, G = rb.PARAM_CASES[pi]
    return (*rb.ab_of(kind), s, rw, cw, G)


def _check(buf, lab, nc, par, what):
    """every output of the kernels on (buf, lab) against the twin: all rows, all columns"""
    a, b, s, rw, cw, G = par
    t = rb.bounds(buf[:, :nc].double(), lab, nc, a, b, s, rw, cw, G)
    lab_dev = lab.to(DEV)
    out = {k: v.cpu() for k, v in kernels(buf.to(DEV), lab_dev, nc, *par).items()}
    assert torch.equal(lab_dev.cpu(), lab), "the labels were modified"
    rs = rb.worst_ratio(dict(out, loss=out["loss"][0]), t, nc)
    rs["coef"] = rb.ratio(out["coef"], torch.cat([t["A"], t["B"], torch.as_tensor(t["cwn"]).reshape(1)]), t["S_coef"])
    valid = t["valid"]
    rs["lse"] = rb.ratio(out["lse"][valid], t["lse"][valid], t["S_lse"][valid])
    print(what, {k: round(v, 4) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), (what, rs)
    dl = out["dl"]
    assert not dl[:, nc:].any() and not dl[~valid].any(), "pad columns and rows that are not valid must be exact zeros"
    assert torch.equal(out["sums"][2], t["sums"][2].float()), "the label counts are exact"
    return out, t


@pytest.mark.parametrize("nc,ld", rb.CLASS_CASES)
def test_kernels_match_the_twin(nc, ld):
    """one case per class count and pitch; inside it every row count around a workgroup with every parameter set (each
    launch pair is a fraction of a second, so the twelve stay one quick case)"""
    for rows in rb.ROW_COUNTS:
        buf, lab = _inputs(rows, nc, ld)
        for pi in range(len(rb.PARAM_CASES)):
            _check(buf, lab, nc, _params(pi), f"{rows}x{nc}@{ld} params {pi}")


def test_second_grid_stride_trip():
    """SIGMA_CE_BLOCKS * 256 + 257 rows: every thread of the forward has a row, 257 of them a second one"""
    buf, lab = _inputs(rb.BIG_ROWS, 5, 8)
    _check(buf, lab, 5, _params(2), f"{rb.BIG_ROWS}x5@8")


@pytest.mark.parametrize("nc,ld", [(5, 8), (40, 40)])
def test_exact_case(nc, ld):
    """-inf everywhere but one finite column per row: p is exactly 0 or 1, so the sums are integer counts, bit for bit"""
    rows = 1000
    g = torch.Generator().manual_seed(5)
    r = torch.arange(rows)
    hot = torch.randint(0, nc, (rows,), generator=g)       # the label's column, the only finite one of most rows
    lab = hot.clone()
    lab[r % 10 == 7] = IGNORE
    lab[r % 10 == 3] = -2
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = float("-inf")
    buf[r, hot] = torch.randn(rows, generator=g) * 3.0
    # rows whose prediction misses the label: a second finite column 200 above the label's, exp(-200) = 0 in fp32
    miss = r % 5 == 1
    other = (hot + 1) % nc
    buf[r[miss], other[miss]] = buf[r[miss], hot[miss]] + 200.0
    pred = torch.where(miss, other, hot)
    valid = rb.is_valid(lab, nc, IGNORE)
    want = torch.zeros(3, nc)
    for c in range(nc):
        want[0, c] = int((valid & (lab == c) & (pred == c)).sum())
        want[1, c] = int((valid & (pred == c)).sum())
        want[2, c] = int((valid & (lab == c)).sum())
    out = kernels(buf.to(DEV), lab.to(DEV), nc, 0.5, 0.5, 0.0, 1.0, 0.0, 1.0)
    assert torch.equal(out["sums"].cpu(), want) and float(want[0].sum()) > 0 and float((want[1] - want[0]).sum()) > 0
    dl = out["dl"].cpu()
    assert bool(torch.isfinite(dl).all()) and not dl[:, nc:].any() and not dl[~valid].any()
    t = twin(buf[:, :nc].double(), lab, IGNORE, 0.5, 0.5)
    assert abs(float(out["loss"]) - float(t["loss"])) <= rb.U * abs(float(t["loss"]))      # exact sums, fp64, one rounding


def test_all_pixels_ignored():
    buf, lab = _inputs(257, 9, 12)
    lab = torch.where(torch.arange(257) % 2 == 0, torch.full_like(lab, IGNORE), torch.full_like(lab, -3))
    out = kernels(buf.to(DEV), lab.to(DEV), 9, 0.5, 0.5, 1.0, 1.0, 1.0, 1.0)
    for k in ("loss", "terms", "sums", "coef", "dl"):
        assert not out[k].cpu().any(), k                   # exact zeros, the pad included


def test_one_class_present_and_a_class_never_labelled():
    buf, lab = _inputs(257, 9, 12)
    plain, lab1 = rb.region_inputs(257, 9, 12, seed=21, masked=False)      # no -inf: any column may become the label's
    one = torch.where(rb.is_valid(lab1, 9, IGNORE), torch.full_like(lab1, 4), lab1)
    out, t = _check(plain, one, 9, _params(2), "one class present")
    assert int(t["kcount"]) == 1
    coef = out["coef"]
    others = [c for c in range(9) if c != 4]
    assert not coef[others].any() and not coef[9:18][others].any() and float(coef[4]) < 0 < float(coef[9 + 4])
    # class 8 is never a label in these inputs: predicted (P_8 > 0), outside K (zero coefficients), whatever the kind
    out, t = _check(buf, lab, 9, _params(1), "absent class")
    assert float(out["sums"][1, 8]) > 0 and float(out["sums"][2, 8]) == 0 and int(t["kcount"]) == 8
    assert float(out["coef"][8]) == 0 and float(out["coef"][9 + 8]) == 0


def test_labels_outside_the_classes_are_ignored():
    """labels in [classes, ld) and negative ones give the bytes of ignore_index at the same rows"""
    buf, lab = _inputs(257, 5, 8)
    assert bool(((lab >= 5) & (lab < 8)).any()) and bool((lab < 0).any())
    clean = torch.where(rb.is_valid(lab, 5, IGNORE), lab, torch.full_like(lab, IGNORE))
    x = buf.to(DEV)
    got, want = kernels(x, lab.to(DEV), 5, *_params(2)), kernels(x, clean.to(DEV), 5, *_params(2))
    for k in ("loss", "terms", "sums", "coef", "dl"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_runs_give_identical_bytes(deterministic):
    from sigma_amd.pointwise import region_loss
    buf, lab = _inputs(rb.BIG_ROWS, 5, 8)
    x, y = buf.to(DEV), lab.to(DEV)
    first = kernels(x, y, 5, *_params(2))
    again = kernels(x, y, 5, *_params(2))
    for k in first:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), k
    saved = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        runs = []
        x4 = x[:257 * 40].view(1, 257, 40, 8)[..., :5].permute(0, 3, 1, 2)
        for _ in range(2):
            leaf = x4.detach().requires_grad_(True)
            loss = region_loss(leaf, y[:257 * 40].view(1, 257, 40), IGNORE, 0.3, 0.7, 0.5, 0.8, 1.25)
            (loss * 0.37).backward()
            runs.append((loss.detach().clone(), leaf.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    finally:
        torch.use_deterministic_algorithms(saved)


@pytest.mark.parametrize("nc,ld", [(9, 12), (40, 40)])
def test_function_is_the_kernels(nc, ld):
    """``region_loss`` on the (B, classes, H, W) view of channels-last rows: the bytes of the raw launches; it runs with
    frozen logits and under no_grad, and the labels get no gradient"""
    from sigma_amd.pointwise import region_loss
    B, H, W = 2, 11, 13
    buf, lab = rb.region_inputs(B * H * W, nc, ld, seed=7)
    a, b, s, rw, cw, G = par = _params(2)
    x, y = buf.to(DEV), lab.to(DEV)
    raw = kernels(x, y, nc, *par)
    base = x.clone().requires_grad_(True)
    logits = base.view(B, H, W, ld)[..., :nc].permute(0, 3, 1, 2)
    loss, terms, sums = region_loss(logits, y.view(B, H, W), IGNORE, a, b, s, rw, cw, with_terms=True)
    (loss * G).backward()
    assert loss.dim() == 0 and torch.equal(loss.detach(), raw["loss"][0]) and torch.equal(terms, raw["terms"]) and torch.equal(sums, raw["sums"])
    assert not terms.requires_grad and not sums.requires_grad
    assert torch.equal(base.grad[:, :nc], raw["dl"][:, :nc]) and not base.grad[:, nc:].any()
    with torch.no_grad():
        assert torch.equal(region_loss(logits, y.view(B, H, W), IGNORE, a, b, s, rw, cw), raw["loss"][0])
    frozen = region_loss(logits.detach(), y.view(B, H, W), IGNORE, a, b, s, rw, cw)
    assert not frozen.requires_grad and torch.equal(frozen, raw["loss"][0])
    # what the path does not take
    assert region_loss(logits.contiguous(), y.view(B, H, W), IGNORE, a, b, s, rw, cw) is None
    assert region_loss(logits, y.view(B, H, W), IGNORE, a, 0.0, s, rw, cw) is None


def test_region_loss2d_routes():
    """the class on the kernels (``last_terms``) and on its torch formulation: NCHW logits, and more than 64 classes.  The
    torch formulation is fp32 ATen sums over 286 pixels of terms below 1 (loss and terms of order 1): 1e-5 is 168 u, above
    the (pixels + classes) u / 2 of a pairwise fp32 sum and far below what a wrong route would give"""
    from sigma_amd.utils.loss_opr import RegionLoss2d
    B, H, W, nc = 2, 11, 13, 8
    buf, lab = rb.region_inputs(B * H * W, nc, nc, seed=9, masked=False)
    crit = RegionLoss2d("jaccard", smooth=1.0, ce_weight=0.5)
    t = twin(buf.double(), lab, IGNORE, 1.0, 1.0, 1.0, 1.0, 0.5)
    nhwc = buf.to(DEV).view(B, H, W, nc)
    loss = crit(nhwc.permute(0, 3, 1, 2), lab.to(DEV).view(B, H, W))
    assert crit.last_terms is not None and crit.last_terms.is_cuda
    assert abs(float(crit.last_terms[0]) - float(t["region"])) < 1e-5 and abs(float(crit.last_terms[1]) - float(t["ce"])) < 1e-5
    crit2 = RegionLoss2d("jaccard", smooth=1.0, ce_weight=0.5)
    nchw = nhwc.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    loss2 = crit2(nchw, lab.to(DEV).view(B, H, W))
    loss2.backward()
    assert crit2.last_terms is None and abs(float(loss2.detach()) - float(t["loss"])) < 1e-5 and abs(float(loss) - float(t["loss"])) < 1e-5
    got = nchw.grad.permute(0, 2, 3, 1).reshape(-1, nc).cpu().double()
    assert float((got - t["dl"]).abs().max()) < 1e-6
    wide = torch.randn(1, 4, 5, 68, device=DEV).permute(0, 3, 1, 2)
    y = torch.randint(0, 68, (1, 4, 5), device=DEV)
    crit3 = RegionLoss2d("dice")
    tw = twin(wide.permute(0, 2, 3, 1).reshape(-1, 68).cpu().double(), y.view(-1).cpu(), IGNORE, 0.5, 0.5)
    assert abs(float(crit3(wide, y)) - float(tw["loss"])) < 1e-5 and crit3.last_terms is None


def _through_the_model(model, nc):
    """loss and every logits gradient of a model whose criterion is a ``RegionLoss2d``: equal, bit for bit, to
    ``RegionLossFn`` called on the same logits"""
    import sigma_amd.pointwise as pw
    from tests.model_utils import fill
    rgb, x, label = (t.to(DEV) for t in fill.make_inputs(2, 64, 96, nc, seed=3))
    seen = []
    real = pw.region_loss

    def spy(logits, *a, **k):
        out = real(logits, *a, **k)
        assert out is not None, "the model's logits did not take the kernels"
        logits.retain_grad()
        seen.append(logits)
        return out

    pw.region_loss, saved = spy, pw.region_loss
    try:
        loss = model(rgb, x, label)
        loss.backward()
    finally:
        pw.region_loss = saved
    crit = model.criterion
    total = None
    for logits in seen:
        assert logits.grad is not None
        leaf = logits.detach().requires_grad_(True)
        args = pw._loss_rows(leaf, label, None)
        assert args is not None
        logits2, lab, _, ld = args
        term = pw.RegionLossFn.apply(logits2, lab, crit.ignore_index, ld, crit.alpha, crit.beta, crit.smooth, crit.region_weight,
                                     crit.ce_weight)[0]
        term.backward()
        assert torch.equal(leaf.grad, logits.grad) and float(leaf.grad.abs().max()) > 0
        total = term.detach() if total is None else total + term.detach()
    assert torch.equal(total, loss.detach())
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.parameters())
    return len(seen)


def test_region_loss2d_through_the_model():
    from sigma_amd.utils.loss_opr import RegionLoss2d
    from tests.model_utils import cfg_for, fill
    from sigma_amd.models.builder import EncoderDecoder
    crit = RegionLoss2d("dice", smooth=1.0, ce_weight=1.0)
    cwd = os.getcwd()
    os.chdir("/tmp")                  # the (absent) pretrained/ path is relative, as in tests/model_utils.build_model
    try:
        model = EncoderDecoder(cfg_for("sigma_tiny", 9, 64, 96), criterion=crit, norm_layer=torch.nn.BatchNorm2d)
    finally:
        os.chdir(cwd)
    fill.fill_parameters(model)
    assert _through_the_model(model.to(DEV).eval(), 9) == 1


def test_region_loss2d_through_the_model_with_deep_supervision():
    from sigma_amd.utils.loss_opr import RegionLoss2d
    from tests.deepsup_utils import build_ds_model
    model = build_ds_model(9, 64, 96, criterion=RegionLoss2d("tversky", alpha=0.3, beta=0.7, ce_weight=0.5)).to(DEV).eval()
    assert _through_the_model(model, 9) == 4              # x_last and the three expanded aux heads


def test_capture_replays_to_the_eager_bytes():
    r = subprocess.run([sys.executable, "-m", "tests.region_capture_worker"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "[region_capture_worker] done" in r.stdout, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
