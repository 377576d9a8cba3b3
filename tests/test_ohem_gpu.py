"""OHEM cross entropy on the HIP loss path: sigma_ohem_select exactly against torch.sort, ProbOhemCrossEntropy2d end to end
on the padded view against the fp64 twin (tests/ohem_fp64_twin.py), the route, the model, deterministic mode and graph
capture; run with -m gpu.

The select kernel works on fp32 keys it is GIVEN, so its test is exact: tau bit for bit, counts and mined element for
element.  End to end the keys are the kernel's own nll = lse - x_y, which differ from the twin's fp64 values by rounding:
|nll32 - nll64| <= (C + 8) u (|lse| + 1) + u (|lse| + |x_y|) (the lse bound of tests/test_loss_options_gpu.py and one
subtraction), and tau is either one of these keys or -log(thresh) rounded once.  A valid row can change sides only if it
lies that close to tau; the inputs are CHOSEN so that none does: the tests assert, on the twin's fp64 values, that no valid
row lies within delta_r = 64 u (|lse_r| + |x_{r,y}| + 1) of tau (64 >= C + 10 does not hold for the 65- and 67-class cases:
there the same assertion is made with C + 10 in place of 64).  Exempt are rows that are bit-identical copies of the row that
defines tau -- planted, so that ties are exercised: equal inputs give equal keys on either side -- and the one-class case,
where nll is exactly 0 in fp64 and on the kernel (lse = x).  The seeds below were found on the CPU, where the twin runs;
the share of rows the assertion may exclude is zero.

Under that condition the kept set equals the twin's and loss and gradient are the cross-entropy kernels' on the mined
labels; the bounds are those of tests/test_loss_options_gpu.py (``_k_row``, ``_k_sum``, ``_k_dl``).  What the rows-sized
summation adds: in the kernel nothing -- ohem_final_kernel forms w_y * nll, the product ce_opt_row_loss forms at eps = 0,
and adds the rows in the order and with the block sum of the forward kernel (the test below asks for the same BITS as
sigma_softmax_ce_opt_fwd on the mined labels).  Outside it, torch adds the SIGMA_CE_BLOCKS partial pairs; the tests there
keep to 256 rows so that one pair is non-zero.  Here nb = ceil(rows / 256) pairs are: adding the others is exact, and the
nb - 1 roundings cost at most (nb - 1) u S in any order.  So: loss sum K = _k_sum + _k_row + nb - 1; denominator
K_den = _k_sum + nb - 1; 'mean' = sum / den: K = (K of the sum) + K_den + 1 on S / den; gradient through the device-formed
upstream / den: _k_dl + K_den + 2 (tests/test_loss_options_gpu.py: 2C + 37 where K_den = 11).
"""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from sigma_amd import _capi
from tests.ohem_fp64_twin import VARIANTS, twin
from tests.test_head_classes_gpu import CE_LD_CASES, IGNORE, _boom
from tests.test_loss_options_gpu import _k_dl, _k_row, _k_sum, _ref
from tests.test_stream_fp64_gpu import U, _guarded, _intact, check, rejects

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = "ohem cross entropy"
SENT = -0x5A5A5A5A5A5A5A5A


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# sigma_ohem_select on given keys

def _nl_thresh(thresh):
    """(float)(0.0 - log((double)thresh)) with thresh held as a float, as the entry point forms it"""
    return np.float32(0.0 - math.log(float(np.float32(thresh))))


def _select_ref(keys, lab, nc, thresh, min_kept):
    """torch.sort on the same fp32 keys (CPU): tau (np.float32), (num_valid, kept), mined"""
    valid = (lab != IGNORE) & (lab >= 0) & (lab < nc)
    nv = int(valid.sum())
    if 0 < min_kept <= nv:
        kth = torch.sort(keys[valid], descending=True).values[min_kept - 1].numpy()
        nlt = _nl_thresh(thresh)
        tau = kth if kth < nlt else nlt
        keep = valid & ~(keys < float(tau))
    else:
        tau, keep = np.float32("-inf"), valid
    return np.float32(tau), (nv, int(keep.sum())), torch.where(keep, lab, torch.full_like(lab, IGNORE))


def _guarded_i64(n, margin=64):
    buf = torch.full((n + 2 * margin,), SENT, device=DEV, dtype=torch.int64)
    return buf, buf[margin:margin + n], margin


def _intact_i64(g, what):
    buf, view, m = g
    n = view.numel()
    assert bool((buf[:m] == SENT).all()) and bool((buf[m + n:] == SENT).all()), f"{what}: guard band written"


def _run_select(keys, lab, nc, thresh, min_kept):
    lib = _capi.load()
    rows = keys.numel()
    k_d, l_d = keys.to(DEV), lab.to(DEV)
    mined, counts = _guarded_i64(rows), _guarded_i64(2)
    tau = _guarded((1,), 64)
    need = int(lib.sigma_ohem_workspace_bytes(rows))
    ws = torch.full((need + 512,), 0xA5, device=DEV, dtype=torch.uint8)
    p = _capi.OhemParams()
    p.rows, p.ignore_index, p.classes, p.thresh, p.min_kept = rows, IGNORE, nc, thresh, min_kept
    p.nll, p.labels = k_d.data_ptr() if rows else None, l_d.data_ptr() if rows else None
    p.mined, p.tau, p.counts = mined[1].data_ptr() if rows else None, tau[1].data_ptr(), counts[1].data_ptr()
    p.workspace, p.workspace_bytes = ws[256:].data_ptr(), need
    _capi.check(lib.sigma_ohem_select(ctypes.byref(p), _stream()), "ohem_select")
    torch.cuda.synchronize()
    _intact_i64(mined, "mined")
    _intact_i64(counts, "counts")
    _intact(tau, "tau")
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + need:] == 0xA5).all()), "workspace: guard band written"
    return tau[1].cpu().numpy()[0], tuple(int(v) for v in counts[1].cpu()), mined[1].cpu()


def _keys(rows, seed, ignored=0.1, nc=5):
    g = torch.Generator().manual_seed(seed)
    keys = (torch.randn(rows, generator=g) * 2.0).abs()
    lab = torch.randint(0, nc, (rows,), generator=g)
    drop = torch.rand(rows, generator=g) < ignored
    lab[drop] = IGNORE
    keys[drop] = 0.0                                   # what the forward writes at ignored rows
    return keys, lab


def _from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.float32).copy())


SWEEP = _capi.SIGMA_OHEM_HIST_BLOCKS * 256                # rows one grid sweep of ohem_hist_kernel covers (csrc/ohem.hip)
SIZES = (1, 255, 256, 257, SWEEP + 3)


def _select_cases():
    cases = {}
    for rows in SIZES:
        keys, lab = _keys(rows, seed=400 + rows % 97)
        if rows == 1:
            lab[0], keys[0] = 2, 0.5
        nv = int((lab != IGNORE).sum())
        cases[f"rows{rows}"] = (keys, lab, 5, 0.7, max(1, nv // 3))        # thresh or the k-th value, as the data say
        cases[f"rows{rows}_kth"] = (keys, lab, 5, 1e-6, max(1, nv // 2))   # -log thresh = 13.8: the k-th value governs
    keys, lab = _keys(3000, seed=411)
    nv = int((lab != IGNORE).sum())
    for name, k in (("k1", 1), ("k_valid", nv), ("k_valid_plus_1", nv + 1), ("k0", 0), ("k_negative", -3)):
        cases[name] = (keys, lab, 5, 1e-6, k)
    cases["thresh_one"] = (keys, lab, 5, 1.0, nv // 2)                      # tau = min(k-th, 0): every valid row stays
    cases["all_equal"] = (torch.full((1000,), 1.25), torch.randint(0, 5, (1000,), generator=torch.Generator().manual_seed(412)), 5, 0.05, 500)
    # 50 bit-identical keys straddling rank k
    keys, lab = _keys(3000, seed=413, ignored=0.0)
    order = torch.sort(keys, descending=True).indices
    keys[order[980:1030]] = float(keys[order[1000]])
    cases["ties_straddle_k"] = (keys, lab, 5, 1e-6, 1001)
    # keys that differ only in the lowest digit / only in the highest digit (both signs, all finite)
    r = np.arange(2000)
    cases["lowest_digit"] = (_from_bits(0x3F800000 + (r * 7) % 256), torch.zeros(2000, dtype=torch.int64), 5, 1e-6, 777)
    hi = _from_bits(((r * 5) % 256).astype(np.uint32) << 24)
    cases["highest_digit_top"] = (hi, torch.zeros(2000, dtype=torch.int64), 5, 1e-6, 40)
    cases["highest_digit_low"] = (hi, torch.zeros(2000, dtype=torch.int64), 5, 1e-6, 1800)     # a negative k-th value
    # zeros of ignored rows next to valid rows whose key is zero, the k-th value among the zeros
    keys, lab = _keys(2000, seed=414, ignored=0.3)
    keys[::3] = 0.0
    nv = int((lab != IGNORE).sum())
    cases["zeros_mixed"] = (keys, lab, 5, 1e-6, nv - 5)
    keys, lab = _keys(2000, seed=415)
    keys[5:900:50] = float("inf")
    lab[5:900:50] = 1
    cases["inf_keys_k2"] = (keys, lab, 5, 0.7, 2)
    cases["inf_keys_kth"] = (keys, lab, 5, 1e-30, 2)                        # -log thresh = 69: the k-th value, +inf, does not govern
    # labels outside [0, classes) count as ignored
    keys, lab = _keys(1000, seed=416)
    lab[::7], lab[3::11] = 5, -1
    cases["labels_out_of_range"] = (keys, lab, 5, 1e-6, 300)
    return cases


SELECT_CASES = None


def _select_case(name):
    global SELECT_CASES
    if SELECT_CASES is None:
        SELECT_CASES = _select_cases()
    return SELECT_CASES[name]


SELECT_NAMES = ([f"rows{r}{s}" for r in SIZES for s in ("", "_kth")] +
                ["k1", "k_valid", "k_valid_plus_1", "k0", "k_negative", "thresh_one", "all_equal", "ties_straddle_k", "lowest_digit",
                 "highest_digit_top", "highest_digit_low", "zeros_mixed", "inf_keys_k2", "inf_keys_kth", "labels_out_of_range"])


@pytest.mark.parametrize("name", SELECT_NAMES)
def test_select_is_exact(name):
    """tau bit-equal to the value torch.sort of the same fp32 keys gives, counts and mined equal element for element,
    guard bands around mined, tau, counts and the workspace intact"""
    keys, lab, nc, thresh, k = _select_case(name)
    assert set(SELECT_NAMES) == set(SELECT_CASES)
    tau, counts, mined = _run_select(keys, lab, nc, thresh, k)
    want_tau, want_counts, want_mined = _select_ref(keys, lab, nc, thresh, k)
    assert tau.tobytes() == want_tau.tobytes(), (tau, want_tau)
    assert counts == want_counts
    assert torch.equal(mined, want_mined)
    if name == "ties_straddle_k":
        assert counts[1] == 1030                       # every tie is kept: more than k rows survive
    if name in ("k_valid_plus_1", "k0", "k_negative"):
        assert tau == np.float32("-inf") and counts[0] == counts[1]


def test_select_with_no_rows_writes_tau_and_counts():
    tau, counts, mined = _run_select(torch.zeros(0), torch.zeros(0, dtype=torch.int64), 5, 0.7, 10)
    assert tau == np.float32("-inf") and counts == (0, 0) and mined.numel() == 0


def test_select_survives_nan_keys():
    """NaN keys (NaN logits) of either sign: the call returns, mined holds labels or ignore_index only and the valid
    count is right; which side of tau they land on is not specified"""
    keys, lab = _keys(3000, seed=421)
    keys[::13] = float("nan")
    keys[5::17] = -float("nan")
    valid = lab != IGNORE
    for k in (1, 700, int(valid.sum())):
        tau, counts, mined = _run_select(keys, lab, 5, 0.7, k)
        assert counts[0] == int(valid.sum()) and 0 <= counts[1] <= counts[0]
        assert bool(((mined == lab) | (mined == IGNORE)).all()) and int((mined != IGNORE).sum()) == counts[1]
        assert not math.isnan(float(tau))


# ---------------------------------------------------------------------------------------------------------------------
# end to end on the padded view

E2E_CASES = CE_LD_CASES + [(3001, 40, 40)]
# seeds for which no valid row lies within delta_r of tau (found on the CPU: the twin runs there)
E2E_SEEDS = {case: 500 for case in E2E_CASES}
BRANCHES = ("thresh", "kth")


def _weights_cpu(nc, seed):
    w = torch.rand(nc, generator=torch.Generator().manual_seed(seed)) * 2.0 + 0.1
    if nc > 1:
        w[nc // 2] = 0.0
    return w


def _e2e_inputs(case, branch):
    """CPU tensors: x (rows, nc) fp32 ~ N(0, 3^2); labels as tests/test_head_classes_gpu.py::_labels (10 % ignored, labels
    inside the pad and negative ones); thresh, min_kept of the branch.  "kth": two bit-identical copies of the row that
    defines tau are planted over rows that would have been dropped."""
    rows, nc, ld = case
    g = torch.Generator().manual_seed(E2E_SEEDS[case])
    x = torch.randn(rows, nc, generator=g) * 3.0
    lab = torch.randint(0, nc, (rows,), generator=g)
    lab[torch.rand(rows, generator=g) < 0.1] = IGNORE
    r = torch.arange(rows)
    if ld > nc:
        lab = torch.where(r % 7 == 3, nc + r % (ld - nc), lab)
    lab = torch.where(r % 11 == 5, -1 - r % 3, lab)
    if rows == 1:
        lab[0] = nc - 1
    nv = int(((lab != IGNORE) & (lab >= 0) & (lab < nc)).sum())
    if branch == "thresh":
        thresh, min_kept = 0.7, max(1, nv // 16)
    else:
        thresh, min_kept = 1e-6, max(1, 3 * nv // 4)
        t = twin(x, lab, IGNORE, thresh, min_kept)
        if t["tau_row"] >= 0 and min_kept + 4 < nv:
            order = torch.sort(t["p"], stable=True).indices
            for j in (int(order[min_kept]), int(order[min_kept + 4])):      # valid rows above the threshold: k + 2 rows survive
                x[j], lab[j] = x[t["tau_row"]], lab[t["tau_row"]]
    return x, lab, thresh, min_kept


def _gap_violations(case, x, lab, t):
    """valid rows within delta_r of tau that are neither copies of the row defining tau nor rows of the one-class case"""
    rows, nc, ld = case
    if not t["mining"]:
        return 0
    delta = max(64, nc + 10) * U * (t["lse"].abs() + t["xy"].abs() + 1.0)
    near = t["valid"] & (t["dist"] <= delta)
    if nc == 1:
        exempt = t["nll"] == 0.0
    elif t["tau_row"] >= 0:
        exempt = (x == x[t["tau_row"]]).all(1) & (lab == lab[t["tau_row"]])
    else:
        exempt = torch.zeros_like(near)
    return int((near & ~exempt).sum())


def _padded_view(x, ld):
    rows, nc = x.shape
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :nc] = x
    buf = buf.to(DEV).view(1, 1, rows, ld).requires_grad_()
    return buf, buf[..., :nc].permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", E2E_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in E2E_CASES])
def test_class_on_the_padded_view_against_the_twin(case):
    """ProbOhemCrossEntropy2d on the (1, nc, 1, rows) view of a (rows, ld) buffer whose pad holds NaN: both mining
    branches (thresh governs / the k-th value governs, with planted ties) and min_kept above the valid count, with and
    without class weights (one class with weight zero), every reduction.  The gap condition of the module docstring is
    asserted first; then the kept set is the twin's exactly (mined labels, counts), the partial sums and row losses of
    the select kernel are the BITS of sigma_softmax_ce_opt_fwd on the mined labels, loss and gradient lie under the
    bounds of the module docstring, the pad of the gradient is exact zeros, and each wrong variant of the twin fails."""
    from sigma_amd.pointwise import OhemCEFn, SoftmaxCEOptFn, ohem_cross_entropy, ohem_stages
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    rows, nc, ld = case
    lib = _capi.load()
    nb = min(-(-rows // 256), _capi.SIGMA_CE_BLOCKS)
    K_den = _k_sum(rows) + nb - 1
    K_sum = _k_sum(rows) + _k_row(nc) + nb - 1
    failed = set()
    ratios = {}
    for branch in BRANCHES + ("none",):
        x, lab, thresh, min_kept = _e2e_inputs(case, "kth" if branch == "none" else branch)
        if branch == "none":
            min_kept = rows + 1                                       # above the valid count: nothing is mined
        lab_d = lab.to(DEV)
        x64 = x.double().to(DEV)
        for has_w in (False, True):
            w = _weights_cpu(nc, seed=431).to(DEV) if has_w else None
            t = twin(x, lab, IGNORE, thresh, min_kept, weight=w.cpu() if has_w else None)
            nv = int(t["valid"].sum())
            assert _gap_violations(case, x, lab, t) == 0, "the inputs put a valid row within rounding of tau: choose another seed"
            if nv >= 16 and nc > 1:
                assert t["mining"] == (branch != "none")
                if branch == "thresh":
                    assert t["threshold"] == thresh and int(t["keep"].sum()) > min_kept
                if branch == "kth":
                    assert t["threshold"] > thresh and int(t["keep"].sum()) == min_kept + 2             # the planted ties
            # the stages directly: kept set, counts, tau, and the bits of a forward on the mined labels
            buf, view = _padded_view(x, ld)
            logits2 = view.detach().permute(0, 2, 3, 1).reshape(-1, nc)
            st = ohem_stages(logits2, lab_d, w, IGNORE, ld, thresh, min_kept, want_row_loss=True)
            torch.cuda.synchronize()
            assert torch.equal(st["mined"].cpu(), t["mined"]), f"{branch}: kept set differs from the twin's"
            assert tuple(int(v) for v in st["counts"].cpu()) == (nv, int(t["keep"].sum()))
            if not t["mining"]:
                assert float(st["tau"]) == float("-inf")
            elif t["tau_row"] < 0:
                assert st["tau"].cpu().numpy()[0].tobytes() == _nl_thresh(thresh).tobytes()
            else:
                assert float(st["tau"]) == float(st["nll"][t["tau_row"]])
            lse2 = torch.empty(rows, device=DEV)
            row2 = torch.empty(rows, device=DEV)
            part2 = torch.empty(_capi.SIGMA_CE_BLOCKS, 2, device=DEV)
            p = SoftmaxCEOptFn._params(logits2, st["mined"], w, lse2, IGNORE, ld, 0.0)
            p.row_loss, p.partial = row2.data_ptr(), part2.data_ptr()
            _capi.check(lib.sigma_softmax_ce_opt_fwd(ctypes.byref(p), _stream()), "ce opt fwd on the mined labels")
            torch.cuda.synchronize()
            assert torch.equal(st["partial"], part2) and torch.equal(st["row_loss"], row2) and torch.equal(st["lse"], lse2)
            mined_d = t["mined"].to(DEV)
            r0 = _ref(x64, mined_d, nc, w, 0.0, 0.0)
            den = float(r0["wy"].sum())
            S_sum = r0["S_row"].sum().view(1)
            for red in ("mean", "sum", "none"):
                crit = ProbOhemCrossEntropy2d(IGNORE, red, thresh, min_kept, weight=w)
                up = (torch.randn(rows, generator=torch.Generator().manual_seed(432)).to(DEV).view(1, 1, rows) if red == "none"
                      else torch.tensor(1.7, device=DEV))
                buf, view = _padded_view(x, ld)
                if rows == 1:
                    # a one-row view has no pitch to read (any strides are contiguous): the layout gate declines it, as that
                    # of cross_entropy does, and the class takes its torch formulation; the Function is given the pitch
                    assert ohem_cross_entropy(view, lab_d.view(1, 1, rows), IGNORE, thresh, min_kept, weight=w, reduction=red) is None
                    assert bool(torch.isfinite(crit(view, lab_d.view(1, 1, rows))).all())
                    loss = OhemCEFn.apply(buf.view(-1, ld)[:, :nc], lab_d, w, IGNORE, ld, thresh, min_kept, red, (1, 1, rows))
                else:
                    loss = crit(view, lab_d.view(1, 1, rows))
                assert type(loss.grad_fn).__name__.startswith(OhemCEFn.__name__)
                (loss * up).sum().backward()
                g = buf.grad.view(-1, ld)
                assert bool((g[:, nc:] == 0).all()), "pad columns of the gradient are not exact zeros"
                assert bool((g[~t["keep"].to(DEV)] == 0).all()), "a dropped row has a gradient"
                tag = f"{branch} {'w ' if has_w else ''}{red}"
                if red == "none":
                    assert tuple(loss.shape) == (1, 1, rows)
                    ratios[tag] = check(FAMILY, loss.detach().view(-1), r0["row"], r0["S_row"], _k_row(nc), f"per-pixel loss ({tag})")
                    assert bool((loss.detach().view(-1)[~t["keep"].to(DEV)] == 0).all())
                    gup, K = up.view(-1), _k_dl(nc)
                elif red == "sum":
                    ratios[tag] = check(FAMILY, loss.detach().double().view(1), r0["row"].sum().view(1), S_sum, K_sum, f"loss ({tag})")
                    gup, K = float(up), _k_dl(nc)
                elif den == 0.0:
                    assert bool(torch.isnan(loss)) and bool((g == 0).all()), "a zero denominator: NaN loss, zero gradient"
                    continue
                else:
                    ratios[tag] = check(FAMILY, loss.detach().double().view(1), (r0["row"].sum() / den).view(1), S_sum / den,
                                        K_sum + K_den + 1, f"loss ({tag})")
                    gup, K = float(up) / den, _k_dl(nc) + K_den + 2
                    wrong = twin(x, lab, IGNORE, thresh, min_kept, weight=w.cpu() if has_w else None, variant="den_valid")
                    if wrong["den"] != t["den"] and math.isfinite(float(wrong["loss"])):
                        try:
                            rejects(loss.detach().double().view(1), wrong["loss"].to(DEV).view(1), S_sum / den, K_sum + K_den + 1, "den_valid")
                            failed.add("den_valid")
                        except AssertionError:
                            pass
                r = _ref(x64, mined_d, nc, w, 0.0, gup)
                ratios[tag + " grad"] = check(FAMILY, g[:, :nc], r["dl"], r["S_dl"], K, f"gradient ({tag})")
            for variant in ("exact_k", "strict"):
                wrong = twin(x, lab, IGNORE, thresh, min_kept, weight=w.cpu() if has_w else None, variant=variant)
                if not torch.equal(st["mined"].cpu(), wrong["mined"]):
                    failed.add(variant)
    print(f"\n{case}: worst ratio {max(ratios.values()):.3g} of the bound ({max(ratios, key=ratios.get)})")
    if rows >= 255 and nc > 1:
        assert failed == set(VARIANTS), f"wrong variants the kernel's output did not fail: {set(VARIANTS) - failed}"


# ---------------------------------------------------------------------------------------------------------------------
# route, model, deterministic mode, capture

def test_route_runs_without_torch_and_declines_contiguous_nchw(monkeypatch):
    """With F.cross_entropy, softmax and sort raising, the class still returns on the padded view (9 classes at pitch 12)
    and on contiguous channels-last logits (40 classes).  Contiguous (B, 5, H, W) logits are declined by
    ohem_cross_entropy and take the class's torch formulation, which agrees with the twin."""
    from sigma_amd.pointwise import ohem_cross_entropy
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    crit = ProbOhemCrossEntropy2d(IGNORE, "mean", 0.7, 50)
    g = torch.Generator().manual_seed(441)
    lab = torch.randint(0, 5, (2, 9, 11), generator=g)
    lab[torch.rand(2, 9, 11, generator=g) < 0.1] = IGNORE
    lab = lab.to(DEV)
    with monkeypatch.context() as m:
        for mod, name in ((F, "cross_entropy"), (F, "softmax"), (torch, "softmax"), (torch, "sort"), (torch, "argsort"), (F, "nll_loss"),
                          (F, "log_softmax")):
            m.setattr(mod, name, _boom)
        for nc, ld in ((9, 12), (40, 40)):
            buf = (torch.randn(2, 9, 11, ld, generator=g) * 3.0).to(DEV).requires_grad_()
            loss = crit(buf[..., :nc].permute(0, 3, 1, 2), lab)
            loss.backward()
            torch.cuda.synchronize()
            assert torch.isfinite(loss) and bool(torch.isfinite(buf.grad).all()) and bool((buf.grad[..., nc:] == 0).all())
        nchw = (torch.randn(2, 5, 9, 11, generator=g) * 3.0).to(DEV)
        assert ohem_cross_entropy(nchw, lab, IGNORE, 0.7, 50) is None
        with pytest.raises(AssertionError):
            crit(nchw, lab)                                           # the fallback is torch's: it meets the patched functions
    x = nchw.clone().requires_grad_()
    loss = crit(x, lab)
    loss.backward()
    t = twin(nchw.permute(0, 2, 3, 1).reshape(-1, 5).cpu(), lab.view(-1).cpu(), IGNORE, 0.7, 50)
    torch.testing.assert_close(loss.detach().double().cpu(), t["loss"], rtol=1e-5, atol=0.0)
    kept = x.grad.permute(0, 2, 3, 1).reshape(-1, 5).abs().sum(1) != 0
    assert torch.equal(kept.cpu(), t["keep"])
    # other dtypes, a weight of another dtype or size, a thresh outside (0, 1]: declined, not refused
    pad = torch.randn(2, 9, 11, 8, device=DEV)
    view = pad[..., :5].permute(0, 3, 1, 2)
    assert ohem_cross_entropy(view, lab, IGNORE, 0.7, 50) is not None
    assert ohem_cross_entropy(view.double(), lab, IGNORE, 0.7, 50) is None
    assert ohem_cross_entropy(view, lab, IGNORE, 0.7, 50, weight=torch.ones(5, device=DEV, dtype=torch.float64)) is None
    assert ohem_cross_entropy(view, lab, IGNORE, 0.7, 50, weight=torch.ones(4, device=DEV)) is None
    assert ohem_cross_entropy(view, lab, IGNORE, 1.5, 50) is None
    assert ohem_cross_entropy(view, lab, IGNORE, 0.7, 50, reduction="batchmean") is None


@pytest.mark.parametrize("nc,thresh", [(9, 0.7), (40, 1e-6)], ids=["9-thresh", "40-kth"])
def test_model_step_with_the_ohem_criterion(nc, thresh):
    """sigma_tiny 64x96, batch 1 (eval mode: no random depth), criterion = ProbOhemCrossEntropy2d(255, min_kept = a quarter
    of the pixels; thresh governs with 9 classes, the k-th value with 40, whose untrained logits leave no pixel above 0.7): loss and every parameter gradient are finite and equal those of the same model with
    nn.CrossEntropyLoss on the labels the twin mines from the model's own logits -- loss at rtol 1e-5
    (tests/test_loss_options_gpu.py), gradients under the model-level tolerance of tests/test_model_gpu.py (rtol 1e-4,
    atol 1e-6 + 1e-5 max |grad|).  The gap condition is asserted on the model's logits."""
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    from tests.model_utils import build_model, fill
    model = build_model("sigma_tiny", nc, 64, 96).cuda().eval()
    rgb, x, label = (t.cuda() for t in fill.make_inputs(1, 64, 96, nc, seed=5))
    min_kept = 64 * 96 // 4
    with torch.no_grad():
        logits = model(rgb, x)
    rows = logits.permute(0, 2, 3, 1).reshape(-1, nc).cpu()
    t = twin(rows, label.view(-1).cpu(), IGNORE, thresh, min_kept)
    assert t["mining"] and (t["threshold"] == thresh) == (nc == 9) and 0 < int(t["keep"].sum()) < int(t["valid"].sum())
    assert _gap_violations((rows.shape[0], nc, nc), rows, label.view(-1).cpu(), t) == 0, "a pixel within rounding of tau: change the input seed"

    def step(criterion, lab):
        model.criterion = criterion
        model.zero_grad(set_to_none=True)
        loss = model(rgb, x, lab)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}

    loss_o, grads_o = step(ProbOhemCrossEntropy2d(IGNORE, min_kept=min_kept, thresh=thresh), label)
    loss_c, grads_c = step(nn.CrossEntropyLoss(ignore_index=IGNORE), t["mined"].view_as(label).cuda())
    assert torch.isfinite(loss_o)
    bad = [n for n, g in grads_o.items() if not bool(torch.isfinite(g).all())]
    assert not bad, bad
    torch.testing.assert_close(loss_o.double().cpu(), t["loss"], rtol=1e-5, atol=0.0)
    torch.testing.assert_close(loss_o, loss_c, rtol=1e-5, atol=0.0)
    for n, a in grads_c.items():
        torch.testing.assert_close(grads_o[n], a, rtol=1e-4, atol=1e-6 + 1e-5 * float(a.abs().max()), msg=lambda m, n=n: f"{n}: {m}")


def test_ohem_step_under_the_deterministic_flag():
    """tests/ohem_deterministic_worker.py, in a child process (the flag stays out of this one): under
    torch.use_deterministic_algorithms(True) two training steps of sigma_tiny with the OHEM criterion from identical
    state are bitwise equal, on the kernel route (9 and 40 classes) and on the class's fallback, and nothing raises"""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    r = subprocess.run([sys.executable, "-m", "tests.ohem_deterministic_worker"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"worker exit {r.returncode}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    assert "[ohem_deterministic_worker] done" in r.stdout


def test_ohem_route_is_captured_into_a_graph():
    """loss + backward of the class (9 classes at pitch 12, weights) captured once by torch.cuda.graph and replayed on two
    inputs held in the captured buffers: one with so few labelled pixels that min_kept exceeds them (nothing is mined),
    one that is mined.  Each replay gives the bits of the eager run on the same input: the branch lives on the device."""
    from sigma_amd.pointwise import ohem_stages
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    nc, ld, B, H, W = 9, 12, 2, 9, 11
    min_kept = 60
    crit = ProbOhemCrossEntropy2d(IGNORE, "mean", 0.7, min_kept, weight=_weights_cpu(nc, seed=451).to(DEV))
    g = torch.Generator().manual_seed(452)
    data = []
    for few in (True, False):
        xs = torch.full((B, H, W, ld), float("nan"))
        xs[..., :nc] = torch.randn(B, H, W, nc, generator=g) * 3.0
        lab = torch.randint(0, nc, (B, H, W), generator=g)
        lab[torch.rand(B, H, W, generator=g) < (0.8 if few else 0.1)] = IGNORE
        assert (int((lab != IGNORE).sum()) < min_kept) == few
        data.append((xs.to(DEV), lab.to(DEV)))
    buf = data[0][0].clone().requires_grad_()
    label = data[0][1].clone()

    def step():
        loss = crit(buf[..., :nc].permute(0, 3, 1, 2), label)
        (grad,) = torch.autograd.grad(loss * 1.7, buf)
        return loss.detach(), grad

    def load(i):
        with torch.no_grad():
            buf.copy_(data[i][0])
            label.copy_(data[i][1])

    eager = []
    for i in range(2):
        load(i)
        eager.append(tuple(t.clone() for t in step()))
        st = ohem_stages(buf.detach()[..., :nc].reshape(-1, nc), label.view(-1), None, IGNORE, ld, 0.7, min_kept)
        nv, kept = (int(v) for v in st["counts"].cpu())
        assert (kept == nv) == (i == 0) and (float(st["tau"]) == float("-inf")) == (i == 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    load(1)
    with torch.cuda.graph(graph):
        loss_g, grad_g = step()
    for i in (0, 1, 0):
        load(i)
        loss_g.zero_()
        grad_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(loss_g) and bool((grad_g[..., nc:] == 0).all())
        assert torch.equal(loss_g, eager[i][0]) and torch.equal(grad_g, eager[i][1]), f"replay on input {i} differs from eager"
