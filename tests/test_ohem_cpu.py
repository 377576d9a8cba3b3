"""ProbOhemCrossEntropy2d without a GPU: the fp64 twin (tests/ohem_fp64_twin.py) against the reference's own output
(tests/golden/loss_ohem.npz, made by tests/golden/make_golden_ohem.py), the class's torch fallback against the twin, and
the host side of sigma_ohem_select / sigma_ohem_workspace_bytes (include/sigma_ops.h).

Bound (as ``check`` of tests/test_stream_fp64_gpu.py, in fp64): |got - ref| <= 64 x 2^-53 x S with S the summed magnitudes
of the terms: for the loss sum_r w_y (|lse| + |x_y|), divided by the denominator for 'mean'; for the gradient
|g| w_y (p_c (|x_c| + |lse| + 1) + [c == y]).  The kept set must be identical: the kept rows of the fixture are those
with a non-zero gradient (no fixture weight is zero, and no softmax row equals its one-hot row).

Which fixture cases each wrong variant of the twin fails (asserted below):
  exact_k    thresh_governs (110 pixels are under thresh, 8 would be kept), kth_governs_tie (71 kept, 70 would be)
  strict     kth_governs and kth_governs_tie (the pixels AT the k-th value are dropped)
  den_valid  thresh_governs, weighted_mean (and every other case that drops a pixel or has weights)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from sigma_amd import _capi
from tests.capi_refusals import assert_refused
from tests.ohem_fp64_twin import VARIANTS, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = 255
U64 = 2.0 ** -53
K64 = 64
EXPECTED_FAILURES = {"exact_k": {"thresh_governs", "kth_governs_tie"}, "strict": {"kth_governs", "kth_governs_tie"},
                     "den_valid": {"thresh_governs", "weighted_mean"}}


def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "loss_ohem.npz"))
    cases = {}
    for name in [str(n) for n in z["cases"]]:
        w = z[f"{name}.weight"]
        cases[name] = dict(x=torch.from_numpy(z[f"{name}.x"]), target=torch.from_numpy(z[f"{name}.target"]),
                           thresh=float(z[f"{name}.thresh"]), min_kept=int(z[f"{name}.min_kept"]), reduction=str(z[f"{name}.reduction"]),
                           weight=torch.from_numpy(w) if w.size else None, loss=torch.from_numpy(z[f"{name}.loss"]),
                           grad=torch.from_numpy(z[f"{name}.grad"]))
    return cases


FIXTURE = _fixture()
BRANCHES = ("thresh_governs", "kth_governs", "kth_governs_tie", "more_than_valid", "equal_valid", "zero_min_kept", "no_valid",
            "weighted_mean", "sum")


def _rows(c):
    x = c["x"]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]), c["target"].reshape(-1)


def _agrees(c, t, loss, grad_rows):
    """None when (loss, gradient rows, kept set) agree with the twin's result `t` under the bound, else what differs"""
    kept = grad_rows.abs().sum(1) != 0
    if not torch.equal(kept, t["keep"]):
        return f"kept set: {int(kept.sum())} against {int(t['keep'].sum())}"
    S_rows = t["wy"] * (t["lse"].abs() + t["xy"].abs())
    S_loss = S_rows.sum() / (t["den"] if c["reduction"] == "mean" and t["den"] else 1.0)
    want = t["loss"]
    if bool(torch.isnan(want).any()) or bool(torch.isnan(loss).any()):
        if not (bool(torch.isnan(want).all()) and bool(torch.isnan(loss).all())):
            return "NaN on one side only"
    elif float((loss - want).abs().max()) > K64 * U64 * float(S_loss):
        return f"loss: {float(loss)} against {float(want)}"
    x, _ = _rows(c)
    S_dl = (t["gr"].abs() * t["wy"])[:, None] * (t["sm"] * (x.abs() + t["lse"].abs()[:, None] + 1.0) + t["oh"])
    bad = (grad_rows - t["dl"]).abs() > K64 * U64 * S_dl
    if bool(bad.any()):
        return f"gradient: {int(bad.sum())} elements outside the bound"
    return None


def _twin_of(c, variant=None):
    x, lab = _rows(c)
    return twin(x, lab, IGNORE, c["thresh"], c["min_kept"], weight=c["weight"], reduction=c["reduction"], variant=variant)


def test_fixture_covers_the_branches():
    assert set(FIXTURE) == set(BRANCHES)
    t = {n: _twin_of(c) for n, c in FIXTURE.items()}
    assert t["thresh_governs"]["mining"] and t["thresh_governs"]["threshold"] == FIXTURE["thresh_governs"]["thresh"]
    for n in ("kth_governs", "kth_governs_tie", "equal_valid"):
        assert t[n]["mining"] and t[n]["threshold"] > FIXTURE[n]["thresh"], n
    assert int(t["kth_governs"]["keep"].sum()) == FIXTURE["kth_governs"]["min_kept"]
    assert int(t["kth_governs_tie"]["keep"].sum()) == FIXTURE["kth_governs_tie"]["min_kept"] + 1
    assert int(t["equal_valid"]["valid"].sum()) == FIXTURE["equal_valid"]["min_kept"]
    for n in ("more_than_valid", "zero_min_kept", "no_valid"):
        assert not t[n]["mining"] and torch.equal(t[n]["keep"], t[n]["valid"]), n
    assert int(t["more_than_valid"]["valid"].sum()) + 1 == FIXTURE["more_than_valid"]["min_kept"]
    assert int(t["no_valid"]["valid"].sum()) == 0 and FIXTURE["zero_min_kept"]["min_kept"] == 0
    # thresh is not applied when min_kept is 0: pixels above it stay
    assert bool((t["zero_min_kept"]["p"][t["zero_min_kept"]["valid"]] > FIXTURE["zero_min_kept"]["thresh"]).any())
    assert FIXTURE["weighted_mean"]["weight"] is not None and FIXTURE["sum"]["reduction"] == "sum"


@pytest.mark.parametrize("name", BRANCHES)
def test_twin_reproduces_the_reference(name):
    c = FIXTURE[name]
    grad_rows = c["grad"].permute(0, 2, 3, 1).reshape(-1, c["x"].shape[1])
    assert _agrees(c, _twin_of(c), c["loss"], grad_rows) is None
    if name == "no_valid":
        assert bool(torch.isnan(c["loss"])) and bool((c["grad"] == 0).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_variants_fail_the_fixture(variant):
    failed = set()
    for name, c in FIXTURE.items():
        grad_rows = c["grad"].permute(0, 2, 3, 1).reshape(-1, c["x"].shape[1])
        why = _agrees(c, _twin_of(c, variant), c["loss"], grad_rows)
        if why is not None:
            failed.add(name)
    assert EXPECTED_FAILURES[variant] <= failed, (variant, failed)


@pytest.mark.parametrize("name", BRANCHES)
def test_class_fallback_equals_the_twin(name):
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    c = FIXTURE[name]
    crit = ProbOhemCrossEntropy2d(IGNORE, c["reduction"], c["thresh"], c["min_kept"], weight=c["weight"])
    x = c["x"].clone().requires_grad_()
    loss = crit(x, c["target"])
    loss.backward()
    grad_rows = x.grad.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    assert _agrees(c, _twin_of(c), loss.detach(), grad_rows) is None
    assert torch.equal(crit.mined_labels(c["x"], c["target"]).reshape(-1), _twin_of(c)["mined"])


def test_class_fallback_none_reduction_and_deterministic_flag():
    """'none' returns (B, H, W) with zeros at dropped pixels; under the deterministic flag the fallback ends in
    pointwise.cross_entropy_deterministic and gives the same numbers"""
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    c = FIXTURE["kth_governs_tie"]
    x, lab = _rows(c)
    t = twin(x, lab, IGNORE, c["thresh"], c["min_kept"], reduction="none")
    rows = ProbOhemCrossEntropy2d(IGNORE, "none", c["thresh"], c["min_kept"])(c["x"], c["target"])
    assert tuple(rows.shape) == tuple(c["target"].shape)
    assert bool((rows.reshape(-1)[~t["keep"]] == 0).all())
    torch.testing.assert_close(rows.reshape(-1), t["loss"], rtol=1e-12, atol=1e-12)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        det = ProbOhemCrossEntropy2d(IGNORE, "mean", c["thresh"], c["min_kept"])(c["x"], c["target"])
    finally:
        torch.use_deterministic_algorithms(was)
    torch.testing.assert_close(det, c["loss"], rtol=1e-12, atol=0.0)


def test_signature_and_use_weight():
    import inspect
    from sigma_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    names = list(inspect.signature(ProbOhemCrossEntropy2d.__init__).parameters)
    assert names == ["self", "ignore_label", "reduction", "thresh", "min_kept", "down_ratio", "use_weight", "weight"]
    with pytest.raises(NotImplementedError, match="weight="):
        ProbOhemCrossEntropy2d(IGNORE, use_weight=True)
    crit = ProbOhemCrossEntropy2d(IGNORE, "mean", 0.7, 1000, 8)
    assert (crit.thresh, crit.min_kept, crit.down_ratio) == (0.7, 1000, 8)


def _ohem_params(**kw):
    p = _capi.OhemParams()
    p.rows, p.ignore_index, p.classes, p.thresh, p.min_kept = 100, IGNORE, 5, 0.7, 10
    # never dereferenced: every call below is refused before any launch (aligned non-null addresses)
    p.nll, p.labels, p.mined, p.tau, p.counts, p.workspace = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    p.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_select_refuses_bad_arguments_before_any_launch():
    lib = _capi.load()
    # every refusal is SIGMA_OPS_ERR_ARG (1) with a reason of its own in the error text
    refused = lambda p, **kw: assert_refused(lib.sigma_ohem_select, ctypes.byref(p), None, **kw)
    assert_refused(lib.sigma_ohem_select, None, None, says="NULL")
    for field in ("nll", "labels", "mined", "tau", "counts", "workspace"):
        refused(_ohem_params(**{field: None}), says=field, msg=field)
    for field, addr in (("nll", 0x10002), ("tau", 0x40001), ("labels", 0x20004), ("mined", 0x30004), ("counts", 0x50004),
                        ("workspace", 0x60008), ("weight", 0x70002), ("row_loss", 0x80002), ("partial", 0x90002)):
        refused(_ohem_params(**{field: addr}), says="align", msg=field)
    need = int(lib.sigma_ohem_workspace_bytes(100))
    refused(_ohem_params(workspace_bytes=need - 1), says="workspace")
    refused(_ohem_params(workspace_bytes=0), says="workspace")
    for th in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused(_ohem_params(thresh=th), says="thresh", msg=th)
    refused(_ohem_params(rows=-1), says="rows")
    refused(_ohem_params(rows=2 ** 31), says="rows")
    refused(_ohem_params(classes=0), says="classes")


def test_workspace_query():
    lib = _capi.load()
    last = 0
    for rows in (0, 1, 255, 256, 257, 131075, 2457600, 2 ** 31 - 1):
        b = int(lib.sigma_ohem_workspace_bytes(rows))
        assert b > 0 and b % 16 == 0 and b >= last, (rows, b)
        last = b
    assert_refused(lib.sigma_ohem_workspace_bytes, -1, code=-1, says="rows")
    assert_refused(lib.sigma_ohem_workspace_bytes, 2 ** 31, code=-1, says="rows")


def test_ohem_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of sigma_ohem_params from gcc against the ctypes mirror (the method of
    tests/test_capi_cpu.py::test_struct_layout_matches_header)"""
    cname, cls = "sigma_ohem_params", _capi.OhemParams
    lines = [f'printf("%s %zu\\n", "{cname}", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("%s.%s %zu\\n", "{cname}", "{fname}", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_ops.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    assert f"#define SIGMA_OHEM_HIST_BLOCKS {_capi.SIGMA_OHEM_HIST_BLOCKS}\n" in header
    assert "sigma_ohem_select" in _capi.OPS_SYMBOLS and "sigma_ohem_workspace_bytes" in _capi.OPS_AUX_SYMBOLS
