"""The region-overlap losses without a GPU: the torch formulation of ``RegionLoss2d`` against the fp64 twin, an fp32
emulation of the kernels of csrc/region.hip under the derived bounds (tests/region_loss_bounds.py) and the twin's wrong
variants outside them, the identities between the kinds, every refusal of include/sigma_region.h (host only: no kernel is
reached), the layout of its struct, and the constructor's checks."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

from sigma_amd import _capi, _capi_region
from sigma_amd.utils.loss_opr import RegionLoss2d
from tests import region_loss_bounds as rb
from tests.capi_refusals import assert_refused
from tests.region_loss_twin import KINDS, VARIANTS, formula_gradient, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = rb.IGNORE

# (rows, classes, ld): every class count and pitch of the GPU test at a ragged row count, the threshold row counts at the
# smallest class count, and the row count of the second grid-stride trip
EMU_CASES = [(257, nc, ld) for nc, ld in rb.CLASS_CASES] + [(r, 5, 8) for r in rb.ROW_COUNTS] + [(rb.BIG_ROWS, 5, 8)]


@functools.lru_cache(maxsize=None)
def _case(rows, nc, ld, pi):
    kind, s, rw, cw, G = rb.PARAM_CASES[pi]
    a, b = rb.ab_of(kind)
    buf, lab = rb.region_inputs(rows, nc, ld, seed=rows + nc)
    t = rb.bounds(buf[:, :nc].double(), lab, nc, a, b, s, rw, cw, G)
    return buf, lab, (a, b, s, rw, cw, G), t


@pytest.mark.parametrize("kind", ["dice", "jaccard", "tversky"])
def test_torch_formulation_matches_the_twin(kind):
    """loss and gradient in fp64, with ignored pixels, labels outside [0, classes) and a class that is never a label"""
    B, nc, H, W = 2, 6, 7, 9
    buf, lab = rb.region_inputs(B * H * W, nc, nc, seed=3, masked=False)
    ab = dict(alpha=0.3, beta=0.7) if kind == "tversky" else {}
    a, b = (0.3, 0.7) if kind == "tversky" else KINDS[kind]
    for s, cw in ((0.0, 0.0), (1.0, 0.5)):
        crit = RegionLoss2d(kind, ignore_index=IGNORE, smooth=s, ce_weight=cw, region_weight=0.75, **ab)
        x = buf.double().view(B, H, W, nc).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        loss = crit(x, lab.view(B, H, W))
        loss.backward()
        t = twin(buf.double(), lab, IGNORE, a, b, s, 0.75, cw)
        assert float(t["sums"][2][nc - 1]) == 0.0 and int(t["kcount"]) == nc - 1          # the absent class is outside K
        assert abs(float(loss.detach()) - float(t["loss"])) <= 1e-12 * max(1.0, abs(float(t["loss"])))
        got = x.grad.permute(0, 2, 3, 1).reshape(-1, nc)
        assert float((got - t["dl"]).abs().max()) <= 1e-12 * max(1.0, float(t["dl"].abs().max()))
        assert float((formula_gradient(t) - t["dl"]).abs().max()) <= 1e-12        # the issue's gradient is the autograd one


def test_torch_formulation_with_nothing_labelled_is_zero():
    x = torch.randn(1, 4, 3, 3, dtype=torch.float64, requires_grad=True)
    loss = RegionLoss2d("dice", ce_weight=1.0)(x, torch.full((1, 3, 3), 255))
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(x.grad.abs().max()) == 0.0


def test_dice_and_jaccard_are_tversky():
    buf, lab = rb.region_inputs(300, 9, 9, seed=1)
    x = buf.double()
    for kind, ab in KINDS.items():
        assert ab == {"dice": (0.5, 0.5), "jaccard": (1.0, 1.0)}[kind]
        t = twin(x, lab, IGNORE, *ab, s=0.25, cw=0.5)
        # Dice = 2 I / (P + Y) and Jaccard = I / (P + Y - I), written out with the smoothing term
        I, P, Y = t["sums"]
        idx = (I + 0.25) / (0.5 * (P + Y) + 0.25) if kind == "dice" else (I + 0.25) / (P + Y - I + 0.25)
        present = Y > 0
        assert float((t["T"][present] - idx[present]).abs().max()) <= 1e-14
        crit_t = RegionLoss2d("tversky", alpha=ab[0], beta=ab[1], smooth=0.25, ce_weight=0.5)
        crit_k = RegionLoss2d(kind, smooth=0.25, ce_weight=0.5)
        xi = x.view(3, 10, 10, 9).permute(0, 3, 1, 2)
        assert float(crit_t(xi, lab.view(3, 10, 10))) == float(crit_k(xi, lab.view(3, 10, 10)))


@pytest.mark.parametrize("pi", range(len(rb.PARAM_CASES)))
@pytest.mark.parametrize("rows,nc,ld", EMU_CASES, ids=[f"{r}x{c}@{l}" for r, c, l in EMU_CASES])
def test_fp32_emulation_stays_under_the_bounds(rows, nc, ld, pi):
    buf, lab, (a, b, s, rw, cw, G), t = _case(rows, nc, ld, pi)
    out = rb.emulate(buf, lab, nc, a, b, s, rw, cw, G)
    rs = rb.worst_ratio(out, t, nc)
    rs["lse"] = rb.ratio(out["lse"], t["lse"], t["S_lse"])
    rs["coef"] = rb.ratio(out["coef"], torch.cat([t["A"], t["B"], torch.as_tensor(t["cwn"]).reshape(1)]), t["S_coef"])
    print(rows, nc, ld, pi, {k: round(v, 4) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), rs
    assert not out["dl"][:, nc:].any() and not out["dl"][~t["valid"].numpy()].any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_each_wrong_variant_exceeds_the_bounds(variant):
    """on the inputs of the emulation test: the right kernels (their emulation) held against a wrong twin fail at least one
    bound on at least one input, and where they do the margin is not marginal"""
    worst = 0.0
    for rows, nc, ld in [(257, 5, 8), (257, 9, 12), (257, 40, 40)]:
        for pi in range(len(rb.PARAM_CASES)):
            buf, lab, (a, b, s, rw, cw, G), t = _case(rows, nc, ld, pi)
            wrong = dict(t)
            w = twin(buf[:, :nc].double(), lab, IGNORE, a, b, s, rw, cw, upstream=G, variant=variant)
            wrong.update({k: w[k] for k in ("loss", "region", "ce", "sums", "dl")})
            out = rb.emulate(buf, lab, nc, a, b, s, rw, cw, G)
            worst = max(worst, max(rb.worst_ratio(out, wrong, nc).values()))
    print(variant, worst)
    assert worst > 10.0, (variant, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI of include/sigma_region.h

def _p(**kw):
    good = dict(rows=8, classes=9, ld=12, ignore_index=255, alpha=0.5, beta=0.5, smooth=0.0, region_weight=1.0, ce_weight=0.0,
                logits=0x10000, labels=0x20000, lse=0x30000, workspace=0x40000, workspace_bytes=1 << 20, loss=0x50000,
                terms=0x50010, coef=0x60000, sums=0x70000, scale=0x80000, dlogits=0x90000)
    p = _capi_region.RegionParams()
    for k, v in dict(good, **kw).items():
        setattr(p, k, v)
    return ctypes.byref(p)


NAN = float("nan")
# what all three entry points refuse on the values: (field values, the text names)
VALUE_REFUSALS = [(dict(classes=0), "classes"), (dict(classes=65, ld=68), "classes"), (dict(ld=10), "ld"), (dict(ld=8), "ld"),
                  (dict(rows=-1), "rows"), (dict(beta=0.0), "beta"), (dict(beta=-0.5), "beta"), (dict(beta=NAN), "beta"),
                  (dict(alpha=-0.1), "alpha"), (dict(alpha=NAN), "alpha"), (dict(smooth=-1.0), "smooth"), (dict(smooth=NAN), "smooth"),
                  (dict(region_weight=-1.0), "region_weight"), (dict(region_weight=NAN), "region_weight"),
                  (dict(ce_weight=-0.5), "ce_weight"), (dict(ce_weight=NAN), "ce_weight")]
FWD_REFUSALS = [(dict(logits=None), "logits"), (dict(labels=None), "labels"), (dict(lse=None), "lse"), (dict(coef=None), "coef"),
                (dict(loss=None), "loss"), (dict(terms=None), "terms"), (dict(sums=None), "sums"), (dict(workspace=None), "workspace"),
                (dict(workspace_bytes=1024 * 29 * 4 - 1), "workspace"), (dict(logits=0x10004), "logits"), (dict(labels=0x20004), "labels"),
                (dict(lse=0x30002), "lse"), (dict(sums=0x70001), "sums"), (dict(workspace=0x40002), "workspace")]
BWD_REFUSALS = [(dict(logits=None), "logits"), (dict(labels=None), "labels"), (dict(lse=None), "lse"), (dict(coef=None), "coef"),
                (dict(scale=None), "scale"), (dict(dlogits=None), "dlogits"), (dict(dlogits=0x90008), "dlogits"),
                (dict(logits=0x10008), "logits"), (dict(scale=0x80002), "scale"), (dict(coef=0x60002), "coef")]


def test_the_binding_covers_the_header():
    text = open(os.path.join(ROOT, "include", "sigma_region.h")).read()
    declared = set(re.findall(r"^\w+ (sigma_\w+)\(", text, flags=re.M))
    assert declared == set(_capi_region.SIGNATURES) == set(_capi_region.REGION_SYMBOLS)
    assert not declared & set(_capi.SIGNATURES) and not set(_capi_region.STRUCTS) & set(_capi.STRUCTS)
    lib = _capi_region.load()
    for name, (restype, argtypes) in _capi_region.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    ops = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    assert int(re.search(r"#define SIGMA_CE_BLOCKS (\d+)", ops).group(1)) == rb.SIGMA_CE_BLOCKS


def test_struct_layout_matches_the_compiler(tmp_path):
    cls = _capi_region.RegionParams
    lines = [f'printf("%zu\\n", sizeof(sigma_region_params));']
    lines += [f'printf("%zu\\n", offsetof(sigma_region_params, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_region.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]


@pytest.mark.parametrize("name", ["sigma_region_loss_fwd", "sigma_region_loss_bwd"])
def test_every_refusal_names_the_field(name):
    fn = getattr(_capi_region.load(), name)
    assert_refused(fn, None, None, says="NULL", msg=name)
    for kw, says in VALUE_REFUSALS + (FWD_REFUSALS if name.endswith("fwd") else BWD_REFUSALS):
        text = assert_refused(fn, _p(**kw), None, says=says, msg=(name, kw))
        assert name not in text and name[len("sigma_"):] not in text
    # no rows: the row pointers are not looked at, and the backward launches nothing
    if name.endswith("bwd"):
        assert fn(_p(rows=0, logits=None, labels=None, lse=None, dlogits=None), None) == 0


def test_workspace_query():
    fn = _capi_region.load().sigma_region_loss_workspace_bytes
    assert_refused(fn, None, code=-1, says="NULL")
    for kw, says in VALUE_REFUSALS:
        assert_refused(fn, _p(**kw), code=-1, says=says, msg=kw)
    for nc in (1, 5, 40, 64):      # pointers are not looked at
        assert fn(_p(classes=nc, ld=64, logits=None, workspace=None)) == rb.SIGMA_CE_BLOCKS * (3 * nc + 2) * 4


def test_constructor_rejects_bad_arguments():
    for kw in (dict(kind="iou"), dict(kind="tversky"), dict(kind="tversky", alpha=0.3), dict(kind="tversky", alpha=-0.1, beta=0.5),
               dict(kind="tversky", alpha=0.5, beta=0.0), dict(kind="tversky", alpha=0.5, beta=NAN), dict(kind="dice", alpha=0.5),
               dict(kind="jaccard", beta=1.0), dict(smooth=-1.0), dict(smooth=NAN), dict(ce_weight=-1.0), dict(region_weight=NAN)):
        with pytest.raises(ValueError):
            RegionLoss2d(**kw)
    c = RegionLoss2d("tversky", alpha=0.3, beta=0.7, smooth=1.0, ce_weight=0.5)
    assert (c.alpha, c.beta, c.smooth, c.ce_weight, c.region_weight, c.ignore_index, c.last_terms) == (0.3, 0.7, 1.0, 0.5, 1.0, 255, None)
    assert (RegionLoss2d().alpha, RegionLoss2d().beta) == (0.5, 0.5) and (RegionLoss2d("jaccard").alpha, RegionLoss2d("jaccard").beta) == (1.0, 1.0)
