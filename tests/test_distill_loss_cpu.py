"""The distillation loss without a GPU: the fp64 twin against an independent anchor (F.kl_div), the torch formulation of
``DistillLoss2d`` against the twin, an fp32 emulation of the kernels of csrc/distill.hip under the derived bounds
(tests/distill_loss_bounds.py) on every input of the GPU test and the twin's wrong variants outside them, every refusal of
include/sigma_distill.h (host only: no kernel is reached), the layout of its struct, the constructor's checks, and
``EncoderDecoder.attach_teacher`` on CPU models."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from sigma_amd import _capi, _capi_distill
from sigma_amd.utils.loss_opr import DistillLoss2d
from tests import distill_loss_bounds as db
from tests.capi_refusals import assert_refused
from tests.distill_loss_twin import VARIANTS, formula_gradient, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = db.IGNORE


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0, 4.0])
def test_twin_matches_kl_div(T):
    """no ignored rows, no cross-entropy term: the twin is F.kl_div(..., "batchmean") T^2 on the (rows, classes) matrix"""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(301, 7, generator=g, dtype=torch.float64) * 3.0
    t64 = torch.randn(301, 7, generator=g, dtype=torch.float64) * 3.0
    lab = torch.randint(0, 7, (301,), generator=g)
    t = twin(x, t64, lab, IGNORE, T, 1.0, 0.0)
    leaf = x.clone().requires_grad_(True)
    anchor = F.kl_div(F.log_softmax(leaf / T, dim=1), F.softmax(t64 / T, dim=1), reduction="batchmean") * T * T
    anchor.backward()
    anchor = anchor.detach()
    assert abs(float(t["loss"]) - float(anchor)) <= 1e-12 * abs(float(anchor)) and float(anchor) > 0
    assert float((t["dl"] - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
    assert float((formula_gradient(t) - t["dl"]).abs().max()) <= 1e-12 * float(t["dl"].abs().max())


@pytest.mark.parametrize("kd_all", [False, True])
def test_torch_formulation_matches_the_twin(kd_all):
    """loss and gradient in fp64, with ignored pixels and labels outside [0, classes); the teacher gets no gradient"""
    B, nc, H, W = 2, 6, 7, 9
    buf, tbuf, lab = db.distill_inputs(B * H * W, nc, nc, nc, seed=3)
    nchw = lambda b: b.double().view(B, H, W, nc).permute(0, 3, 1, 2).contiguous()
    for T, kw, cw in ((1.0, 1.0, 0.0), (2.0, 0.7, 0.5), (0.5, 0.0, 1.0)):
        crit = DistillLoss2d(T, kw, cw, ignore_index=IGNORE, kd_all=kd_all)
        x, te = nchw(buf).requires_grad_(True), nchw(tbuf).requires_grad_(True)
        loss = crit(x, lab.view(B, H, W), te)
        loss.backward()
        t = twin(buf.double(), tbuf.double(), lab, IGNORE, T, kw, cw, kd_all)
        assert abs(float(loss.detach()) - float(t["loss"])) <= 1e-12 * max(1.0, abs(float(t["loss"])))
        got = x.grad.permute(0, 2, 3, 1).reshape(-1, nc)
        assert float((got - t["dl"]).abs().max()) <= 1e-12 * max(1.0, float(t["dl"].abs().max()))
        assert float((formula_gradient(t) - t["dl"]).abs().max()) <= 1e-12        # the issue's gradient is the autograd one
        assert te.grad is None and crit.last_terms is None


def test_torch_formulation_edge_cases():
    """nothing labelled: loss and gradient 0 without kd_all, the KD term alone with it; a -inf teacher logit contributes 0"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    te = torch.randn(1, 4, 3, 3, generator=g, dtype=torch.float64)
    nothing = torch.full((1, 3, 3), 255)
    loss = DistillLoss2d(2.0, 1.0, 1.0)(x, nothing, te)
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(x.grad.abs().max()) == 0.0
    x.grad = None
    loss = DistillLoss2d(2.0, 1.0, 1.0, kd_all=True)(x, nothing, te)
    loss.backward()
    rows = lambda v: v.detach().permute(0, 2, 3, 1).reshape(-1, 4)
    t = twin(rows(x), rows(te), nothing.view(-1), 255, 2.0, 1.0, 1.0, True)
    assert float(t["ce"]) == 0.0 and float(t["kd"]) > 0 and abs(float(loss.detach()) - float(t["loss"])) <= 1e-12
    assert float((rows(x.grad) - t["dl"]).abs().max()) <= 1e-12
    te2 = te.clone()
    te2[:, 1] = float("-inf")
    x.grad = None
    loss = DistillLoss2d(2.0)(x, torch.zeros(1, 3, 3, dtype=torch.long), te2)
    loss.backward()
    assert bool(torch.isfinite(loss.detach())) and bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------------------------------------------------------------
# the emulation of the kernels under the bounds, on the inputs of tests/test_distill_loss_gpu.py

# (rows, classes, ld, ld_t, params): every class count and pitch at a ragged row count with every parameter set, the
# threshold row counts at one class count, and the row count of the second grid-stride trip
EMU_CASES = ([(257, nc, ld, ldt, pi) for nc, ld, ldt in db.CLASS_CASES for pi in range(len(db.PARAM_CASES))]
             + [(r, 5, 8, 12, 1) for r in db.ROW_COUNTS] + [(db.BIG_ROWS, *db.BIG_CASE, 2)])


@functools.lru_cache(maxsize=None)
def _case(rows, nc, ld, ldt):
    return db.distill_inputs(rows, nc, ld, ldt, seed=rows + nc)


def _held(buf, tbuf, lab, nc, par, what):
    T, kw, cw, kd_all, G = par
    t = db.bounds(buf[:, :nc].double(), tbuf[:, :nc].double(), lab, nc, T, kw, cw, kd_all, G)
    out = db.emulate(buf, tbuf, lab, nc, T, kw, cw, kd_all, G)
    rs = db.worst_ratio(out, t, nc)
    print(what, {k: round(v, 4) for k, v in rs.items()})
    assert all(v <= 1.0 for v in rs.values()), (what, rs)
    outside = ~(t["in_s"] | t["valid"]).numpy()
    assert not out["dl"][:, nc:].any() and not out["dl"][outside].any()
    return out, t


@pytest.mark.parametrize("rows,nc,ld,ldt,pi", EMU_CASES, ids=[f"{r}x{c}@{l}@{lt}-p{pi}" for r, c, l, lt, pi in EMU_CASES])
def test_fp32_emulation_stays_under_the_bounds(rows, nc, ld, ldt, pi):
    buf, tbuf, lab = _case(rows, nc, ld, ldt)
    _held(buf, tbuf, lab, nc, db.PARAM_CASES[pi], f"{rows}x{nc}@{ld}@{ldt} params {pi}")


@pytest.mark.parametrize("rows,nc,ld,ldt", db.REGIME_CASES, ids=[f"{r}x{c}@{l}@{lt}" for r, c, l, lt in db.REGIME_CASES])
@pytest.mark.parametrize("regime", db.UNMASKED_REGIMES + db.MASK_KINDS)
def test_fp32_emulation_stays_under_the_bounds_on_the_regimes(regime, rows, nc, ld, ldt):
    pair = db.masked_pair if regime in db.MASK_KINDS else db.regime_pair
    buf, tbuf, lab = pair(regime, rows, nc, ld, ldt, seed=700 + nc)
    for par in db.REGIME_PARAMS:
        out, t = _held(buf, tbuf, lab, nc, par, f"{regime} {rows}x{nc} T {par[0]}")
        if regime in db.MASK_KINDS:
            masked = torch.isinf(tbuf[:, :nc])
            assert bool(masked.any()) and not t["q"][masked].any()


def test_student_only_mask_gives_an_infinite_loss_and_a_finite_gradient():
    buf, tbuf, lab = db.masked_pair("student", 300, 9, 12, 12, seed=709)
    out = db.emulate(buf, tbuf, lab, 9, 2.0, 1.0, 0.5, False, 1.0)
    t = twin(buf[:, :9].double(), tbuf[:, :9].double(), lab, IGNORE, 2.0, 1.0, 0.5)
    assert float(out["loss"]) == float("inf") == float(t["loss"]) and float(out["terms"][0]) == float("inf")
    assert bool(torch.isfinite(t["dl"]).all()) and bool(torch.isfinite(torch.as_tensor(out["dl"])).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_each_wrong_variant_exceeds_the_bounds(variant):
    """on the inputs of the emulation test: the right kernels (their emulation) held against a wrong twin fail at least one
    bound on at least one input, and where they do the margin is not marginal"""
    worst = 0.0
    for rows, nc, ld, ldt in [(257, 5, 8, 12), (257, 9, 12, 12), (257, 40, 40, 44)]:
        for pi in (1, 2):                                     # T = 2 and T = 4 with a cross-entropy term
            T, kw, cw, kd_all, G = db.PARAM_CASES[pi]
            buf, tbuf, lab = _case(rows, nc, ld, ldt)
            x64, t64 = buf[:, :nc].double(), tbuf[:, :nc].double()
            wrong = db.bounds(x64, t64, lab, nc, T, kw, cw, kd_all, G)
            w = twin(x64, t64, lab, IGNORE, T, kw, cw, kd_all, upstream=G, variant=variant)
            wrong.update({k: w[k] for k in ("loss", "kd", "ce", "dl")})
            out = db.emulate(buf, tbuf, lab, nc, T, kw, cw, kd_all, G)
            worst = max(worst, max(db.worst_ratio(out, wrong, nc).values()))
    print(variant, worst)
    assert worst > 10.0, (variant, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI of include/sigma_distill.h

def _p(**kw):
    good = dict(rows=8, classes=9, ld=12, ld_t=16, kd_all=0, ignore_index=255, temperature=2.0, kd_weight=1.0, ce_weight=0.0,
                logits=0x10000, teacher=0x18000, labels=0x20000, lse=0x30000, workspace=0x40000, workspace_bytes=1 << 20,
                loss=0x50000, terms=0x50010, coef=0x60000, scale=0x80000, dlogits=0x90000)
    p = _capi_distill.DistillParams()
    for k, v in dict(good, **kw).items():
        setattr(p, k, v)
    return ctypes.byref(p)


NAN = float("nan")
# what all three entry points refuse on the values: (field values, the text names)
VALUE_REFUSALS = [(dict(classes=0), "classes"), (dict(classes=65, ld=68, ld_t=68), "classes"), (dict(ld=10), "ld"), (dict(ld=8), "ld"),
                  (dict(ld_t=10), "ld_t"), (dict(ld_t=8), "ld_t"), (dict(rows=-1), "rows"), (dict(temperature=0.0), "temperature"),
                  (dict(temperature=-1.0), "temperature"), (dict(temperature=NAN), "temperature"),
                  (dict(kd_weight=-1.0), "kd_weight"), (dict(kd_weight=NAN), "kd_weight"),
                  (dict(ce_weight=-0.5), "ce_weight"), (dict(ce_weight=NAN), "ce_weight")]
FWD_REFUSALS = [(dict(logits=None), "logits"), (dict(teacher=None), "teacher"), (dict(labels=None), "labels"), (dict(lse=None), "lse"),
                (dict(coef=None), "coef"), (dict(loss=None), "loss"), (dict(terms=None), "terms"), (dict(workspace=None), "workspace"),
                (dict(workspace_bytes=1024 * 4 * 4 - 1), "workspace"), (dict(logits=0x10004), "logits"), (dict(teacher=0x18008), "teacher"),
                (dict(labels=0x20004), "labels"), (dict(lse=0x30002), "lse"), (dict(loss=0x50001), "loss"), (dict(terms=0x50012), "terms"),
                (dict(coef=0x60002), "coef"), (dict(workspace=0x40002), "workspace")]
BWD_REFUSALS = [(dict(logits=None), "logits"), (dict(teacher=None), "teacher"), (dict(labels=None), "labels"), (dict(lse=None), "lse"),
                (dict(coef=None), "coef"), (dict(scale=None), "scale"), (dict(dlogits=None), "dlogits"), (dict(dlogits=0x90008), "dlogits"),
                (dict(logits=0x10008), "logits"), (dict(teacher=0x18004), "teacher"), (dict(scale=0x80002), "scale"),
                (dict(coef=0x60002), "coef")]


def test_the_binding_covers_the_header():
    text = open(os.path.join(ROOT, "include", "sigma_distill.h")).read()
    declared = set(re.findall(r"^\w+ (sigma_\w+)\(", text, flags=re.M))
    assert declared == set(_capi_distill.SIGNATURES) == set(_capi_distill.DISTILL_SYMBOLS) and len(declared) == 3
    assert not declared & set(_capi.SIGNATURES) and not set(_capi_distill.STRUCTS) & set(_capi.STRUCTS)
    lib = _capi_distill.load()
    for name, (restype, argtypes) in _capi_distill.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    fields = re.search(r"typedef struct sigma_distill_params \{(.*?)\} sigma_distill_params;", text, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    types = {"const", "float", "double", "void", "int32_t", "int64_t"}
    names = [n for n in re.findall(r"\w+", fields) if n not in types]
    assert names == [n for n, _ in _capi_distill.DistillParams._fields_]
    ops = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    assert int(re.search(r"#define SIGMA_CE_BLOCKS (\d+)", ops).group(1)) == db.SIGMA_CE_BLOCKS


def test_struct_layout_matches_the_compiler(tmp_path):
    cls = _capi_distill.DistillParams
    lines = ['printf("%zu\\n", sizeof(sigma_distill_params));']
    lines += [f'printf("%zu\\n", offsetof(sigma_distill_params, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_distill.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]


@pytest.mark.parametrize("name", ["sigma_distill_loss_fwd", "sigma_distill_loss_bwd"])
def test_every_refusal_names_the_field(name):
    fn = getattr(_capi_distill.load(), name)
    assert_refused(fn, None, None, says="NULL", msg=name)
    for kw, says in VALUE_REFUSALS + (FWD_REFUSALS if name.endswith("fwd") else BWD_REFUSALS):
        text = assert_refused(fn, _p(**kw), None, says=says, msg=(name, kw))
        assert name not in text and name[len("sigma_"):] not in text
        if says in ("ld", "ld_t"):
            assert re.search(rf"\b{says}\b", text), (kw, text)          # "ld" alone would also match "ld_t"
    # no rows: the row pointers are not looked at, and the backward launches nothing
    if name.endswith("bwd"):
        assert fn(_p(rows=0, logits=None, teacher=None, labels=None, lse=None, dlogits=None), None) == 0


def test_workspace_query():
    fn = _capi_distill.load().sigma_distill_loss_workspace_bytes
    assert_refused(fn, None, code=-1, says="NULL")
    for kw, says in VALUE_REFUSALS:
        assert_refused(fn, _p(**kw), code=-1, says=says, msg=kw)
    for nc in (1, 5, 40, 64):      # pointers are not looked at
        assert fn(_p(classes=nc, ld=64, ld_t=68, logits=None, teacher=None, workspace=None)) == db.SIGMA_CE_BLOCKS * 4 * 4


def test_constructor_rejects_bad_arguments():
    for kw in (dict(temperature=0.0), dict(temperature=-2.0), dict(temperature=NAN), dict(temperature=float("inf")),
               dict(kd_weight=-1.0), dict(kd_weight=NAN), dict(ce_weight=-0.1), dict(ce_weight=NAN)):
        with pytest.raises(ValueError):
            DistillLoss2d(**kw)
    c = DistillLoss2d(4.0, 0.5, 0.25, ignore_index=7, kd_all=True)
    assert (c.temperature, c.kd_weight, c.ce_weight, c.ignore_index, c.kd_all, c.last_terms) == (4.0, 0.5, 0.25, 7, True, None)
    d = DistillLoss2d()
    assert (d.temperature, d.kd_weight, d.ce_weight, d.ignore_index, d.kd_all) == (1.0, 1.0, 0.0, 255, False)
    assert not list(d.parameters()) and not list(d.buffers())


# ---------------------------------------------------------------------------------------------------------------------
# the model hook

def test_attach_teacher_on_cpu_models():
    from tests.deepsup_utils import build_ds_model
    from tests.model_utils import build_model
    student, teacher = build_model("sigma_tiny", 9, 64, 96), build_model("sigma_tiny", 9, 64, 96)
    names = [n for n, _ in student.named_parameters()]
    keys = list(student.state_dict())
    modules = [n for n, _ in student.named_modules()]
    teacher.train()
    crit = DistillLoss2d(2.0, 1.0, 0.5)
    student.attach_teacher(teacher, crit)
    assert [n for n, _ in student.named_parameters()] == names and list(student.state_dict()) == keys
    assert [n for n, _ in student.named_modules()] == modules
    inside = {id(m) for m in student.modules()}
    assert id(teacher) not in inside and id(crit) not in inside and not any(id(m) in inside for m in teacher.modules())
    mine = {id(p) for p in student.parameters()}
    assert not any(id(p) in mine for p in teacher.parameters())
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    assert all(p.requires_grad for p in student.parameters())
    student.train()
    assert student.training and not teacher.training and not any(m.training for m in teacher.modules())
    student.double()                                          # to() and its kin do not reach the teacher
    assert next(teacher.parameters()).dtype == torch.float32
    student.float()
    student.detach_teacher()
    assert student._distill is None and [n for n, _ in student.named_modules()] == modules
    with pytest.raises(ValueError, match="classes"):
        student.attach_teacher(build_model("sigma_tiny", 5, 64, 96), crit)
    with pytest.raises(ValueError, match="on meta"):
        student.attach_teacher(build_model("sigma_tiny", 9, 64, 96).to("meta"), crit)
    with pytest.raises(ValueError, match="deep_supervision"):
        build_ds_model(9, 64, 96).attach_teacher(teacher, crit)
    assert student._distill is None
