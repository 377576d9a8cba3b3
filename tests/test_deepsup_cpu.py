"""Deep supervision without a GPU: the fp64 twin against F.interpolate and against the reference's own output
(tests/golden/model_tiny_64x96_ds.npz), the fp32 emulation of the kernels inside the bounds the GPU test uses, the wrong
variants of the twin outside them, the product model's keys and size check, the C ABI's struct and argument checks, and
the count of the kernels csrc/deepsup.hip compiles to."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sigma_amd import _capi
from tests.capi_refusals import assert_refused
from tests.deepsup_bounds import CASE_IDS, CASES, U, bounds, deepsup_inputs, emulate_fp32
from tests.deepsup_fp64_twin import VARIANTS, twin, upsample
from tests.deepsup_utils import build_ds_model
from tests.model_utils import build_model, digest, fill, load_model_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,s", [(1, 4), (2, 16), (3, 2), (5, 8), (4, 1), (7, 3), (6, 32), (9, 5)])
def test_twin_interpolation_is_f_interpolate(n, s):
    """the written-out index formula against F.interpolate(align_corners=False) in fp64, odd and even sizes and scales"""
    g = torch.Generator().manual_seed(n * 100 + s)
    z = torch.randn(2, n, n + 2, 3, generator=g, dtype=torch.float64)
    ref = F.interpolate(z.permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert float((upsample(z, s) - ref).abs().max()) <= 1e-12


def test_twin_on_the_fixture_is_the_references_output():
    """The commuted order -- the 1x1 head on the coarse map, then the interpolation -- on the reference's own normed maps
    and weights gives the reference's aux logits and loss terms, to the fixture's own fp32 rounding:
        logits      32 u max |logit| of the head (5e-6 to 6.4e-6 on logits of scale 2.6 to 3.4; measured 8e-7 to 1.7e-6)
        digests     sums over N = 55296 logits of errors that are each below that and do not share a sign:
                    sqrt(N) times it (1.2e-3 to 1.5e-3 on sums of mass 3e4 to 4e4; measured 3e-5 to 6e-5)
        loss terms  8 u |term| (1.2e-6; measured at most 2e-7, the rounding of the stored fp32 value itself)
    Why these suffice: the reference interpolates C = 384 / 192 / 96 channels in fp32 and adds C products per logit; its
    rounding errors add up like a random walk, a few u of the logit scale, and a loss term is a mean of 6144 rows, each
    1-Lipschitz in its logits, in which they average out further.  The worst case over every summation order,
    (C + 4) u sum_k |w_k| |x^_k| per logit, is 5e-5 to 3e-4 and says nothing about the commuted order: it is printed next
    to the measured error and not asserted."""
    meta, z = load_model_golden("tiny_64x96_ds")
    nc = meta["num_classes"]
    label = torch.from_numpy(z["label"].astype(np.int64))
    for i, s in enumerate((16, 8, 4)):
        x = torch.from_numpy(z[f"coarse{i}"]).double()
        C = x.shape[-1]
        w = fill.value_for(f"decode_head.output_ds.{i}.weight", (nc, C, 1, 1)).view(nc, C).double()
        t = twin(x @ w.t(), label, s, 255)
        worst = (C + 4) * U * (upsample(x.abs(), s) @ w.abs().t())
        got = t["zhat"].permute(0, 3, 1, 2)
        ref = torch.from_numpy(z[f"aux{i}_s4"]).double()
        tol = 32 * U * float(ref.abs().max())
        err = (got[:, :, ::4, ::4] - ref).abs()
        print(f"head {i}: logits max err {float(err.max()):.3e} tol {tol:.3e} (worst case {float(worst.max()):.3e}) scale {float(ref.abs().max()):.2f}")
        assert float(err.max()) <= tol
        d, dref = digest(got), z[f"aux{i}_digest"]
        dtol = got.numel() ** 0.5 * tol
        print(f"head {i}: digest diff {abs(d - dref).max():.3e} tol {dtol:.3e}")
        assert all(abs(d[k] - dref[k]) <= dtol for k in range(3))
        term = float(z["terms"][1 + i])
        print(f"head {i}: loss {float(t['loss']):.7f} stored {term:.7f} tol {8 * U * abs(term):.3e}")
        assert abs(float(t["loss"]) - term) <= 8 * U * abs(term)
    assert abs(float(z["terms"].sum()) - float(z["loss"])) <= 4 * U * float(z["loss"])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp32_emulation_stays_inside_the_bounds(case):
    B, h, w, s, nc, ld = case
    buf, lab = deepsup_inputs(case)
    g = 1.0 / 37.0
    b = bounds(buf[..., :nc].double(), lab, s, g=g)
    e = emulate_fp32(buf, lab, s, nc, g)
    assert bool(((e["lse"].double() - b["lse"]).abs() <= b["E_lse"]).all())
    assert bool(((e["row"].double() - b["row"]).abs() <= b["E_row"]).all())
    assert bool(((e["partial"][:, 0].double() - b["partial"][:, 0]).abs() <= b["E_partial"]).all())
    assert torch.equal(e["partial"][:, 1].double(), b["partial"][:, 1])
    assert bool(((e["dl"][..., :nc].double() - b["dl"]).abs() <= b["E_dl"]).all())
    assert bool((e["dl"][..., nc:] == 0).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_variants_leave_the_bounds(variant):
    """each wrong formulation of the twin differs from the right one by more than the bounds in some case and quantity"""
    hit = []
    for case, cid in zip(CASES, CASE_IDS):
        B, h, w, s, nc, ld = case
        buf, lab = deepsup_inputs(case)
        x64 = buf[..., :nc].double()
        good = bounds(x64, lab, s)
        bad = bounds(x64, lab, s, variant=variant)
        out = dict(lse=bool(((bad["lse"] - good["lse"]).abs() > good["E_lse"]).any()),
                   partial=bool(((bad["partial"][:, 0] - good["partial"][:, 0]).abs() > good["E_partial"]).any()),
                   count=not torch.equal(bad["partial"][:, 1], good["partial"][:, 1]),
                   loss=abs(float(bad["loss"]) - float(good["loss"])) > good["E_loss"],
                   dl=bool(((bad["dl"] - good["dl"]).abs() > good["E_dl"]).any()))
        hit += [(cid, k) for k, v in out.items() if v]
    assert hit, variant
    if variant != "count_all":          # the interpolation variants must show in the kernels' own outputs
        assert any(k in ("lse", "dl") for _, k in hit), hit


def test_model_keys_with_and_without_the_flag():
    meta, z = load_model_golden("tiny_64x96_ds")
    model = build_ds_model(meta["num_classes"], meta["H"], meta["W"])
    assert sorted(model.state_dict().keys()) == [str(k) for k in z["keys"]]
    assert model.deep_supervision is True and model.decode_head.deep_supervision is True
    assert [m.normalized_shape[0] for m in model.decode_head.norm_ds] == [384, 192, 96]
    assert [tuple(m.weight.shape) for m in model.decode_head.output_ds] == [(9, 384, 1, 1), (9, 192, 1, 1), (9, 96, 1, 1)]
    from sigma_amd import train_step as ts
    assert ts.unoptimized_parameters(model.decode_head.norm_ds, ts.group_weight(model, 6e-5)) == 0
    assert ts.unoptimized_parameters(model.decode_head.output_ds, ts.group_weight(model, 6e-5)) == 0
    # without the flag: what the model has always been (the fixture of the default model holds the reference's keys)
    _, z0 = load_model_golden("tiny_64x96")
    plain = build_model("sigma_tiny", 9, 64, 96)
    assert sorted(plain.state_dict().keys()) == [str(k) for k in z0["keys"]]
    assert plain.deep_supervision is False and plain.decode_head.deep_supervision is False
    assert not hasattr(plain.decode_head, "norm_ds") and not hasattr(plain.decode_head, "output_ds")
    extra = set(model.state_dict()) - set(plain.state_dict())
    assert extra and all(".norm_ds." in k or ".output_ds." in k for k in extra)


def test_flag_refuses_sizes_that_do_not_halve_five_times():
    with pytest.raises(ValueError, match="72x88"):
        build_ds_model(5, 72, 88)
    model = build_ds_model(9, 64, 96)
    with pytest.raises(ValueError, match="72x88"):
        model(torch.zeros(1, 3, 72, 88), torch.zeros(1, 3, 72, 88))


def test_expand_logits_is_the_twin_and_differentiable_on_the_cpu():
    from sigma_amd.models.decoders.MambaDecoder import expand_logits
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 5, 9, generator=g).requires_grad_(True)
    out = expand_logits(z, 8)
    assert tuple(out.shape) == (2, 9, 24, 40)
    ref = upsample(z.detach().double(), 8).permute(0, 3, 1, 2)
    assert float((out.detach().double() - ref).abs().max()) <= 4 * U * float(z.detach().abs().max())
    go = torch.randn(out.shape, generator=g)
    out.backward(go)
    from tests.deepsup_fp64_twin import adjoint
    gref = adjoint(go.double().permute(0, 2, 3, 1), 3, 5, 8)
    assert float((z.grad.double() - gref).abs().max()) <= (256 + 2) * U * float(adjoint(go.double().abs().permute(0, 2, 3, 1), 3, 5, 8).max())


def test_interpolation_matrices_built_under_inference_mode_are_not_kept():
    """an evaluation under torch.inference_mode() must not leave inference tensors behind for a later training step"""
    from sigma_amd.models.decoders import MambaDecoder as md
    key = (3, 7, torch.device("cpu"), torch.float32)
    md._INTERP.pop(key, None)
    with torch.inference_mode():
        U_inf = md.interp_matrix(3, 7, "cpu")
    assert key not in md._INTERP and U_inf.is_inference()
    z = torch.randn(1, 3, 3, 4, requires_grad=True)
    md.expand_logits(z, 7).sum().backward()                 # a training step afterwards saves the matrices for its backward
    assert key in md._INTERP and not md._INTERP[key].is_inference() and torch.equal(md._INTERP[key], U_inf)
    assert z.grad is not None


def test_struct_layout_matches_header(tmp_path):
    cname, cls = "sigma_upsample_ce_params", _capi.UpsampleCeParams
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
    assert _capi.SIGMA_SCAN_ABI_VERSION == 13 and _capi.load().sigma_scan_abi_version() == 13      # additions only
    assert "sigma_upsample_ce_fwd" in header and "sigma_upsample_ce_bwd" in header
    assert {"sigma_upsample_ce_fwd", "sigma_upsample_ce_bwd"} <= set(_capi.OPS_SYMBOLS)


def _good_params():
    """arguments both directions accept; the addresses are never dereferenced on the host"""
    p = _capi.UpsampleCeParams()
    p.batch, p.height, p.width, p.scale, p.classes, p.ld, p.ignore_index = 2, 3, 5, 8, 9, 12, 255
    p.logits, p.labels, p.lse, p.partial, p.scale_grad, p.dlogits = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    return p


REFUSED = [("classes", 0), ("classes", 65), ("ld", 10), ("ld", 8), ("scale", 0), ("scale", 33), ("batch", 0), ("height", 0),
           ("width", -1), ("logits", None), ("labels", None), ("lse", None), ("logits", 0x1004), ("labels", 0x2004), ("lse", 0x3002)]


@pytest.mark.parametrize("field,value", REFUSED, ids=[f"{f}={v}" for f, v in REFUSED])
def test_refused_arguments_return_err_arg_without_a_device(field, value):
    lib = _capi.load()
    for fn in (lib.sigma_upsample_ce_fwd, lib.sigma_upsample_ce_bwd):
        p = _good_params()
        setattr(p, field, value)
        assert_refused(fn, ctypes.byref(p), None, says=field)


def test_refused_sizes_and_direction_specific_pointers():
    lib = _capi.load()
    for fn in (lib.sigma_upsample_ce_fwd, lib.sigma_upsample_ce_bwd):
        assert_refused(fn, None, None, says="NULL")
        p = _good_params()                             # 2^31 fine pixels: one more than the kernels index
        p.batch, p.height, p.width, p.scale = 2, 1024, 1024, 32
        assert_refused(fn, ctypes.byref(p), None, says="fine pixels")
        p.batch, p.height, p.width, p.scale = 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 32
        assert_refused(fn, ctypes.byref(p), None, says="pixels")
    for fn, field, bad in ((lib.sigma_upsample_ce_fwd, "partial", None), (lib.sigma_upsample_ce_fwd, "partial", 0x4002),
                           (lib.sigma_upsample_ce_bwd, "scale_grad", None), (lib.sigma_upsample_ce_bwd, "scale_grad", 0x5001),
                           (lib.sigma_upsample_ce_bwd, "dlogits", None), (lib.sigma_upsample_ce_bwd, "dlogits", 0x6008)):
        p = _good_params()
        setattr(p, field, bad)
        assert_refused(fn, ctypes.byref(p), None, says=field)


def test_kernel_family_is_one_forward_and_one_backward_template(tmp_path):
    """deepsup.hip compiles to ten kernels: upsample_loss_fwd_kernel and upsample_loss_bwd_kernel, each instantiated for
    the plain criterion (without weights only) and for the option and focal criteria without and with class weights --
    and no second pair of templates beside them.  None of the ten keeps anything in scratch memory."""
    from sigma_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f"no hipcc at {build.HIPCC}")
    if shutil.which("c++filt") is None:
        pytest.skip("no c++filt")
    out = tmp_path / "deepsup.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.check_call([build.HIPCC, *flags, "--offload-device-only", "-S", os.path.join(build.CSRC, "deepsup.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    kernels = re.findall(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", out.read_text(), re.M | re.S)
    assert len(kernels) == len({n for n, _ in kernels}) == 10 == 2 * (1 + 2 * 2)
    names = subprocess.run(["c++filt"], input="\n".join(n for n, _ in kernels), capture_output=True, text=True).stdout.split("\n")
    inst = sorted(m.groups() for n in names for m in [re.search(r"::(\w+)<\(.*?UpLoss\)(\d), (true|false)>\(", n)] if m)
    kinds = [("0", "false"), ("1", "false"), ("1", "true"), ("2", "false"), ("2", "true")]       # kUpPlain, kUpOpt, kUpFocal
    assert inst == [(t, k, hw) for t in ("upsample_loss_bwd_kernel", "upsample_loss_fwd_kernel") for k, hw in kinds]
    for name, desc in kernels:
        (size,) = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
        assert int(size) == 0 and ".amdhsa_uses_dynamic_stack 0" in desc, name


def test_front_end_declines_cpu_tensors():
    from sigma_amd.pointwise import upsampled_cross_entropy
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    assert upsampled_cross_entropy(crit, torch.zeros(1, 2, 2, 12), 4, torch.zeros(1, 8, 8, dtype=torch.long)) is None
