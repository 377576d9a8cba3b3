"""Host side of the classifier head and loss for class counts that are no multiple of 4 (MFNet 9, PST900 5, SUN-RGBD 37):
the padding helpers of sigma_amd/gemm.py, the argument checks of sigma_softmax_ce_fwd_ld / _bwd_ld and their ctypes
signatures against include/sigma_ops.h -- no GPU, no launch is reached."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn

from sigma_amd import _capi
from tests.capi_refusals import assert_refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sigma_softmax_ce_fwd_ld", "sigma_softmax_ce_bwd_ld")


def test_cross_entropy_still_declines_cpu_tensors():
    from sigma_amd.pointwise import cross_entropy
    crit = nn.CrossEntropyLoss(reduction="mean", ignore_index=255)
    label = torch.zeros(2, 3, 5, dtype=torch.long)
    for nc, ld in ((9, 12), (5, 8), (40, 40), (9, 9)):
        buf = torch.randn(2, 3, 5, ld)
        assert cross_entropy(crit, buf[..., :nc].permute(0, 3, 1, 2), label) is None


@pytest.mark.parametrize("nc", range(1, 71))
def test_padding_helpers(nc):
    """ld = 4 ceil(nc / 4); the padded weight is the weight followed by exact zero rows and is no parameter; the weight
    gradient handed back is the contiguous first nc rows in the parameter's shape"""
    from sigma_amd import gemm
    C = 8
    ld = gemm.padded_classes(nc)
    assert ld % 4 == 0 and nc <= ld < nc + 4
    conv = nn.Conv2d(C, nc, kernel_size=1, bias=False)
    wp = gemm.pad_rows(conv.weight.view(nc, -1), ld)
    assert tuple(wp.shape) == (ld, C) and wp.is_contiguous() and not isinstance(wp, nn.Parameter)
    assert torch.equal(wp[:nc], conv.weight.detach().view(nc, C))
    assert wp[nc:].numel() == (ld - nc) * C and not wp[nc:].any()
    assert (torch.signbit(wp[nc:]) == 0).all()                  # +0.0, not -0.0
    dwp = torch.randn(ld, C)
    dw = gemm.unpad_rows(dwp, conv.weight.shape)
    assert tuple(dw.shape) == tuple(conv.weight.shape) and dw.is_contiguous() and dw.stride() == conv.weight.stride()
    assert torch.equal(dw.view(nc, C), dwp[:nc])
    assert [n for n, _ in conv.named_parameters()] == ["weight"]


def test_decoder_keeps_its_parameters_and_state_dict_keys():
    from sigma_amd.models.decoders.MambaDecoder import MambaDecoder

    def keys(nc):
        m = MambaDecoder(img_size=(64, 96), in_channels=(32, 64, 128, 256), num_classes=nc, embed_dim=32, depths=(1, 1, 1, 1))
        assert tuple(m.output.weight.shape) == (nc, 32, 1, 1)
        return sorted(m.state_dict()), sorted(n for n, _ in m.named_parameters()), sorted(n for n, _ in m.named_buffers())

    want = keys(40)
    for nc in (5, 9, 37):
        assert keys(nc) == want


def _null():
    return ctypes.c_void_p(None)


def test_new_entry_points_check_their_arguments_before_any_launch():
    lib = _capi.load()
    ERR = 1                                                      # SIGMA_OPS_ERR_ARG
    ok = ctypes.c_void_p(0x10000)                                # 16-byte aligned, never dereferenced: every call below is refused
    odd = ctypes.c_void_p(0x10004)

    def fwd_status(rows=8, classes=9, ld=12, logits=ok, labels=ok, lse=ok, partial=ok):
        return lib.sigma_softmax_ce_fwd_ld(logits, labels, rows, classes, ld, 255, lse, partial, _null())

    def bwd_status(rows=8, classes=9, ld=12, logits=ok, labels=ok, lse=ok, scale=ok, dl=ok):
        return lib.sigma_softmax_ce_bwd_ld(logits, labels, lse, scale, rows, classes, ld, 255, dl, _null())

    # fwd / bwd: the status of a call that must be refused -- with a reason of its own in the error text (assert_refused)
    fwd = lambda **kw: assert_refused(lambda: fwd_status(**kw), code=ERR, msg=kw) and ERR
    bwd = lambda **kw: assert_refused(lambda: bwd_status(**kw), code=ERR, msg=kw) and ERR

    for f in (fwd, bwd):
        assert f(ld=10) == ERR and f(ld=9) == ERR and f(ld=13) == ERR           # ld % 4 != 0
        assert f(ld=8) == ERR and f(classes=13) == ERR                          # ld < classes
        assert f(classes=0) == ERR and f(classes=-3) == ERR                     # classes < 1
        assert f(rows=-1) == ERR
        assert f(logits=_null()) == ERR and f(labels=_null()) == ERR and f(lse=_null()) == ERR
        assert f(logits=odd) == ERR                                             # alignment
    assert fwd(partial=_null()) == ERR and fwd(rows=0, partial=_null()) == ERR
    assert bwd(scale=_null()) == ERR and bwd(dl=_null()) == ERR and bwd(dl=odd) == ERR
    assert bwd_status(rows=0, logits=_null(), dl=_null()) == 0                  # nothing to write: success without a launch
    # the contiguous entry points still want classes % 4 == 0
    assert_refused(lib.sigma_softmax_ce_fwd, ok, ok, 8, 9, 255, ok, ok, _null(), says="classes")
    assert_refused(lib.sigma_softmax_ce_bwd, ok, ok, ok, ok, 8, 9, 255, ok, _null(), says="classes")


_CTYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def _declared(name):
    """the parameter types of `name` as include/sigma_ops.h declares it"""
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", header, flags=re.M)
    assert m, name
    types = []
    for arg in m.group(1).split(","):
        t = re.sub(r"\w+$", "", arg.strip()).strip()               # drop the parameter's name
        types.append(re.sub(r"\s+", " ", t).replace(" *", "*"))
    return types


def test_ctypes_signatures_match_the_header(tmp_path):
    """A C file redeclares both functions from the types this test read out of the header -- the compiler rejects a
    redeclaration that conflicts with sigma_ops.h -- and prints every parameter's size; those and the pointer / integer
    kinds are what _capi.load() gives ctypes."""
    lib = _capi.load()
    decls, prints = [], []
    for name in NEW:
        types = _declared(name)
        decls.append(f"int {name}({', '.join(types)});")
        for i, t in enumerate(types):
            prints.append(f'printf("{name} {i} %zu\\n", sizeof({t}));')
    src = tmp_path / "sig.c"
    src.write_text('#include <stdio.h>\n#include "sigma_ops.h"\n' + "\n".join(decls) + "\nint main(void){" + "".join(prints) + "return 0;}")
    exe = tmp_path / "sig"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        n, i, s = line.split()
        sizes[(n, int(i))] = int(s)
    for name in NEW:
        types = _declared(name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(types), name
        for i, (t, ct) in enumerate(zip(types, fn.argtypes)):
            assert ctypes.sizeof(ct) == sizes[(name, i)], (name, i, t)
            assert ct is (ctypes.c_void_p if t.endswith("*") else _CTYPES[t]), (name, i, t)
    assert [t for t in _declared(NEW[0]) if not t.endswith("*")] == ["int64_t", "int32_t", "int32_t", "int64_t"]
    assert [t for t in _declared(NEW[1]) if not t.endswith("*")] == ["int64_t", "int32_t", "int32_t", "int64_t"]


def test_header_says_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    assert "added under ABI 13" in header
    assert _capi.SIGMA_SCAN_ABI_VERSION == 13 and _capi.load().sigma_scan_abi_version() == 13


def test_head_launches_open_no_census_key():
    """host planning (sigma_gemm_plan, sigma_gemm_workspace_bytes): the three GEMMs of the padded head at the token counts
    of 720x1280 (batch 1), 480x640 (batch 2 and 8) and 64x96, C = 128 / 96, 5 / 9 / 37 classes, take kernel variants that
    tests/test_stream_fp64_gpu.py's census already maps to an fp64 case"""
    import tests.test_stream_fp64_gpu as census
    from sigma_amd import gemm
    lib = _capi.load()

    def params(M, N, K, lda, ldb, ldc):
        p = _capi.GemmParams()
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
        p.A, p.Bt, p.C = 0x10000, 0x20000, 0x30000               # never dereferenced (16-byte aligned non-null)
        p.batch, p.pieces = 1, 2
        return p

    for M in (921600, 614400, 2457600, 6144):
        for C in (128, 96):
            for nc in (5, 9, 37):
                ld = gemm.padded_classes(nc)
                want = {"nt": (64, "rows", "own"), "nn": (C, "rows", "own"), "tn": (C, "rows", "two-stage")}
                for form, p in (("nt", params(M, ld, C, C, C, ld)), ("nn", params(M, C, ld, ld, C, C)), ("tn", params(M, ld, C, ld, C, C))):
                    need = int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), _capi.GEMM_FORMS[form]))
                    if need > 0:
                        p.workspace, p.workspace_bytes = 0x50000, need
                    key = census.launch_key(lib, f"sigma_gemm_{form}_split3", (ctypes.byref(p), None))
                    assert key[-3:] == want[form], (M, C, nc, form, key)
                    assert key in census.COVERED, (M, C, nc, form, key)
