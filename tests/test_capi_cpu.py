"""CPU-side checks of the C-ABI library: it loads, exports every symbol that
include/sigma_scan.h declares, and its host-side validation behaves like the reference's
TORCH_CHECKs -- all without touching a GPU (no compute entry point is reached)."""
import ctypes
import os
import re

import pytest

from sigma_amd import _capi
from tests.capi_refusals import assert_refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_abi_version():
    lib = _capi.load()
    assert lib.sigma_scan_abi_version() == _capi.SIGMA_SCAN_ABI_VERSION


def test_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "sigma_scan.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+|int64_t\s+)(sigma_\w+)\s*\(", header, flags=re.M))
    assert declared == set(_capi.EXPORTED_SYMBOLS), declared ^ set(_capi.EXPORTED_SYMBOLS)
    lib = _capi.load()
    for name in declared:
        assert getattr(lib, name) is not None
    ops = open(os.path.join(ROOT, "include", "sigma_ops.h")).read()
    declared_ops = set(re.findall(r"^\s*int\s+(sigma_\w+)\s*\(", ops, flags=re.M))
    assert declared_ops == set(_capi.OPS_SYMBOLS), declared_ops ^ set(_capi.OPS_SYMBOLS)
    for name in declared_ops:
        assert getattr(lib, name) is not None
    gemm = open(os.path.join(ROOT, "include", "sigma_gemm.h")).read()
    declared_gemm = set(re.findall(r"^\s*(?:int|int64_t)\s+(sigma_\w+)\s*\(", gemm, flags=re.M))
    assert declared_gemm == set(_capi.GEMM_SYMBOLS) | set(_capi.GEMM_AUX_SYMBOLS), declared_gemm ^ set(_capi.GEMM_SYMBOLS)
    for name in declared_gemm:
        assert getattr(lib, name) is not None


def test_struct_layout_matches_header(tmp_path):
    """Compile include/sigma_scan.h with gcc and compare sizeof/offsetof of every field with the
    ctypes mirror in sigma_amd/_capi.py."""
    import subprocess
    lines = []
    structs = tuple(_capi.STRUCTS.items())
    # every struct the three headers define has a mirror, each mirror stands under one name, and no mirror is left out
    typedefs = {n for h in ("sigma_scan.h", "sigma_ops.h", "sigma_gemm.h")
                for n in re.findall(r"^\}\s*(sigma_\w+)\s*;", open(os.path.join(ROOT, "include", h)).read(), flags=re.M)}
    assert typedefs == set(_capi.STRUCTS) and len(typedefs) >= 13, typedefs ^ set(_capi.STRUCTS)
    mirrors = {v for v in vars(_capi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert mirrors == set(_capi.STRUCTS.values()) and len(mirrors) == len(structs)
    for cname, cls in structs:
        lines.append(f'printf("%s %zu\\n", "{cname}", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("%s.%s %zu\\n", "{cname}", "{fname}", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sigma_scan.h"\n#include "sigma_ops.h"\n#include "sigma_gemm.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == ctypes.sizeof(cls)
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


HEADERS = ("sigma_scan.h", "sigma_ops.h", "sigma_gemm.h")
_RESTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def _prototypes():
    """{name: (return type, [parameter declarations])} of every function the three headers declare"""
    out = {}
    for h in HEADERS:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for ret, name, params in re.findall(r"^\s*(const\s+char\s*\*|int64_t|int)\s*(sigma_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
            params = " ".join(params.split())
            assert name not in out, name
            out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [q.strip() for q in params.split(",")])
    return out


def test_signature_table_matches_the_prototypes():
    """Every row of _capi.SIGNATURES against its prototype: the parameter count, the struct behind every
    ``const sigma_X *`` parameter, the return type -- and no row without a prototype, no prototype without a row."""
    protos = _prototypes()
    assert set(protos) == set(_capi.SIGNATURES), set(protos) ^ set(_capi.SIGNATURES)
    assert len(protos) >= 50
    n_struct = 0
    for name, (ret, params) in protos.items():
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is _RESTYPES[ret], name
        assert len(argtypes) == len(params), (name, params)
        for i, decl in enumerate(params):
            m = re.fullmatch(r"(?:const\s+)?(sigma_\w+)\s*\*\s*\w+", decl)
            if m:
                assert argtypes[i] is ctypes.POINTER(_capi.STRUCTS[m.group(1)]), (name, i, decl)
                n_struct += 1
            else:
                assert "sigma_" not in decl, (name, decl)          # a struct parameter the pattern above did not take
                assert not any(argtypes[i] is ctypes.POINTER(cls) for cls in _capi.STRUCTS.values()), (name, i, decl)
    pointers = {ctypes.POINTER(cls) for cls in _capi.STRUCTS.values()}
    assert n_struct == sum(a in pointers for _, args in _capi.SIGNATURES.values() for a in args) > 0
    # the public tuples are the table's groups: a symbol cannot be listed without a signature, or the reverse
    groups = (_capi.EXPORTED_SYMBOLS, _capi.OPS_SYMBOLS, _capi.OPS_AUX_SYMBOLS, _capi.GEMM_SYMBOLS, _capi.GEMM_AUX_SYMBOLS)
    assert sorted(n for g in groups for n in g) == sorted(_capi.SIGNATURES)


def test_binding_is_complete_after_load():
    lib = _capi.load()
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == list(argtypes) and all(a is b for a, b in zip(fn.argtypes, argtypes)), name


def _params(**kw):
    p = _capi.FwdParams()
    p.batch, p.dim, p.seqlen, p.dstate, p.n_groups = 1, 8, 100, 4, 2
    p.n_chunks = 1
    p.io_dtype = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_host_validation_without_gpu():
    lib = _capi.load()
    assert_refused(lib.sigma_selective_scan_fwd, None, None, says="NULL")      # NULL params
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(io_dtype=7)), None) == 3
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(n_groups=3)), None) == 2   # dim % groups
    assert "dividable" in _capi.last_error()
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(dstate=257)), None) == 2
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(n_chunks=2)), None) == 2
    assert_refused(lib.sigma_selective_scan_fwd, ctypes.byref(_params()), None, says="non-NULL")      # NULL tensors
    # empty problems are a no-op success (nothing is launched)
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(seqlen=0, n_chunks=0)), None) == 0
    assert lib.sigma_selective_scan_fwd(ctypes.byref(_params(batch=0)), None) == 0


def test_options_and_launch_plan():
    lib = _capi.load()
    with pytest.raises(RuntimeError):
        _capi.set_option("fwd_items", 8)
    with pytest.raises(RuntimeError):
        _capi.set_option("no_such_option", 1)
    assert _capi.get_option("no_such_option") == -1
    for gone in ("rl_chain", "rl_chain_timeouts"):        # the chained walk of the row-lane backward was removed (ABI 13)
        with pytest.raises(RuntimeError):
            _capi.set_option(gone, 0)
        assert _capi.get_option(gone) == -1
    plan = (ctypes.c_int32 * 6)()
    # headline shape (1, 768, 19200), N=16, G=4: few rows -> the sequence is split inside the workgroup
    p = _params(batch=1, dim=768, seqlen=19200, dstate=16, n_groups=4, n_chunks=10)
    assert lib.sigma_scan_fwd_plan(ctypes.byref(p), ctypes.byref(plan)) == 0
    items, rows, grid, lds, tiles, nb = list(plan)
    assert items in (4, 5, 10, 20) and 1 <= rows <= 16 and 1 <= rows * tiles <= 16 and nb in (1, 2, 4, 8)
    assert (768 // 4) % rows == 0 and grid == 768 // rows and lds <= 160 * 1024
    assert tiles > 1 and grid >= 128          # one image per GPU still fills the chip
    # the same launch on the row-lane kernels (ckpt_pitch 16): 12 row blocks are cut into segments so that no CU holds a
    # workgroup more than the others (round 6: 48 segments = 576 workgroups, three on 64 CUs and two on the rest, ran 170 us;
    # 40-42 segments = 480-504, two at most, 149-152 us) -- and the dominant training launch is not cut at all
    for b, d, L, n, g in ((1, 768, 19200, 16, 4), (2, 768, 19200, 16, 4), (1, 1536, 4800, 16, 4), (2, 3072, 1200, 16, 4)):
        pr = _params(batch=b, dim=d, seqlen=L, dstate=n, n_groups=g, n_chunks=(L + 2047) // 2048)
        pr.ckpt_pitch = 16
        assert lib.sigma_scan_fwd_plan(ctypes.byref(pr), ctypes.byref(plan)) == 0
        assert plan[0] == 16 and plan[5] == -200 and plan[4] > 1 and plan[2] == b * (d // 64) * plan[4]
        assert 384 <= plan[2] <= 512 or plan[2] % 256 == 0, list(plan)
    pr = _params(batch=16, dim=3072, seqlen=1200, dstate=16, n_groups=4, n_chunks=1)
    pr.ckpt_pitch = 16
    assert lib.sigma_scan_fwd_plan(ctypes.byref(pr), ctypes.byref(plan)) == 0 and plan[4] == 1 and plan[2] == 768
    # a training batch has enough rows: no sequence split; long 16-state rows take 1280-element tiles ...
    pb = _params(batch=16, dim=768, seqlen=19200, dstate=16, n_groups=4, n_chunks=10)
    assert lib.sigma_scan_fwd_plan(ctypes.byref(pb), ctypes.byref(plan)) == 0
    assert plan[0] == 20 and plan[1] == 12 and plan[4] == 1 and plan[2] == 16 * 768 // 12
    # ... short ones 640-element tiles, 8 rows per workgroup, two workgroups per CU
    pc = _params(batch=16, dim=3072, seqlen=1200, dstate=16, n_groups=4, n_chunks=1)
    assert lib.sigma_scan_fwd_plan(ctypes.byref(pc), ctypes.byref(plan)) == 0
    assert plan[0] == 10 and plan[1] == 8 and plan[4] == 1 and 2 * plan[3] <= 160 * 1024
    # few-state scans (fusion / decoder): 16 rows share one B/C stage
    pd = _params(batch=8, dim=768, seqlen=19200, dstate=4, n_groups=4, n_chunks=10)
    assert lib.sigma_scan_fwd_plan(ctypes.byref(pd), ctypes.byref(plan)) == 0
    assert plan[0] == 10 and plan[1] == 16 and plan[4] == 1
    _capi.set_option("fwd_waves", 16)
    try:
        assert lib.sigma_scan_fwd_plan(ctypes.byref(p), ctypes.byref(plan)) == 0
        assert plan[1] == 16 and plan[2] == 48 and plan[4] == 1
    finally:
        _capi.set_option("fwd_waves", 0)
    # reference unit-test shape: 24 rows, 2 groups -> 12 rows per group; L = 372 -> tiles of 5 x 64 or 4 x 64
    p = _params(batch=2, dim=24, seqlen=372, dstate=8, n_groups=2, n_chunks=1)
    assert lib.sigma_scan_fwd_plan(ctypes.byref(p), ctypes.byref(plan)) == 0
    assert 12 % plan[1] == 0 and plan[2] == 48 // plan[1]
    bp = _capi.BwdParams()
    bp.fwd = p
    assert lib.sigma_scan_bwd_plan(ctypes.byref(bp), ctypes.byref(plan)) == 0
    assert plan[0] in (4, 5, 10) and plan[3] <= 160 * 1024 and 12 % plan[1] == 0
    # P = 12 / rows partial slabs of (B, G, N, L) for each of dB, dC (none when one workgroup owns the group)
    P = 12 // plan[1]
    assert lib.sigma_scan_bwd_workspace_bytes(ctypes.byref(bp)) == (0 if P == 1 else 2 * P * 2 * 2 * 8 * 372 * 4)
    # extension fields are validated
    bad = _params(batch=1, dim=8, seqlen=64, dstate=4, n_groups=2, n_chunks=1)
    bad.rev_group_mask = 0b100
    assert lib.sigma_scan_fwd_plan(ctypes.byref(bad), ctypes.byref(plan)) != 0


def test_operator_module_raises_without_gpu_tensors():
    import torch
    from sigma_amd import selective_scan_cuda_core as core
    u = torch.randn(1, 8, 16)
    A = -torch.rand(8, 4)
    Bm = torch.randn(1, 1, 4, 16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        core.fwd(u, u, A, Bm, Bm, None, None, False, 1)


def test_gemm_workspace_query_is_host_side_planning():
    """sigma_gemm_workspace_bytes needs no GPU: the scratch of the two-stage sums follows from the launch geometry --
    reduction slices x output bytes for a weight gradient (tn), problems per output for shared outputs (c_mod), nothing
    when every work item owns its output; bad arguments answer -1."""
    lib = _capi.load()

    def params(M, N, K, lda, ldb, ldc, **kw):
        p = _capi.GemmParams()
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
        p.A, p.Bt, p.C = 0x10000, 0x20000, 0x30000          # never dereferenced by the query (16-byte aligned non-null)
        p.batch, p.pieces = kw.pop("batch", 1), 2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    q = lambda p, form: int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), form))
    # forward / input gradient of a linear layer: every tile owns its output
    assert q(params(19200, 1536, 384, 384, 384, 1536), 0) == 0
    assert q(params(19200, 384, 1536, 1536, 384, 384), 1) == 0
    # weight gradient of the stage-2 in_proj (19200 tokens, 1536 x 384): 36 tiles -> 14 slices in one round of 512 workgroups
    assert q(params(19200, 1536, 384, 1536, 384, 384), 2) == 14 * 1536 * 384 * 4
    # few tokens: one slice, no scratch
    assert q(params(200, 72, 44, 72, 44, 44), 2) == 0
    # the sliced nn form (dW_x = dx^T x with dx channel-major): 768 x 384 output, 19200-long reduction
    need = q(params(768, 384, 19200, 19200, 384, 384, k_slices=1), 1)
    assert need > 0 and need % (768 * 384 * 4) == 0 and need // (768 * 384 * 4) <= 512 // 18
    # shared outputs: 32 problems summed into 2 outputs of 112 x 768 -> 16 parts per output
    sh = params(112, 768, 1200, 1200, 1200, 768, batch=32, c_mod=2, strideA=112 * 1200, strideB=768 * 1200, strideC=112 * 768, accumulate=1)
    assert q(sh, 0) == 2 * 16 * 112 * 768 * 4
    # bad arguments
    assert_refused(q, params(19200, 1536, 384, 384, 384, 1536), 7, code=-1, says="form")
    bad = params(19200, 1536, 383, 384, 384, 1536)
    assert_refused(q, bad, 0, code=-1, says="K")


def test_gemm_ragged_shared_outputs_and_transposed_range_are_planned_on_the_host():
    """Two C-ABI answers decided before any launch: ragged shared outputs (batch % c_mod != 0) ask for scratch sized by
    ceil(batch / c_mod) parts per output -- the query used to answer 0, "no scratch needed", and the launch then fell
    back to atomics onto a C the caller had not zero-filled; c_mod >= batch changes nothing (every problem owns its
    output): the sliced nn form of a single problem asks for the scratch of ONE output whatever c_mod says.  The t_cols
    part pins the accepted contract (a single problem's strideC is not checked; what t_cols cannot take is refused, -1,
    by the query as by the launch); that such a strideC no longer reaches the direct epilogue is a GPU matter
    (tests/test_gemm_gpu.py::test_transposed_column_range_ignores_the_batch_stride_of_a_single_problem)."""
    lib = _capi.load()

    def params(M, N, K, lda, ldb, ldc, **kw):
        p = _capi.GemmParams()
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
        p.A, p.Bt, p.C = 0x10000, 0x20000, 0x30000          # never dereferenced by the query (16-byte aligned non-null)
        p.batch, p.pieces = kw.pop("batch", 1), 2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    q = lambda p, form: int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), form))
    M, N, K = 32, 192, 1200
    for form in (0, 1):
        for Z, cm in ((5, 2), (7, 3), (3, 2), (6, 4)):
            p = params(M, N, K, K, K if form == 0 else N, N, batch=Z, c_mod=cm, strideA=M * K, strideB=N * K, strideC=M * N)
            assert q(p, form) == cm * -(-Z // cm) * M * N * 4, (form, Z, cm)
        # batch <= c_mod: every problem owns its output
        assert q(params(M, N, K, K, K, N, batch=2, c_mod=2, strideA=M * K, strideB=N * K, strideC=M * N), form) == 0
    # sliced nn, one problem: the scratch of its slices for one output, for any c_mod (c_mod >= batch = no sharing)
    base = q(params(64, 64, 19200, 19200, 64, 64, k_slices=1), 1)
    assert base > 0 and base % (64 * 64 * 4) == 0
    for cm in (1, 2, 4):
        assert q(params(64, 64, 19200, 19200, 64, 64, k_slices=1, c_mod=cm, strideC=64 * 64), 1) == base, cm
    Ct = 0x40000
    tc = params(64, 128, 32, 32, 32, 96, Ct=Ct, ldct=64, t_cols=32)
    for sC in (0, 2, 3, 96):
        tc.strideC = sC
        assert q(tc, 0) == 0, sC
    for field, value in (("batch", 2), ("t_cols", 48), ("ldct", 60), ("accumulate", 1), ("M", 66), ("ldc", 98)):
        bad = params(64, 128, 32, 32, 32, 96, Ct=Ct, ldct=64, t_cols=32, strideC=2)
        setattr(bad, field, value)
        if field == "batch":
            bad.strideA, bad.strideB = 64 * 32, 128 * 32
        assert_refused(q, bad, 0, code=-1, says="t_cols", msg=field)


def test_gemm_plan_reports_the_kernel_variant_on_the_host():
    """sigma_gemm_plan (include/sigma_gemm.h): tile width, tiles, slices, kernel variant, epilogue and residual load kind,
    from the planning code of the entry points, without a GPU"""
    def params(M, N, K, lda, ldb, ldc, **kw):
        p = _capi.GemmParams()
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
        p.A, p.Bt, p.C = 0x10000, 0x20000, 0x30000          # never dereferenced (16-byte aligned non-null)
        p.batch, p.pieces = kw.pop("batch", 1), kw.pop("pieces", 2)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    plan = _capi.gemm_plan
    a = plan(params(19200, 1536, 384, 384, 384, 1536), "nt")                 # in_proj of stage 2
    assert (a["bn"], a["ntm"], a["ntn"], a["slices"], a["items"]) == (128, 150, 12, 1, 1800)
    assert (a["pieces"], a["res"], a["epilogue"], a["store"], a["res_load"], a["summed"]) == (2, False, "rows", "store", "none", False)
    assert plan(params(3000, 192, 96, 96, 96, 192), "nt")["bn"] == 96
    assert plan(params(1001, 36, 68, 68, 68, 36), "nt")["bn"] == 64
    assert plan(params(257, 70, 100, 100, 100, 70, pieces=3), "nt") == dict(a, bn=96, ntm=3, ntn=1, items=3, slice_k=128, pieces=3, epilogue="direct")
    # the weight gradient of the stage-2 in_proj: 14 slices (the workspace query above); two-stage only with the scratch
    w = params(19200, 1536, 384, 1536, 384, 384)
    t = plan(w, "tn")
    assert (t["bn"], t["ntm"], t["ntn"], t["slices"], t["items"]) == (128, 12, 3, 14, 504) and t["slice_k"] * 14 >= 19200 > t["slice_k"] * 13
    assert (t["summed"], t["two_stage"], t["store"], t["epilogue"]) == (True, False, "atomic", "direct")
    w.workspace, w.workspace_bytes = 0x50000, 14 * 1536 * 384 * 4
    t = plan(w, "tn")
    assert (t["summed"], t["two_stage"], t["store"], t["epilogue"], t["reduce_vec"]) == (True, True, "store", "rows", True)
    w.workspace_bytes -= 1
    assert plan(w, "tn")["store"] == "atomic"
    # accumulate, a misaligned C, residuals as vector and as scalar loads
    r = params(300, 768, 1536, 1536, 1536, 768, accumulate=1, residual=0x60000, ldr=768)
    got = plan(r, "nt")
    assert (got["res"], got["res_load"], got["epilogue"], got["store"]) == (True, "vector", "rows", "accumulate")
    r.ldr, r.C = 770, 0x30004
    got = plan(r, "nt")
    assert (got["res_load"], got["epilogue"]) == ("scalar", "direct")
    assert plan(params(257, 70, 100, 100, 100, 70, residual=0x60000, ldr=70), "nt")["res_load"] == "scalar"
    x = plan(params(64, 128, 32, 32, 32, 96, Ct=0x40000, ldct=64, t_cols=32, strideC=2), "nt")
    assert x["epilogue"] == "transposed"
    # refused as the launch refuses: unknown form, K % 4, residuals with three pieces or on tn, a bias on tn
    assert plan(params(19200, 1536, 384, 384, 384, 1536), 7) is None
    assert plan(params(19200, 1536, 383, 384, 384, 1536), "nt") is None
    assert plan(params(300, 768, 1536, 1536, 1536, 768, residual=0x60000, ldr=768, pieces=3), "nt") is None
    assert plan(params(300, 768, 1536, 768, 1536, 1536, residual=0x60000, ldr=1536), "tn") is None
    assert plan(params(300, 768, 1536, 768, 1536, 1536, bias=0x70000), "tn") is None
    assert plan(params(300, 768, 1536, 768, 1536, 1536), "tn") is not None
    assert plan(params(0, 768, 1536, 1536, 1536, 768), "nt")["items"] == 0       # empty: nothing is launched
    # Refusals that belong to the plan, so the launch, the plan query and the size query give ONE answer, before any HIP
    # call (the pointers are fake): SIGMA_OPS_ERR_ARG, SIGMA_OPS_ERR_ARG, -1.  The launch used to find out on its own way
    # to the kernel (SIGMA_OPS_ERR_LAUNCH) and the size query answered 0, "fine, no scratch".
    lib = _capi.load()

    def answers(p, form):
        f, out = _capi.GEMM_FORMS[form], (ctypes.c_int32 * 8)()
        planned = int(lib.sigma_gemm_plan(ctypes.byref(p), f, ctypes.byref(out)))
        assert planned != 0, "accepted: not launched on the fake pointers"
        # the three answers, each with a reason of its own in the error text -- the same one, as they share the plan
        reasons = [assert_refused(lib.sigma_gemm_plan, ctypes.byref(p), f, ctypes.byref(out), code=planned),
                   assert_refused(getattr(lib, f"sigma_gemm_{form}_split3"), ctypes.byref(p), None, code=planned),
                   assert_refused(lib.sigma_gemm_workspace_bytes, ctypes.byref(p), f, code=-1)]
        assert len(set(reasons)) == 1, reasons
        return (int(getattr(lib, f"sigma_gemm_{form}_split3")(ctypes.byref(p), None)), planned, int(lib.sigma_gemm_workspace_bytes(ctypes.byref(p), f)))

    for form, ldb in (("nt", 1536), ("nn", 768)):
        # a residual with three pieces: no such kernel
        assert answers(params(300, 768, 1536, 1536, ldb, 768, residual=0x60000, ldr=768, pieces=3), form) == (1, 1, -1), form
        assert plan(params(300, 768, 1536, 1536, ldb, 768, residual=0x60000, ldr=768), form)["res"], form    # two pieces: fine
        # more than 2^31 - 1 work items: 2^30 + 1 tiny problems of two row tiles each (2^30 - 1 of them are 2^31 - 2 items)
        many = dict(strideA=256 * 4, strideB=4 * 4, strideC=256 * 4)
        assert answers(params(256, 4, 4, 4, 4, 4, batch=2**30 + 1, **many), form) == (1, 1, -1), form
        assert plan(params(256, 4, 4, 4, 4, 4, batch=2**30 - 1, **many), form)["items"] == 2**31 - 2, form
